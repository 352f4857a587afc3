/* graphblas_maxflow_subset.h — the C declarations algo.maxFlow adds to the subset headers, TRANSCRIBED from the reference's
 * bindgen output (graph/src/graph/graphblas/mod.rs, lagraph_bindings.rs and lagraphx_bindings.rs; the line of each `pub fn` /
 * `pub static` is cited).  tests/shim/replay_maxflow_rs.c is written against this file, graphblas_msf_subset.h,
 * lagraph_subset.h and graphblas_subset.h only. */
#ifndef GRAPHBLAS_MAXFLOW_SUBSET_H
#define GRAPHBLAS_MAXFLOW_SUBSET_H
#include "graphblas_msf_subset.h"

enum { LAGraph_VALUE = 0, LAGraph_BOUND = 1, LAGraph_STATE_UNKNOWN = -1 };   /* LAGraph_State, lagraph_bindings.rs:99-105 */
extern GrB_BinaryOp GrB_MAX_FP64;                             /* mod.rs:1967 */
int LAGraph_Cached_EMin(LAGraph_Graph G, char* msg);          /* lagraph_bindings.rs:234-237 */
int LAGr_MaxFlow(double* f, GrB_Matrix* flow_mtx, GrB_Matrix* res_mtx, LAGraph_Graph G, GrB_Index src, GrB_Index sink,
                 char* msg);                                  /* lagraphx_bindings.rs:610-618 */
#endif
