/* graphblas_msf_subset.h — the C declarations algo.MSF adds to the two subset headers, TRANSCRIBED from the reference's bindgen
 * output (graph/src/graph/graphblas/mod.rs and lagraphx_bindings.rs; the line of each `pub fn` / `pub static` is cited).
 * tests/shim/replay_msf_rs.c is written against this file, lagraph_subset.h and graphblas_subset.h only. */
#ifndef GRAPHBLAS_MSF_SUBSET_H
#define GRAPHBLAS_MSF_SUBSET_H
#include "lagraph_subset.h"

extern GrB_Type GrB_FP64;                                     /* mod.rs:550 */
extern GrB_BinaryOp GrB_MIN_FP64;                             /* mod.rs:1964 */
GrB_Info GrB_Matrix_build_FP64(GrB_Matrix C, const GrB_Index* I, const GrB_Index* J, const double* X, GrB_Index nvals,
                               GrB_BinaryOp dup);             /* mod.rs:9609 */
GrB_Info GrB_Matrix_setElement_FP64(GrB_Matrix C, double x, GrB_Index i, GrB_Index j);        /* mod.rs:9765 */
GrB_Info GrB_Matrix_extractElement_FP64(double* x, GrB_Matrix A, GrB_Index i, GrB_Index j);   /* mod.rs:9877 */
GrB_Info GrB_Matrix_extractTuples_FP64(GrB_Index* I, GrB_Index* J, double* X, GrB_Index* nvals, GrB_Matrix A);   /* mod.rs:10021 */
int LAGraph_msf(GrB_Matrix* forest_edges, GrB_Vector* componentId, GrB_Matrix A, bool sanitize, char* msg);   /* lagraphx_bindings.rs:261-267 */
#endif
