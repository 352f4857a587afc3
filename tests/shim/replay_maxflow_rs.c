/* replay_maxflow_rs.c — the GraphBLAS + LAGraph calls of the reference's algo.maxFlow procedure around its solve
 * (algo_procedures.rs:3112-3216), issued through the C ABI (declarations: graphblas_maxflow_subset.h, graphblas_msf_subset.h,
 * lagraph_subset.h, graphblas_subset.h, transcribed from the bindgen output) against
 * falkordb_amd/lib/{liblagraphx,liblagraph,libgraphblas}.so:
 *   GxB_init with the caller's allocator + LAGraph_Init (matrix.rs:126-183); GrB_Matrix_new(GrB_FP64, n, n) (:3121);
 *   GrB_Matrix_build_FP64(.., GrB_MAX_FP64) (:3141-3148) + GrB_Matrix_wait (:3150); LAGraph_New(DIRECTED) over the borrowed
 *   matrix (create_lagraph_graph, :3152-3155); LAGraph_Cached_AT + LAGraph_Cached_EMin (:3157-3158); LAGr_MaxFlow(&f, &flow_mtx,
 *   NULL, G, src, sink, msg) (:3161-3170); G->A = NULL + LAGraph_Delete (delete_lagraph_graph, :3172); GrB_Matrix_nvals +
 *   GrB_Matrix_extractTuples_FP64 on flow_mtx (:3183-3196); GrB_Matrix_free (:3197); LAGraph_Finalize.
 * Input (text, argv[1]): n narcs, narcs lines "u v <capacity bits, hex>" (a position may repeat: GrB_MAX_FP64 keeps the largest),
 * then commands: "flow <src> <sink>", "boolflow <src> <sink>" (the same pattern as a GrB_BOOL matrix), "errors <src> <sink>".
 * Output per flow command: "flow <value bits, hex> nvals <k> emin <emin != NULL> <emin_state>", k lines "<row> <col> <flow bits,
 * hex>"; per errors command one line "errors <name> <code> ..." each; then "capacities <nnz>" and "allocator_blocks <live>"
 * (tests/test_gpu_maxflow_shim.py). */
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "graphblas_maxflow_subset.h"

#define OK(call)                                                                       \
    do {                                                                               \
        int info_ = (int)(call);                                                       \
        if (info_ != 0) { fprintf(stderr, "%s -> %d (line %d)\n", #call, info_, __LINE__); exit(2); } \
    } while (0)

static size_t live_blocks = 0;                                /* the allocator matrix::init hands to GxB_init */
static void* my_malloc(size_t n) { ++live_blocks; return malloc(n); }
static void* my_calloc(size_t a, size_t b) { ++live_blocks; return calloc(a, b); }
static void* my_realloc(void* p, size_t n) { if (!p) ++live_blocks; return realloc(p, n); }
static void my_free(void* p) { if (p) --live_blocks; free(p); }

/* create_lagraph_graph: the graph borrows the matrix (LAGraph_New moves the handle in, the caller keeps its own copy) */
static LAGraph_Graph graph_over(GrB_Matrix m) {
    char msg[LAGRAPH_MSG_LEN];
    LAGraph_Graph g = NULL;
    GrB_Matrix moved = m;
    OK(LAGraph_New(&g, &moved, LAGraph_ADJACENCY_DIRECTED, msg));
    if (moved != NULL || g->A != m) { fprintf(stderr, "LAGraph_New did not move the matrix in\n"); exit(2); }
    return g;
}
static void drop_graph(LAGraph_Graph* g) {                    /* delete_lagraph_graph */
    char msg[LAGRAPH_MSG_LEN];
    (*g)->A = NULL;
    OK(LAGraph_Delete(g, msg));
}

static void run_flow(GrB_Matrix cap, GrB_Index src, GrB_Index sink) {
    char msg[LAGRAPH_MSG_LEN];
    GrB_Index n = 0;
    OK(GrB_Matrix_nrows(&n, cap));
    LAGraph_Graph g = graph_over(cap);
    OK(LAGraph_Cached_AT(g, msg));                                                /* :3157 */
    OK(LAGraph_Cached_EMin(g, msg));                                              /* :3158 */
    OK(LAGraph_Cached_EMin(g, msg));                                              /* (a second call leaves it alone) */
    const int has_emin = g->emin != NULL, emin_state = (int)g->emin_state;
    double f = -1.0;
    GrB_Matrix flow = NULL;
    OK(LAGr_MaxFlow(&f, &flow, NULL, g, src, sink, msg));                         /* :3161-3170 */
    drop_graph(&g);                                                               /* :3172 */
    if (!flow) { fprintf(stderr, "flow_mtx is NULL\n"); exit(2); }
    GrB_Index nf = 0, fn = 0, fm = 0;
    OK(GrB_Matrix_nvals(&nf, flow));                                              /* :3183-3196 */
    OK(GrB_Matrix_nrows(&fn, flow));
    OK(GrB_Matrix_ncols(&fm, flow));
    if (fn != n || fm != n) { fprintf(stderr, "flow_mtx is %llu x %llu\n", (unsigned long long)fn, (unsigned long long)fm); exit(2); }
    GrB_Index* fr = malloc((nf + 1) * sizeof(GrB_Index));
    GrB_Index* fc = malloc((nf + 1) * sizeof(GrB_Index));
    double* fv = malloc((nf + 1) * sizeof(double));
    GrB_Index got = nf;
    OK(GrB_Matrix_extractTuples_FP64(fr, fc, fv, &got, flow));
    uint64_t b;
    memcpy(&b, &f, sizeof b);
    printf("flow %016" PRIx64 " nvals %llu emin %d %d\n", b, (unsigned long long)got, has_emin, emin_state);
    for (GrB_Index k = 0; k < got; ++k) {
        memcpy(&b, &fv[k], sizeof b);
        printf("%llu %llu %016" PRIx64 "\n", (unsigned long long)fr[k], (unsigned long long)fc[k], b);
    }
    free(fr); free(fc); free(fv);
    OK(GrB_Matrix_free(&flow));                                                   /* :3197 */
}

static void run_errors(GrB_Matrix cap, GrB_Index src, GrB_Index sink) {
    char msg[LAGRAPH_MSG_LEN];
    GrB_Index n = 0;
    OK(GrB_Matrix_nrows(&n, cap));
    double f = -1.0;
    GrB_Matrix flow = (GrB_Matrix)&n, res = (GrB_Matrix)&n;
    LAGraph_Graph g = graph_over(cap);
    msg[0] = 0;
    int code = LAGr_MaxFlow(&f, &flow, NULL, g, src, sink, msg);
    printf("errors uncached_at %d %d %s\n", code, flow == NULL, strlen(msg) ? "message" : "silent");
    OK(LAGraph_Cached_AT(g, msg));
    flow = (GrB_Matrix)&n; msg[0] = 0;
    code = LAGr_MaxFlow(&f, &flow, NULL, g, src, sink, msg);
    printf("errors uncached_emin %d %d %s\n", code, flow == NULL, strlen(msg) ? "message" : "silent");
    OK(LAGraph_Cached_EMin(g, msg));
    flow = (GrB_Matrix)&n;
    code = LAGr_MaxFlow(&f, &flow, NULL, g, n, sink, msg);
    printf("errors bad_src %d %d\n", code, flow == NULL);
    flow = (GrB_Matrix)&n;
    code = LAGr_MaxFlow(&f, &flow, NULL, g, src, n + 7, msg);
    printf("errors bad_sink %d %d\n", code, flow == NULL);
    flow = (GrB_Matrix)&n;
    code = LAGr_MaxFlow(&f, &flow, NULL, g, src, src, msg);
    printf("errors src_is_sink %d %d\n", code, flow == NULL);
    flow = (GrB_Matrix)&n; msg[0] = 0;
    code = LAGr_MaxFlow(&f, &flow, &res, g, src, sink, msg);
    printf("errors res_mtx %d %d %d %s\n", code, flow == NULL, res == NULL, strlen(msg) ? "message" : "silent");
    flow = (GrB_Matrix)&n;
    code = LAGr_MaxFlow(&f, &flow, NULL, NULL, src, sink, msg);
    printf("errors null_graph %d %d\n", code, flow == NULL);
    code = LAGraph_Cached_EMin(NULL, msg);
    printf("errors emin_null_graph %d\n", code);
    f = -1.0;
    OK(LAGr_MaxFlow(&f, NULL, NULL, g, src, sink, msg));                          /* flow_mtx is nullable */
    uint64_t b;
    memcpy(&b, &f, sizeof b);
    printf("errors null_flow_mtx 0 %016" PRIx64 "\n", b);
    drop_graph(&g);
    /* an empty matrix: no smallest entry to cache, the flow is 0 and empty */
    GrB_Matrix e = NULL;
    OK(GrB_Matrix_new(&e, GrB_FP64, 5, 5));
    g = graph_over(e);
    OK(LAGraph_Cached_AT(g, msg));
    OK(LAGraph_Cached_EMin(g, msg));
    const int has = g->emin != NULL, state = (int)g->emin_state;
    flow = NULL;
    OK(LAGr_MaxFlow(&f, &flow, NULL, g, 0, 4, msg));
    GrB_Index nf = 9;
    OK(GrB_Matrix_nvals(&nf, flow));
    printf("errors empty_matrix 0 %d %d %g %llu\n", has, state, f, (unsigned long long)nf);
    OK(GrB_Matrix_free(&flow));
    drop_graph(&g);
    OK(GrB_Matrix_free(&e));
    /* a UINT64 matrix carries edge ids, not capacities */
    OK(GrB_Matrix_new(&e, GrB_UINT64, 5, 5));
    g = graph_over(e);
    code = LAGraph_Cached_EMin(g, msg);
    printf("errors uint64_matrix %d\n", code);
    drop_graph(&g);
    OK(GrB_Matrix_free(&e));
    /* GrB_MAX_FP64 keeps the larger of two values at one position */
    OK(GrB_Matrix_new(&e, GrB_FP64, 4, 4));
    GrB_Index di[3] = {0, 0, 2}, dj[3] = {1, 1, 3};
    double dx[3] = {-2.5, 5.0, 7.0}, got = 0;
    OK(GrB_Matrix_build_FP64(e, di, dj, dx, 3, GrB_MAX_FP64));
    OK(GrB_Matrix_extractElement_FP64(&got, e, 0, 1));
    OK(GrB_Matrix_nvals(&nf, e));
    printf("errors build_dup_max 0 %g %llu\n", got, (unsigned long long)nf);
    OK(GrB_Matrix_free(&e));
}

int main(int argc, char** argv) {
    if (argc < 2) return 1;
    FILE* in = fopen(argv[1], "r");
    if (!in) return 1;
    unsigned long long n = 0, na = 0;
    if (fscanf(in, "%llu %llu", &n, &na) != 2) return 3;
    char msg[LAGRAPH_MSG_LEN];
    OK(GxB_init(GrB_NONBLOCKING, my_malloc, my_calloc, my_realloc, my_free));    /* matrix.rs:126-135 */
    OK(LAGraph_Init(msg));                                                        /* matrix.rs:174-183 */
    GrB_Index* I = malloc((na + 1) * sizeof(GrB_Index));
    GrB_Index* J = malloc((na + 1) * sizeof(GrB_Index));
    double* X = malloc((na + 1) * sizeof(double));
    bool* B = malloc((na + 1) * sizeof(bool));
    for (unsigned long long k = 0; k < na; ++k) {
        unsigned long long i, j;
        uint64_t b;
        if (fscanf(in, "%llu %llu %" SCNx64, &i, &j, &b) != 3) return 3;
        I[k] = i; J[k] = j; B[k] = true;
        memcpy(&X[k], &b, sizeof b);
    }
    GrB_Matrix cap = NULL, pat = NULL;
    OK(GrB_Matrix_new(&cap, GrB_FP64, n, n));                                     /* :3121 */
    if (na) OK(GrB_Matrix_build_FP64(cap, I, J, X, na, GrB_MAX_FP64));            /* :3141-3148 */
    OK(GrB_Matrix_wait(cap, GrB_COMPLETE));                                       /* :3150 */
    OK(GrB_Matrix_new(&pat, GrB_BOOL, n, n));
    if (na) OK(GrB_Matrix_build_BOOL(pat, I, J, B, na, GxB_ANY_BOOL));
    OK(GrB_Matrix_wait(pat, GrB_COMPLETE));
    free(I); free(J); free(X); free(B);
    char cmd[32];
    unsigned long long s, t;
    while (fscanf(in, "%31s %llu %llu", cmd, &s, &t) == 3) {
        if (!strcmp(cmd, "flow")) run_flow(cap, s, t);
        else if (!strcmp(cmd, "boolflow")) run_flow(pat, s, t);
        else if (!strcmp(cmd, "errors")) run_errors(cap, s, t);
        else return 3;
    }
    GrB_Index still = 0;
    OK(GrB_Matrix_nvals(&still, cap));
    printf("capacities %llu\n", (unsigned long long)still);
    OK(GrB_Matrix_free(&cap));
    OK(GrB_Matrix_free(&pat));
    OK(LAGraph_Finalize(msg));                                                    /* matrix.rs:215-221 */
    printf("allocator_blocks %llu\n", (unsigned long long)live_blocks);
    fclose(in);
    return 0;
}
