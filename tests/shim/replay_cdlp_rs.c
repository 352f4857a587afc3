/* replay_cdlp_rs.c — the call sequence of the reference's algo.labelPropagation procedure (algo_procedures.rs:1207-1261, the
 * unlabelled run), issued call for call through the GraphBLAS + LAGraph C ABI (declarations: lagraph_subset.h /
 * graphblas_subset.h, transcribed from the bindgen output) against falkordb_amd/lib/{liblagraphx,liblagraph,libgraphblas}.so:
 *   GxB_init with the caller's allocator + LAGraph_Init (matrix.rs:126-183); GrB_Matrix_dup of the symmetric adjacency and
 *   GrB_Matrix_resize to node_count + deleted (:1208-1212); LAGraph_New(UNDIRECTED) taking ownership; is_symmetric_structure =
 *   TRUE (:1225-1229); LAGraph_cdlp (lagraphx_bindings.rs:218-223); GrB_Vector_nvals + GrB_Vector_extractTuples_INT64
 *   (extract_vector_i64); GrB_Vector_free and LAGraph_Delete (:1260-1261); LAGraph_Finalize.
 * Input (text, argv[1]): n nnz, nnz "row col" pairs (the symmetric pattern), then commands: "cdlp <n_resized> <itermax>", or
 * "errors" (a directed graph of unknown symmetry, a negative itermax, NULL handles).
 * Output per cdlp command: "cdlp <n_resized> nvals <k>" and k lines "<index> <label>"; per errors command one line
 * "errors <name> <code> <handle is NULL> [message|silent]" each; then "adjacency <nnz>" and "allocator_blocks <live>"
 * (tests/test_gpu_cdlp_shim.py). */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "lagraph_subset.h"

/* the one prototype lagraph_subset.h lacks (lagraphx_bindings.rs:218-223) */
int LAGraph_cdlp(GrB_Vector* CDLP_handle, LAGraph_Graph G, int itermax, char* msg);

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

static void run_cdlp(GrB_Matrix adj, GrB_Index n_resized, int itermax) {
    char msg[LAGRAPH_MSG_LEN];
    GrB_Matrix raw = NULL;
    OK(GrB_Matrix_dup(&raw, adj));                                                /* :1208-1212 */
    OK(GrB_Matrix_resize(raw, n_resized, n_resized));
    LAGraph_Graph g = NULL;
    OK(LAGraph_New(&g, &raw, LAGraph_ADJACENCY_UNDIRECTED, msg));                 /* create_lagraph_graph: G owns the duplicate */
    g->is_symmetric_structure = LAGraph_TRUE;                                     /* :1225-1229 */
    GrB_Vector component = NULL;
    OK(LAGraph_cdlp(&component, g, itermax, msg));
    GrB_Index nvals = 0;
    OK(GrB_Vector_nvals(&nvals, component));
    GrB_Index* idx = malloc((nvals + 1) * sizeof(GrB_Index));
    int64_t* val = malloc((nvals + 1) * sizeof(int64_t));
    GrB_Index got = nvals;
    OK(GrB_Vector_extractTuples_INT64(idx, val, &got, component));
    printf("cdlp %llu nvals %llu\n", (unsigned long long)n_resized, (unsigned long long)got);
    for (GrB_Index k = 0; k < got; ++k) printf("%llu %lld\n", (unsigned long long)idx[k], (long long)val[k]);
    free(idx); free(val);
    OK(GrB_Vector_free(&component));
    OK(LAGraph_Delete(&g, msg));
    if (g != NULL) { fprintf(stderr, "LAGraph_Delete left the handle\n"); exit(2); }
}

static void run_errors(GrB_Matrix adj) {
    char msg[LAGRAPH_MSG_LEN];
    GrB_Matrix raw = NULL;
    OK(GrB_Matrix_dup(&raw, adj));
    LAGraph_Graph g = NULL;
    OK(LAGraph_New(&g, &raw, LAGraph_ADJACENCY_DIRECTED, msg));                   /* symmetry unknown: refused, loudly */
    GrB_Vector v = (GrB_Vector)&g;
    msg[0] = 0;
    int r = LAGraph_cdlp(&v, g, 10, msg);
    printf("errors directed %d %d %s\n", r, v == NULL, strlen(msg) ? "message" : "silent");
    g->is_symmetric_structure = LAGraph_TRUE;                                     /* the caller's promise makes it acceptable */
    v = (GrB_Vector)&g;
    r = LAGraph_cdlp(&v, g, -1, msg);
    printf("errors negative_itermax %d %d\n", r, v == NULL);
    r = LAGraph_cdlp(NULL, g, 10, msg);
    printf("errors null_handle %d\n", r);
    v = (GrB_Vector)&g;
    r = LAGraph_cdlp(&v, NULL, 10, msg);
    printf("errors null_graph %d %d\n", r, v == NULL);
    v = NULL;
    OK(LAGraph_cdlp(&v, g, 0, msg));                                              /* itermax 0: the identity labelling */
    GrB_Index nvals = 0;
    OK(GrB_Vector_nvals(&nvals, v));
    printf("errors zero_itermax 0 %llu\n", (unsigned long long)nvals);
    OK(GrB_Vector_free(&v));
    OK(LAGraph_Delete(&g, msg));
}

int main(int argc, char** argv) {
    if (argc < 2) return 1;
    FILE* f = fopen(argv[1], "r");
    if (!f) return 1;
    unsigned long long n = 0, nnz = 0;
    if (fscanf(f, "%llu %llu", &n, &nnz) != 2) return 3;
    char msg[LAGRAPH_MSG_LEN];
    OK(GxB_init(GrB_NONBLOCKING, my_malloc, my_calloc, my_realloc, my_free));    /* matrix.rs:126-135 */
    OK(LAGraph_Init(msg));                                                        /* matrix.rs:174-183 */
    GrB_Index* I = malloc((nnz + 1) * sizeof(GrB_Index));
    GrB_Index* J = malloc((nnz + 1) * sizeof(GrB_Index));
    for (unsigned long long k = 0; k < nnz; ++k) {
        unsigned long long i, j;
        if (fscanf(f, "%llu %llu", &i, &j) != 2) return 3;
        I[k] = i; J[k] = j;
    }
    GrB_Matrix adj = NULL;
    OK(GrB_Matrix_new(&adj, GrB_BOOL, n, n));
    GrB_Scalar s = NULL;
    OK(GrB_Scalar_new(&s, GrB_BOOL));
    OK(GrB_Scalar_setElement_BOOL(s, true));
    OK(GxB_Matrix_build_Scalar(adj, I, J, s, nnz));
    OK(GrB_Scalar_free(&s));
    OK(GrB_Matrix_wait(adj, GrB_MATERIALIZE));
    free(I); free(J);
    char cmd[32];
    while (fscanf(f, "%31s", cmd) == 1) {
        if (!strcmp(cmd, "cdlp")) {
            unsigned long long nr;
            int itermax;
            if (fscanf(f, "%llu %d", &nr, &itermax) != 2) return 3;
            run_cdlp(adj, nr, itermax);
        } else if (!strcmp(cmd, "errors")) {
            run_errors(adj);
        } else {
            return 3;
        }
    }
    GrB_Index still = 0;
    OK(GrB_Matrix_nvals(&still, adj));                                            /* the caller's adjacency survived LAGraph_Delete */
    printf("adjacency %llu\n", (unsigned long long)still);
    OK(GrB_Matrix_free(&adj));
    OK(LAGraph_Finalize(msg));                                                    /* matrix.rs:215-221 */
    printf("allocator_blocks %llu\n", (unsigned long long)live_blocks);
    fclose(f);
    return 0;
}
