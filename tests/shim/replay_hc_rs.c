/* replay_hc_rs.c — the call sequence of the reference's algo.HarmonicCentrality procedure (algo_procedures.rs:2676-2774, the
 * unlabelled run), issued call for call through the GraphBLAS + LAGraph C ABI (declarations: lagraph_subset.h /
 * graphblas_subset.h, transcribed from the bindgen output) against falkordb_amd/lib/{liblagraphx,liblagraph,libgraphblas}.so:
 *   GxB_init with the caller's allocator + LAGraph_Init (matrix.rs:126-183); GrB_Matrix_new + GrB_Matrix_eWiseMult_BinaryOp(
 *   raw, NULL, NULL, GrB_ONEB_BOOL, adj, adj, NULL), the iso rebuild of the adjacency (:2689-2700); GrB_Matrix_resize to
 *   node_count + deleted (:2701-2702); LAGraph_New(DIRECTED) taking ownership (:2710-2713); GrB_Vector_new(BOOL) +
 *   GrB_Vector_assign_BOOL(true, GrB_ALL) (:2725-2737); LAGr_HarmonicCentrality (lagraphx_bindings.rs:486-492);
 *   GrB_Vector_free(nodes); GrB_Vector_nvals + GrB_Vector_extractTuples_FP64 / _INT64 (extract_vector_f64 / _i64);
 *   GrB_Vector_free x 2 and LAGraph_Delete (:2770-2772); LAGraph_Finalize.
 * Input (text, argv[1]): n nnz, nnz "row col" pairs (the directed pattern), then commands: "hc <n_resized>", or "errors"
 * (NULL scores, node_weights that are not all true or not full, a NULL graph, a NULL reachable_nodes).
 * Output per hc command: "hc <n_resized> nvals <k> <k2>" and k lines "<index> <score %.17g> <reachable>"; per errors command
 * one line "errors <name> <code> ..." each; then "adjacency <nnz>" and "allocator_blocks <live>"
 * (tests/test_gpu_hc_shim.py). */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "lagraph_subset.h"

/* what the two subset headers lack (mod.rs:1232, 3036, 11250-11258, 12005-12013; lagraphx_bindings.rs:486-492) */
extern GrB_BinaryOp GrB_ONEB_BOOL;
extern const GrB_Index* GrB_ALL;
GrB_Info GrB_Matrix_eWiseMult_BinaryOp(GrB_Matrix C, GrB_Matrix Mask, GrB_BinaryOp accum, GrB_BinaryOp mult, GrB_Matrix A,
                                       GrB_Matrix B, GrB_Descriptor desc);
GrB_Info GrB_Vector_assign_BOOL(GrB_Vector w, GrB_Vector mask, GrB_BinaryOp accum, bool x, const GrB_Index* I, GrB_Index ni,
                                GrB_Descriptor desc);
int LAGr_HarmonicCentrality(GrB_Vector* scores, GrB_Vector* reachable_nodes, LAGraph_Graph G, GrB_Vector node_weights, char* msg);

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

static LAGraph_Graph make_graph(GrB_Matrix adj, GrB_Index n_resized) {
    char msg[LAGRAPH_MSG_LEN];
    GrB_Index nrows = 0, ncols = 0;
    OK(GrB_Matrix_nrows(&nrows, adj));
    OK(GrB_Matrix_ncols(&ncols, adj));
    GrB_Matrix raw = NULL;
    OK(GrB_Matrix_new(&raw, GrB_BOOL, nrows, ncols));                             /* :2689-2700 */
    OK(GrB_Matrix_eWiseMult_BinaryOp(raw, NULL, NULL, GrB_ONEB_BOOL, adj, adj, NULL));
    OK(GrB_Matrix_resize(raw, n_resized, n_resized));                             /* :2701-2702 */
    LAGraph_Graph g = NULL;
    OK(LAGraph_New(&g, &raw, LAGraph_ADJACENCY_DIRECTED, msg));                   /* create_lagraph_graph: G owns raw */
    if (raw != NULL) { fprintf(stderr, "LAGraph_New left the matrix handle\n"); exit(2); }
    return g;
}

static GrB_Vector all_true(GrB_Index n) {
    GrB_Vector nodes = NULL;
    OK(GrB_Vector_new(&nodes, GrB_BOOL, n));                                      /* :2725-2737 */
    OK(GrB_Vector_assign_BOOL(nodes, NULL, NULL, true, GrB_ALL, n, NULL));
    GrB_Index nv = 0;
    OK(GrB_Vector_nvals(&nv, nodes));
    if (nv != n) { fprintf(stderr, "GrB_Vector_assign_BOOL left %llu of %llu entries\n", (unsigned long long)nv, (unsigned long long)n); exit(2); }
    return nodes;
}

static void run_hc(GrB_Matrix adj, GrB_Index n_resized) {
    char msg[LAGRAPH_MSG_LEN];
    LAGraph_Graph g = make_graph(adj, n_resized);
    GrB_Vector nodes = all_true(n_resized);
    GrB_Vector scores = NULL, reach = NULL;
    OK(LAGr_HarmonicCentrality(&scores, &reach, g, nodes, msg));
    OK(GrB_Vector_free(&nodes));
    GrB_Index nvals = 0, nvals2 = 0;
    OK(GrB_Vector_nvals(&nvals, scores));
    OK(GrB_Vector_nvals(&nvals2, reach));
    GrB_Index* idx = malloc((nvals + 1) * sizeof(GrB_Index));
    double* val = malloc((nvals + 1) * sizeof(double));
    GrB_Index* idx2 = malloc((nvals2 + 1) * sizeof(GrB_Index));
    int64_t* val2 = malloc((nvals2 + 1) * sizeof(int64_t));
    GrB_Index got = nvals, got2 = nvals2;
    OK(GrB_Vector_extractTuples_FP64(idx, val, &got, scores));
    OK(GrB_Vector_extractTuples_INT64(idx2, val2, &got2, reach));
    printf("hc %llu nvals %llu %llu\n", (unsigned long long)n_resized, (unsigned long long)got, (unsigned long long)got2);
    for (GrB_Index k = 0; k < got && k < got2; ++k) {
        if (idx[k] != idx2[k]) { fprintf(stderr, "the two vectors disagree on index %llu\n", (unsigned long long)k); exit(2); }
        printf("%llu %.17g %lld\n", (unsigned long long)idx[k], val[k], (long long)val2[k]);
    }
    free(idx); free(val); free(idx2); free(val2);
    OK(GrB_Vector_free(&scores));
    OK(GrB_Vector_free(&reach));
    OK(LAGraph_Delete(&g, msg));
    if (g != NULL) { fprintf(stderr, "LAGraph_Delete left the handle\n"); exit(2); }
}

static void run_errors(GrB_Matrix adj) {
    char msg[LAGRAPH_MSG_LEN];
    GrB_Index n = 0;
    OK(GrB_Matrix_nrows(&n, adj));
    LAGraph_Graph g = make_graph(adj, n);
    GrB_Vector nodes = all_true(n);
    GrB_Vector s = (GrB_Vector)&g, r = (GrB_Vector)&g;
    int code = LAGr_HarmonicCentrality(NULL, &r, g, nodes, msg);
    printf("errors null_scores %d %d\n", code, r == NULL);
    /* weights: one false entry; a vector with a missing entry; a vector of another length */
    GrB_Vector w = all_true(n);
    OK(GrB_Vector_free(&w));
    OK(GrB_Vector_new(&w, GrB_BOOL, n));
    for (GrB_Index i = 0; i < n; ++i) OK(GrB_Vector_setElement_BOOL(w, i != 1, i));
    s = (GrB_Vector)&g; r = (GrB_Vector)&g; msg[0] = 0;
    code = LAGr_HarmonicCentrality(&s, &r, g, w, msg);
    printf("errors false_weight %d %d %d %s\n", code, s == NULL, r == NULL, strlen(msg) ? "message" : "silent");
    OK(GrB_Vector_free(&w));
    OK(GrB_Vector_new(&w, GrB_BOOL, n));
    for (GrB_Index i = 0; i + 1 < n; ++i) OK(GrB_Vector_setElement_BOOL(w, true, i));
    s = (GrB_Vector)&g; r = (GrB_Vector)&g; msg[0] = 0;
    code = LAGr_HarmonicCentrality(&s, &r, g, w, msg);
    printf("errors sparse_weights %d %d %d %s\n", code, s == NULL, r == NULL, strlen(msg) ? "message" : "silent");
    OK(GrB_Vector_free(&w));
    w = all_true(n + 1);
    s = (GrB_Vector)&g; r = (GrB_Vector)&g; msg[0] = 0;
    code = LAGr_HarmonicCentrality(&s, &r, g, w, msg);
    printf("errors long_weights %d %d %d %s\n", code, s == NULL, r == NULL, strlen(msg) ? "message" : "silent");
    OK(GrB_Vector_free(&w));
    s = (GrB_Vector)&g; r = (GrB_Vector)&g;
    code = LAGr_HarmonicCentrality(&s, &r, NULL, nodes, msg);
    printf("errors null_graph %d %d %d\n", code, s == NULL, r == NULL);
    /* allowed: no reachable_nodes; NULL weights; a full vector set entry by entry */
    s = NULL;
    OK(LAGr_HarmonicCentrality(&s, NULL, g, nodes, msg));
    GrB_Index nv = 0;
    OK(GrB_Vector_nvals(&nv, s));
    printf("errors null_reachable 0 %llu\n", (unsigned long long)nv);
    OK(GrB_Vector_free(&s));
    OK(LAGr_HarmonicCentrality(&s, &r, g, NULL, msg));
    OK(GrB_Vector_nvals(&nv, r));
    printf("errors null_weights 0 %llu\n", (unsigned long long)nv);
    OK(GrB_Vector_free(&s));
    OK(GrB_Vector_free(&r));
    OK(GrB_Vector_new(&w, GrB_BOOL, n));
    for (GrB_Index i = 0; i < n; ++i) OK(GrB_Vector_setElement_BOOL(w, true, i));
    OK(LAGr_HarmonicCentrality(&s, &r, g, w, msg));
    OK(GrB_Vector_nvals(&nv, s));
    printf("errors set_weights 0 %llu\n", (unsigned long long)nv);
    OK(GrB_Vector_free(&s));
    OK(GrB_Vector_free(&r));
    OK(GrB_Vector_free(&w));
    /* the GraphBLAS forms the procedure does not issue are refused, not guessed */
    GrB_Matrix c = NULL;
    OK(GrB_Matrix_new(&c, GrB_BOOL, n, n));
    code = GrB_Matrix_eWiseMult_BinaryOp(c, NULL, NULL, GxB_ANY_BOOL, adj, adj, NULL);
    printf("errors ewise_other_op %d\n", code);
    OK(GrB_Matrix_free(&c));
    GrB_Index one = 0;
    code = GrB_Vector_assign_BOOL(nodes, NULL, NULL, true, &one, 1, NULL);
    printf("errors assign_index_list %d\n", code);
    OK(GrB_Vector_free(&nodes));
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
        if (!strcmp(cmd, "hc")) {
            unsigned long long nr;
            if (fscanf(f, "%llu", &nr) != 1) return 3;
            run_hc(adj, nr);
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
