/* replay_bc_rs.c — the call sequence of the reference's algo.betweenness procedure (algo_procedures.rs:925-1017, the
 * unlabelled run), issued call for call through the GraphBLAS + LAGraph C ABI (declarations: lagraph_subset.h /
 * graphblas_subset.h, transcribed from the bindgen output; LAGr_Betweenness below, lagraph_bindings.rs:539-546) against
 * falkordb_amd/lib/{liblagraphx,liblagraph,libgraphblas}.so:
 *   GxB_init with the caller's allocator + LAGraph_Init (matrix.rs:126-183); GrB_Matrix_dup of the adjacency and
 *   GrB_Matrix_resize to node_count + deleted (:928-932); LAGraph_New(DIRECTED) taking ownership (:942); LAGraph_Cached_AT +
 *   LAGraph_Cached_OutDegree (:945-946); LAGr_Betweenness (:977-983); GrB_Vector_nvals + GrB_Vector_extractTuples_FP64
 *   (extract_vector_f64); GrB_Vector_free and LAGraph_Delete (:992-993); LAGraph_Finalize.
 * Input (text, argv[1]): n nnz, nnz "row col" pairs, then commands "bc <n_resized> <ns> <s_1> ... <s_ns>".
 * Output per command: "bc <n_resized> nvals <k>" and k lines "<index> <score>" (%.17g); then "no_at <info>" (LAGr_Betweenness
 * on a directed graph without G->AT), "bad_source <info>" (a source >= n), "adjacency <nnz>" and "allocator_blocks <live>"
 * (tests/test_gpu_bc_shim.py). */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "lagraph_subset.h"

int LAGr_Betweenness(GrB_Vector* centrality, LAGraph_Graph G, const GrB_Index* sources, int32_t ns, char* msg);

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

static LAGraph_Graph directed_copy(GrB_Matrix adj, GrB_Index n_resized) {
    char msg[LAGRAPH_MSG_LEN];
    GrB_Matrix raw = NULL;
    OK(GrB_Matrix_dup(&raw, adj));
    OK(GrB_Matrix_resize(raw, n_resized, n_resized));
    LAGraph_Graph g = NULL;
    OK(LAGraph_New(&g, &raw, LAGraph_ADJACENCY_DIRECTED, msg));                   /* create_lagraph_graph: G owns the duplicate */
    return g;
}

static void run_bc(GrB_Matrix adj, GrB_Index n_resized, const GrB_Index* src, int32_t ns) {
    char msg[LAGRAPH_MSG_LEN];
    LAGraph_Graph g = directed_copy(adj, n_resized);
    LAGraph_Cached_AT(g, msg);                                                    /* :945-946, return codes ignored */
    LAGraph_Cached_OutDegree(g, msg);
    GrB_Vector centrality = NULL;
    OK(LAGr_Betweenness(&centrality, g, src, ns, msg));
    GrB_Index nvals = 0;
    OK(GrB_Vector_nvals(&nvals, centrality));
    GrB_Index* idx = malloc((nvals + 1) * sizeof(GrB_Index));
    double* val = malloc((nvals + 1) * sizeof(double));
    GrB_Index got = nvals;
    OK(GrB_Vector_extractTuples_FP64(idx, val, &got, centrality));
    printf("bc %llu nvals %llu\n", (unsigned long long)n_resized, (unsigned long long)got);
    for (GrB_Index k = 0; k < got; ++k) printf("%llu %.17g\n", (unsigned long long)idx[k], val[k]);
    free(idx); free(val);
    OK(GrB_Vector_free(&centrality));
    OK(LAGraph_Delete(&g, msg));
    if (g != NULL) { fprintf(stderr, "LAGraph_Delete left the handle\n"); exit(2); }
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
        if (!strcmp(cmd, "bc")) {
            unsigned long long nr;
            int ns;
            if (fscanf(f, "%llu %d", &nr, &ns) != 2 || ns < 0) return 3;
            GrB_Index* src = malloc(((size_t)ns + 1) * sizeof(GrB_Index));
            for (int k = 0; k < ns; ++k) {
                unsigned long long v;
                if (fscanf(f, "%llu", &v) != 1) return 3;
                src[k] = v;
            }
            run_bc(adj, nr, src, ns);
            free(src);
        } else {
            return 3;
        }
    }
    /* a directed graph without G->AT: LAGRAPH_NOT_CACHED; a source >= n: GrB_INVALID_INDEX */
    {
        LAGraph_Graph g = directed_copy(adj, n);
        GrB_Vector c = NULL;
        GrB_Index src[2] = {0, 0};
        printf("no_at %d\n", LAGr_Betweenness(&c, g, src, 1, msg));
        LAGraph_Cached_AT(g, msg);
        src[1] = n;
        printf("bad_source %d\n", LAGr_Betweenness(&c, g, src, 2, msg));
        if (c != NULL) { fprintf(stderr, "a failed call left a vector\n"); exit(2); }
        OK(LAGraph_Delete(&g, msg));
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
