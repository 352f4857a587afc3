/* replay_msf_rs.c — the GraphBLAS + LAGraph calls of the reference's algo.MSF procedure around its forest
 * (algo_procedures.rs:1357-1358, 1704-1744), issued through the C ABI (declarations: graphblas_msf_subset.h, lagraph_subset.h,
 * graphblas_subset.h, transcribed from the bindgen output) against falkordb_amd/lib/{liblagraphx,liblagraph,libgraphblas}.so:
 *   GxB_init with the caller's allocator + LAGraph_Init (matrix.rs:126-183); GrB_Matrix_new(GrB_FP64, n, n) (:1358); the
 *   weighted adjacency built and GrB_Matrix_wait (:1704); LAGraph_msf(&forest_edges, &component_id, weighted_adj, false, msg)
 *   (:1711-1717); GrB_Vector_nvals + GrB_Vector_extractTuples_INT64 on component_id (extract_vector_i64, :1726);
 *   GrB_Matrix_nvals + GrB_Matrix_extractTuples_FP64 on forest_edges (:1729-1741); GrB_Matrix_free / GrB_Vector_free (:1743-1744);
 *   LAGraph_Finalize.  The UDT scoring pipeline in front of the call is not replayed: the weighted matrix is built directly.
 * Input (text, argv[1]): n npairs, npairs lines "lo hi <weight bits, hex>" (each pair is stored in both directions), then
 * commands: "msf" (run on the matrix as it is), "resize <n2>" (GrB_Matrix_resize), "errors".
 * Output per msf command: "msf <n> nvals <k> <ncomp>", k lines "<row> <col> <weight bits, hex>", ncomp lines "<index> <component>";
 * per errors command one line "errors <name> <code> ..." each; then "adjacency <nnz>" and "allocator_blocks <live>"
 * (tests/test_gpu_msf_shim.py). */
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "graphblas_msf_subset.h"

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

static void run_msf(GrB_Matrix w) {
    char msg[LAGRAPH_MSG_LEN];
    GrB_Index n = 0;
    OK(GrB_Matrix_nrows(&n, w));
    GrB_Matrix forest = NULL;
    GrB_Vector comp = NULL;
    OK(LAGraph_msf(&forest, &comp, w, false, msg));                               /* :1711-1717 */
    GrB_Index nc = 0, nf = 0;
    OK(GrB_Vector_nvals(&nc, comp));                                              /* extract_vector_i64 */
    GrB_Index* ci = malloc((nc + 1) * sizeof(GrB_Index));
    int64_t* cv = malloc((nc + 1) * sizeof(int64_t));
    GrB_Index gotc = nc;
    OK(GrB_Vector_extractTuples_INT64(ci, cv, &gotc, comp));
    OK(GrB_Matrix_nvals(&nf, forest));                                            /* :1729-1741 */
    GrB_Index* fr = malloc((nf + 1) * sizeof(GrB_Index));
    GrB_Index* fc = malloc((nf + 1) * sizeof(GrB_Index));
    double* fv = malloc((nf + 1) * sizeof(double));
    GrB_Index gotf = nf;
    OK(GrB_Matrix_extractTuples_FP64(fr, fc, fv, &gotf, forest));
    GrB_Index fn = 0, fm = 0;
    OK(GrB_Matrix_nrows(&fn, forest));
    OK(GrB_Matrix_ncols(&fm, forest));
    if (fn != n || fm != n) { fprintf(stderr, "forest_edges is %llu x %llu\n", (unsigned long long)fn, (unsigned long long)fm); exit(2); }
    printf("msf %llu nvals %llu %llu\n", (unsigned long long)n, (unsigned long long)gotf, (unsigned long long)gotc);
    for (GrB_Index k = 0; k < gotf; ++k) {
        uint64_t b;
        memcpy(&b, &fv[k], sizeof b);
        double again = 0;
        OK(GrB_Matrix_extractElement_FP64(&again, forest, fr[k], fc[k]));
        if (memcmp(&again, &fv[k], sizeof again)) { fprintf(stderr, "extractElement disagrees with extractTuples\n"); exit(2); }
        printf("%llu %llu %016" PRIx64 "\n", (unsigned long long)fr[k], (unsigned long long)fc[k], b);
    }
    for (GrB_Index k = 0; k < gotc; ++k) printf("%llu %lld\n", (unsigned long long)ci[k], (long long)cv[k]);
    free(ci); free(cv); free(fr); free(fc); free(fv);
    OK(GrB_Matrix_free(&forest));                                                 /* :1743-1744 */
    OK(GrB_Vector_free(&comp));
}

static void run_errors(GrB_Matrix w) {
    char msg[LAGRAPH_MSG_LEN];
    GrB_Index n = 0;
    OK(GrB_Matrix_nrows(&n, w));
    GrB_Matrix f = (GrB_Matrix)&n;
    GrB_Vector c = (GrB_Vector)&n;
    int code = LAGraph_msf(NULL, &c, w, false, msg);
    printf("errors null_forest %d %d\n", code, c == NULL);
    f = (GrB_Matrix)&n; c = (GrB_Vector)&n;
    code = LAGraph_msf(&f, &c, NULL, false, msg);
    printf("errors null_a %d %d %d\n", code, f == NULL, c == NULL);
    f = (GrB_Matrix)&n; c = (GrB_Vector)&n; msg[0] = 0;
    code = LAGraph_msf(&f, &c, w, true, msg);
    printf("errors sanitize %d %d %d %s\n", code, f == NULL, c == NULL, strlen(msg) ? "message" : "silent");
    GrB_Matrix u = NULL;
    OK(GrB_Matrix_new(&u, GrB_UINT64, n, n));
    f = (GrB_Matrix)&n; c = (GrB_Vector)&n; msg[0] = 0;
    code = LAGraph_msf(&f, &c, u, false, msg);
    printf("errors uint64_matrix %d %d %d %s\n", code, f == NULL, c == NULL, strlen(msg) ? "message" : "silent");
    OK(GrB_Matrix_free(&u));
    OK(GrB_Matrix_new(&u, GrB_FP64, n, n + 1));
    f = (GrB_Matrix)&n; c = (GrB_Vector)&n;
    code = LAGraph_msf(&f, &c, u, false, msg);
    printf("errors non_square %d %d %d\n", code, f == NULL, c == NULL);
    OK(GrB_Matrix_free(&u));
    f = NULL;
    OK(LAGraph_msf(&f, NULL, w, false, msg));
    GrB_Index nf = 0;
    OK(GrB_Matrix_nvals(&nf, f));
    printf("errors null_component 0 %llu\n", (unsigned long long)nf);
    OK(GrB_Matrix_free(&f));
    /* a BOOL matrix means every weight is 1.0 */
    GrB_Matrix b = NULL;
    OK(GrB_Matrix_new(&b, GrB_BOOL, 3, 3));
    GrB_Index bi[4] = {0, 1, 1, 2}, bj[4] = {1, 0, 2, 1};
    bool bx[4] = {true, true, true, true};
    OK(GrB_Matrix_build_BOOL(b, bi, bj, bx, 4, GxB_ANY_BOOL));
    OK(LAGraph_msf(&f, NULL, b, false, msg));
    double one = 0;
    OK(GrB_Matrix_extractElement_FP64(&one, f, 1, 2));
    OK(GrB_Matrix_nvals(&nf, f));
    printf("errors bool_matrix 0 %llu %g\n", (unsigned long long)nf, one);
    OK(GrB_Matrix_free(&f));
    OK(GrB_Matrix_free(&b));
    /* build with duplicates: GrB_MIN_FP64 keeps the smaller, NULL refuses; setElement overwrites */
    OK(GrB_Matrix_new(&u, GrB_FP64, 4, 4));
    GrB_Index di[3] = {0, 0, 2}, dj[3] = {1, 1, 3};
    double dx[3] = {5.0, -2.5, 7.0};
    code = GrB_Matrix_build_FP64(u, di, dj, dx, 3, NULL);
    printf("errors build_dup_null %d\n", code);
    OK(GrB_Matrix_build_FP64(u, di, dj, dx, 3, GrB_MIN_FP64));
    double got = 0;
    OK(GrB_Matrix_extractElement_FP64(&got, u, 0, 1));
    OK(GrB_Matrix_setElement_FP64(u, -0.0, 2, 3));
    double z = 1;
    OK(GrB_Matrix_extractElement_FP64(&z, u, 2, 3));
    uint64_t zb;
    memcpy(&zb, &z, sizeof zb);
    code = GrB_Matrix_extractElement_FP64(&z, u, 3, 3);
    OK(GrB_Matrix_nvals(&nf, u));
    printf("errors build_dup_min 0 %g %016" PRIx64 " %d %llu\n", got, zb, code, (unsigned long long)nf);
    GrB_Index room = 1;
    code = GrB_Matrix_extractTuples_FP64(di, dj, dx, &room, u);
    printf("errors tuples_no_room %d\n", code);
    OK(GrB_Matrix_free(&u));
}

int main(int argc, char** argv) {
    if (argc < 2) return 1;
    FILE* in = fopen(argv[1], "r");
    if (!in) return 1;
    unsigned long long n = 0, np = 0;
    if (fscanf(in, "%llu %llu", &n, &np) != 2) return 3;
    char msg[LAGRAPH_MSG_LEN];
    OK(GxB_init(GrB_NONBLOCKING, my_malloc, my_calloc, my_realloc, my_free));    /* matrix.rs:126-135 */
    OK(LAGraph_Init(msg));                                                        /* matrix.rs:174-183 */
    GrB_Index* I = malloc((2 * np + 1) * sizeof(GrB_Index));
    GrB_Index* J = malloc((2 * np + 1) * sizeof(GrB_Index));
    double* X = malloc((2 * np + 1) * sizeof(double));
    for (unsigned long long k = 0; k < np; ++k) {
        unsigned long long i, j;
        uint64_t b;
        if (fscanf(in, "%llu %llu %" SCNx64, &i, &j, &b) != 3) return 3;
        I[2 * k] = i; J[2 * k] = j; I[2 * k + 1] = j; J[2 * k + 1] = i;
        memcpy(&X[2 * k], &b, sizeof b);
        memcpy(&X[2 * k + 1], &b, sizeof b);
    }
    GrB_Matrix w = NULL;
    OK(GrB_Matrix_new(&w, GrB_FP64, n, n));                                       /* :1358 */
    OK(GrB_Matrix_build_FP64(w, I, J, X, 2 * np, NULL));
    OK(GrB_Matrix_wait(w, GrB_COMPLETE));                                         /* :1704 */
    free(I); free(J); free(X);
    char cmd[32];
    while (fscanf(in, "%31s", cmd) == 1) {
        if (!strcmp(cmd, "msf")) {
            run_msf(w);
        } else if (!strcmp(cmd, "resize")) {
            unsigned long long nr;
            if (fscanf(in, "%llu", &nr) != 1) return 3;
            OK(GrB_Matrix_resize(w, nr, nr));
        } else if (!strcmp(cmd, "errors")) {
            run_errors(w);
        } else {
            return 3;
        }
    }
    GrB_Index still = 0;
    OK(GrB_Matrix_nvals(&still, w));
    printf("adjacency %llu\n", (unsigned long long)still);
    OK(GrB_Matrix_free(&w));
    OK(LAGraph_Finalize(msg));                                                    /* matrix.rs:215-221 */
    printf("allocator_blocks %llu\n", (unsigned long long)live_blocks);
    fclose(in);
    return 0;
}
