// lagraph_shim.cpp — the LAGraph-named part of the tier-2 boundary: `liblagraph.so` / `liblagraphx.so`,
// exporting the LAGraph entry points the reference's BFS / PageRank / WCC / betweenness / labelPropagation / HarmonicCentrality /
// MSF / maxFlow procedures bind, on the MI355X engine.
// With them next to libgraphblas.so (graphblas_shim.cpp) the reference's UNMODIFIED call sequences run on the GPU:
//   algo.BFS       algo_procedures.rs:1060-1165  LAGraph_New (borrowed adjacency, :389-405) -> LAGr_BreadthFirstSearch_Extended
//                  (lagraphx_bindings.rs:585-594; level, parent|NULL, src, max_level, -1, false) -> GrB_Vector_nvals +
//                  GrB_Vector_extractTuples_INT64 on level / parent (:431-447) -> GrB_Vector_free -> G->A = NULL; LAGraph_Delete
//   algo.pageRank  algo_procedures.rs:734-760    LAGraph_New -> LAGraph_Cached_AT + LAGraph_Cached_OutDegree ->
//                  LAGr_PageRank(0.85, 1e-4, 100) (lagraph_bindings.rs:549-558) -> GrB_Vector_extractTuples_FP64 (:415-429)
//   algo.WCC       algo_procedures.rs:816-871    GrB_Matrix_dup + GrB_Matrix_resize -> LAGraph_New(UNDIRECTED), is_symmetric_structure
//                  = TRUE -> LAGr_ConnectedComponents (lagraph_bindings.rs:521-526) -> GrB_Vector_extractTuples_INT64
//   algo.betweenness algo_procedures.rs:925-1017 GrB_Matrix_dup + GrB_Matrix_resize -> LAGraph_New(DIRECTED) -> LAGraph_Cached_AT +
//                  LAGraph_Cached_OutDegree -> LAGr_Betweenness (lagraph_bindings.rs:539-546) -> GrB_Vector_extractTuples_FP64
//   algo.labelPropagation algo_procedures.rs:1207-1261 GrB_Matrix_dup + GrB_Matrix_resize -> LAGraph_New(UNDIRECTED),
//                  is_symmetric_structure = TRUE -> LAGraph_cdlp (lagraphx_bindings.rs:218-223) -> GrB_Vector_extractTuples_INT64
//   algo.HarmonicCentrality algo_procedures.rs:2676-2774 GrB_Matrix_new + GrB_Matrix_eWiseMult_BinaryOp(GrB_ONEB_BOOL, adj, adj) +
//                  GrB_Matrix_resize -> LAGraph_New(DIRECTED) -> GrB_Vector_new + GrB_Vector_assign_BOOL(true, GrB_ALL) ->
//                  LAGr_HarmonicCentrality (lagraphx_bindings.rs:486-492) -> GrB_Vector_extractTuples_FP64 / _INT64
//   algo.MSF       algo_procedures.rs:1357-1358, 1704-1744 GrB_Matrix_new(GrB_FP64) ... GrB_Matrix_wait -> LAGraph_msf(sanitize =
//                  false) (lagraphx_bindings.rs:261-267) -> GrB_Matrix_nvals + GrB_Matrix_extractTuples_FP64 on the forest,
//                  GrB_Vector_extractTuples_INT64 on componentId.  The UDT scoring pipeline in front of the call (GrB_Type_new,
//                  index-unary operators with host callbacks, UDT monoids, :1403-1701) is not part of this boundary: that pair
//                  reduction is what the host layer's algo_msf does
//   algo.maxFlow   algo_procedures.rs:3112-3216  GrB_Matrix_new(GrB_FP64) + GrB_Matrix_build_FP64(GrB_MAX_FP64) + GrB_Matrix_wait ->
//                  LAGraph_New(DIRECTED) -> LAGraph_Cached_AT + LAGraph_Cached_EMin -> LAGr_MaxFlow(&f, &flow_mtx, NULL, G, src,
//                  sink) (lagraphx_bindings.rs:610-618) -> GrB_Matrix_nvals + GrB_Matrix_extractTuples_FP64 on the flow matrix
//   matrix::init / shutdown  matrix.rs:174-183, 215-221  LAGraph_Init after GxB_init, LAGraph_Finalize
// LAGraph itself is an un-vendored dependency (build.rs:50-52 links prebuilt static archives); what is restated here is its
// published contract as the bindings' own doc comments state it (argument meaning, cached-property rules, return codes:
// lagraph_bindings.rs:23-31) — the algorithms are the engine's fgpu_bfs / fgpu_pagerank / fgpu_wcc / fgpu_betweenness /
// fgpu_cdlp / fgpu_harmonic / fgpu_msf / fgpu_maxflow, pinned against the oracle (WCC, betweenness, CDLP, harmonic centrality, MSF
// and max flow against the checkers of their tests).  Every LAGraph entry point algo_procedures.rs calls computes: none answers
// GrB_NOT_IMPLEMENTED for the forms the procedures send.
//
// One source, two libraries: -DFG_LAGRAPHX builds the LAGraphX (experimental) symbols, without it the LAGraph core ones.
#include "shim_internal.hpp"

extern "C" {
GrB_Info GrB_init(int mode);
GrB_Info GrB_finalize();
GrB_Info GrB_Matrix_free(GrB_Matrix* A);
GrB_Info GrB_Vector_free(GrB_Vector* v);
GrB_Info GrB_Scalar_free(GrB_Scalar* s);
}

// LAGraph_Graph_struct, field for field as bindgen lays it out (lagraph_bindings.rs:108-129; 88 bytes — the caller writes
// G->A itself, algo_procedures.rs:409-413)
struct LAGraph_Graph_struct {
    GrB_Matrix A;
    int32_t kind;                     // LAGraph_Kind: 0 undirected, 1 directed, -1 unknown (lagraph_bindings.rs:77-84)
    GrB_Matrix AT;
    GrB_Vector out_degree, in_degree;
    int32_t is_symmetric_structure;   // LAGraph_Boolean: 0 / 1 / -1 unknown
    int64_t nself_edges;
    GrB_Scalar emin;
    int32_t emin_state;
    GrB_Scalar emax;
    int32_t emax_state;
};
static_assert(sizeof(LAGraph_Graph_struct) == 88, "LAGraph_Graph_struct must match the bindgen layout (lagraph_bindings.rs:132)");
typedef LAGraph_Graph_struct* LAGraph_Graph;

enum { LAGRAPH_INVALID_GRAPH = -1000, LAGRAPH_NOT_CACHED = -1003, LAGRAPH_CONVERGENCE_FAILURE = -1005, LAGRAPH_CACHE_NOT_NEEDED = 1000,
       LAGRAPH_UNKNOWN = -1, LAGRAPH_MSG_LEN = 256 };

namespace {
void clear_msg(char* msg) { if (msg) msg[0] = 0; }
int fail(char* msg, int code, const char* what) {
    if (msg) snprintf(msg, LAGRAPH_MSG_LEN, "%s", what);
    return code;
}
template <typename F>
int guarded(char* msg, F&& f) {
    try {
        return f();
    } catch (const falkor::GrbError& e) {
        if (msg) snprintf(msg, LAGRAPH_MSG_LEN, "%s", e.what());
        switch (e.info) {
            case FGPU_OOM: return GrB_OUT_OF_MEMORY;
            case FGPU_OUT_OF_BOUNDS: return GrB_INDEX_OUT_OF_BOUNDS;
            case FGPU_DIM_MISMATCH: return GrB_DIMENSION_MISMATCH;
            case FGPU_NULL_POINTER: return GrB_NULL_POINTER;
            case FGPU_INVALID: return GrB_INVALID_VALUE;
            default: return GrB_PANIC;
        }
    } catch (const std::bad_alloc&) {
        return fail(msg, GrB_OUT_OF_MEMORY, "out of memory");
    } catch (...) {
        return fail(msg, GrB_PANIC, "unexpected exception");
    }
}
// LAGraph_CheckGraph's O(1) rules (lagraph_bindings.rs:254): A present and square, a recognised kind, cached AT of the
// transposed shape, degree vectors of the matching length
int check_graph(LAGraph_Graph G, char* msg) {
    if (!G) return fail(msg, GrB_NULL_POINTER, "graph is NULL");
    if (!G->A) return fail(msg, LAGRAPH_INVALID_GRAPH, "graph adjacency matrix is NULL");
    if (G->kind != 0 && G->kind != 1) return fail(msg, LAGRAPH_INVALID_GRAPH, "graph kind invalid");
    if (G->A->m.nrows() != G->A->m.ncols()) return fail(msg, LAGRAPH_INVALID_GRAPH, "adjacency matrix must be square");
    if (G->AT && (G->AT->m.nrows() != G->A->m.ncols() || G->AT->m.ncols() != G->A->m.nrows()))
        return fail(msg, LAGRAPH_INVALID_GRAPH, "G->AT has the wrong dimensions");
    if (G->out_degree && G->out_degree->n != G->A->m.nrows()) return fail(msg, LAGRAPH_INVALID_GRAPH, "out_degree has the wrong size");
    if (G->in_degree && G->in_degree->n != G->A->m.ncols()) return fail(msg, LAGRAPH_INVALID_GRAPH, "in_degree has the wrong size");
    return GrB_SUCCESS;
}
void check(fgpu_info i, const char* where) { falkor::check(i, where); }
// A serves as its own transpose: an undirected graph, or a directed one whose structure is cached symmetric (check_graph
// has refused every kind but 0 and 1 by the time this is asked)
bool symmetric(LAGraph_Graph G) { return G->kind == 0 || G->is_symmetric_structure == 1; }

// a full result vector of n entries of T over a pinned block of the engine's result pool (`absent` as vector_over_pinned):
// the engine fills `data`; the vector is freed with the scope unless release() handed it to the caller
template <typename T>
struct ResultVector {
    T* data = nullptr;
    GrB_Vector vec = nullptr;
    ResultVector() {}
    ResultVector(const ResultVector&) = delete;
    ResultVector& operator=(const ResultVector&) = delete;
    ~ResultVector() { GrB_Vector_free(&vec); }
    void alloc(GrB_Type type, uint64_t n, int absent, const char* where) {
        falkor::EngineBuf<T> pin(fgshim::context()->raw());
        pin.alloc(n, where);
        vec = fgshim::vector_over_pinned(type, n, pin.p, absent);
        data = pin.release();   // (the vector owns the block from here on)
    }
    GrB_Vector release() {
        GrB_Vector v = vec;
        vec = nullptr;
        return v;
    }
};

#ifndef FG_LAGRAPHX
// degree(i) = entries of A(i,:) as a GrB_INT64 vector that stores only the non-zero degrees (lagraph_bindings.rs:115-116)
GrB_Vector degrees_of(const Matrix& m) {
    fgpu_ctx* raw = fgshim::context()->raw();
    const uint64_t n = m.nrows();
    falkor::EngineBuf<int64_t> out(raw);
    out.alloc(n, "LAGraph_Cached_OutDegree");
    if (n) {
        // the engine writes 32-bit degrees; a pinned block is device-visible, so the kernel fills it directly
        falkor::EngineBuf<uint32_t> d32(raw);
        d32.alloc(n, "LAGraph_Cached_OutDegree");
        check(fgpu_mat_row_degrees(raw, m.snapshot(), d32.p), "LAGraph_Cached_OutDegree");
        for (uint64_t i = 0; i < n; ++i) out[i] = d32[i];
    }
    GrB_Vector v = fgshim::vector_over_pinned(fgshim::type_int64(), n, out.p, 2);
    out.release();   // (the vector owns the block from here on)
    return v;
}
#endif
}  // namespace

extern "C" {

#ifndef FG_LAGRAPHX
// ---- LAGraph core -------------------------------------------------------------------------------------------------------
// matrix.rs:174-183: called after GxB_init; the reference's LAGraph accepts an initialised GraphBLAS, and brings it up
// itself when it is not (LAGraph's own programs call only LAGraph_Init)
int LAGraph_Init(char* msg) {
    clear_msg(msg);
    if (fgshim::context()) return GrB_SUCCESS;
    const GrB_Info r = GrB_init(0 /* GrB_NONBLOCKING */);
    return r == GrB_SUCCESS ? r : fail(msg, r, "GrB_init failed: no HIP device (this library has no CPU path)");
}
int LAGraph_Finalize(char* msg) {      // matrix.rs:215-221: the only shutdown call — GraphBLAS goes down with it
    clear_msg(msg);
    return GrB_finalize();
}
int LAGraph_Version(int* version_number, char* version_date, char* msg) {
    clear_msg(msg);
    if (!version_number || !version_date) return GrB_NULL_POINTER;
    version_number[0] = 1; version_number[1] = 2; version_number[2] = 1;    // lagraph_bindings.rs:16-19
    strcpy(version_date, "Sept 8, 2025");
    return GrB_SUCCESS;
}
// { G->A = *A; *A = NULL; } — cached properties NULL / unknown (lagraph_bindings.rs:175-181)
int LAGraph_New(LAGraph_Graph* G, GrB_Matrix* A, int kind, char* msg) {
    clear_msg(msg);
    if (!G) return fail(msg, GrB_NULL_POINTER, "G is NULL");
    LAGraph_Graph g = new (std::nothrow) LAGraph_Graph_struct();
    if (!g) return fail(msg, GrB_OUT_OF_MEMORY, "out of memory");
    memset(g, 0, sizeof(*g));
    g->kind = kind;
    g->is_symmetric_structure = kind == 0 ? 1 : LAGRAPH_UNKNOWN;
    g->nself_edges = LAGRAPH_UNKNOWN;
    g->emin_state = g->emax_state = LAGRAPH_UNKNOWN;
    if (A) { g->A = *A; *A = nullptr; }
    *G = g;
    return GrB_SUCCESS;
}
int LAGraph_DeleteCached(LAGraph_Graph G, char* msg) {
    clear_msg(msg);
    if (!G) return GrB_SUCCESS;
    GrB_Matrix_free(&G->AT);
    GrB_Vector_free(&G->out_degree);
    GrB_Vector_free(&G->in_degree);
    GrB_Scalar_free(&G->emin);
    GrB_Scalar_free(&G->emax);
    G->is_symmetric_structure = G->kind == 0 ? 1 : LAGRAPH_UNKNOWN;
    G->nself_edges = LAGRAPH_UNKNOWN;
    G->emin_state = G->emax_state = LAGRAPH_UNKNOWN;
    return GrB_SUCCESS;
}
// frees G->A too: a caller that keeps the matrix sets G->A = NULL first (algo_procedures.rs:409-413)
int LAGraph_Delete(LAGraph_Graph* G, char* msg) {
    clear_msg(msg);
    if (!G || !*G) return GrB_SUCCESS;
    LAGraph_DeleteCached(*G, msg);
    GrB_Matrix_free(&(*G)->A);
    delete *G;
    *G = nullptr;
    return GrB_SUCCESS;
}
int LAGraph_CheckGraph(LAGraph_Graph G, char* msg) {
    clear_msg(msg);
    return check_graph(G, msg);
}
// G->AT = A' unless it exists already (left unchanged then, lagraph_bindings.rs:198); the engine keeps one transpose per
// snapshot, so a second graph over the same adjacency reuses it
int LAGraph_Cached_AT(LAGraph_Graph G, char* msg) {
    clear_msg(msg);
    if (const int r = check_graph(G, msg)) return r;
    if (G->AT) return GrB_SUCCESS;
    if (G->kind == 0) return LAGRAPH_CACHE_NOT_NEEDED;
    return guarded(msg, [&]() -> int {
        G->AT = new GB_Matrix_opaque(G->A->m.transpose());
        return GrB_SUCCESS;
    });
}
int LAGraph_Cached_OutDegree(LAGraph_Graph G, char* msg) {
    clear_msg(msg);
    if (const int r = check_graph(G, msg)) return r;
    if (G->out_degree) return GrB_SUCCESS;
    return guarded(msg, [&]() -> int {
        G->out_degree = degrees_of(G->A->m);
        return GrB_SUCCESS;
    });
}
int LAGraph_Cached_InDegree(LAGraph_Graph G, char* msg) {
    clear_msg(msg);
    if (const int r = check_graph(G, msg)) return r;
    if (G->in_degree) return GrB_SUCCESS;
    if (G->kind == 0) return LAGRAPH_CACHE_NOT_NEEDED;
    return guarded(msg, [&]() -> int {
        G->in_degree = degrees_of(G->AT ? G->AT->m : G->A->m.transpose());
        return GrB_SUCCESS;
    });
}
// LAGr_PageRank (lagraph_bindings.rs:549-558): an Advanced method — G->AT and G->out_degree must be cached
// (LAGRAPH_NOT_CACHED otherwise); centrality is a full GrB_FP32 vector; LAGRAPH_CONVERGENCE_FAILURE when itermax
// iterations did not reach tol
int LAGr_PageRank(GrB_Vector* centrality, int* iters, LAGraph_Graph G, float damping, float tol, int itermax, char* msg) {
    clear_msg(msg);
    if (!centrality || !iters) return fail(msg, GrB_NULL_POINTER, "centrality / iters is NULL");
    *centrality = nullptr;
    if (const int r = check_graph(G, msg)) return r;
    GrB_Matrix AT = symmetric(G) ? G->A : G->AT;
    if (!AT) return fail(msg, LAGRAPH_NOT_CACHED, "G->AT is required");
    if (!G->out_degree) return fail(msg, LAGRAPH_NOT_CACHED, "G->out_degree is required");
    return guarded(msg, [&]() -> int {
        ResultVector<float> out;
        out.alloc(fgshim::type_fp32(), G->A->m.nrows(), 0, "LAGr_PageRank");
        int32_t it = 0, converged = 1;
        const fgpu_info r = fgpu_pagerank_status(fgshim::context()->raw(), G->A->m.snapshot(), AT->m.snapshot(), nullptr, damping, tol,
                                                 itermax, out.data, &it, &converged);
        if (r == FGPU_OK && itermax > 0 && !converged) {   // itermax iterations did not reach tol (one run: the engine reports it)
            *iters = it;
            return fail(msg, LAGRAPH_CONVERGENCE_FAILURE, "pagerank failed to converge");
        }
        check(r, "LAGr_PageRank");
        *iters = it;
        *centrality = out.release();
        return GrB_SUCCESS;
    });
}
// LAGr_ConnectedComponents (lagraph_bindings.rs:521-526) as algo.WCC calls it (algo_procedures.rs:816-871): an undirected
// graph, or one whose G->is_symmetric_structure is cached TRUE; component is a full GrB_INT64 vector, component(i) = the
// smallest vertex of i's component (the labelling LAGraph's FastSV converges to).  A directed graph of unknown symmetry is
// refused with GrB_NOT_IMPLEMENTED — LAGraph proper returns LAGRAPH_SYMMETRIC_STRUCTURE_REQUIRED (-1001) there; the code the
// shim has always returned for it is kept, with a message that names the requirement.
int LAGr_ConnectedComponents(GrB_Vector* component, LAGraph_Graph G, char* msg) {
    clear_msg(msg);
    if (!component) return fail(msg, GrB_NULL_POINTER, "component is NULL");
    *component = nullptr;
    if (const int r = check_graph(G, msg)) return r;
    if (!symmetric(G))
        return fail(msg, GrB_NOT_IMPLEMENTED,
                    "LAGr_ConnectedComponents: symmetric structure required (an undirected graph, or G->is_symmetric_structure = true)");
    return guarded(msg, [&]() -> int {
        ResultVector<int64_t> out;
        out.alloc(fgshim::type_int64(), G->A->m.nrows(), 0, "LAGr_ConnectedComponents");
        check(fgpu_wcc(fgshim::context()->raw(), G->A->m.snapshot(), nullptr, nullptr, out.data, nullptr),
              "LAGr_ConnectedComponents");
        *component = out.release();
        return GrB_SUCCESS;
    });
}
// LAGr_Betweenness (lagraph_bindings.rs:539-546) as algo.betweenness calls it (algo_procedures.rs:884-1017): an Advanced
// method — G->AT must be cached for a directed graph whose structure is not known to be symmetric (LAGRAPH_NOT_CACHED
// otherwise; an undirected or symmetric graph uses A).  centrality is a full GrB_FP64 vector of the unnormalised scores over
// the ns sources as given (batched Brandes, fgpu_betweenness); a source >= n is GrB_INVALID_INDEX.
int LAGr_Betweenness(GrB_Vector* centrality, LAGraph_Graph G, const GrB_Index* sources, int32_t ns, char* msg) {
    clear_msg(msg);
    if (!centrality || !sources) return fail(msg, GrB_NULL_POINTER, "centrality / sources is NULL");
    *centrality = nullptr;
    if (const int r = check_graph(G, msg)) return r;
    if (ns < 0) return fail(msg, GrB_INVALID_VALUE, "ns is negative");
    GrB_Matrix AT = symmetric(G) ? G->A : G->AT;
    if (!AT) return fail(msg, LAGRAPH_NOT_CACHED, "G->AT is required");
    const uint64_t n = G->A->m.nrows();
    for (int32_t i = 0; i < ns; ++i)
        if (sources[i] >= n) return fail(msg, GrB_INVALID_INDEX, "invalid source node");
    return guarded(msg, [&]() -> int {
        ResultVector<double> out;
        out.alloc(fgshim::type_fp64(), n, 0, "LAGr_Betweenness");
        check(fgpu_betweenness(fgshim::context()->raw(), G->A->m.snapshot(), AT->m.snapshot(), nullptr, (const uint64_t*)sources,
                               (uint64_t)ns, out.data, nullptr),
              "LAGr_Betweenness");
        *centrality = out.release();
        return GrB_SUCCESS;
    });
}
// LAGraph_Cached_EMin (lagraph_bindings.rs:233-237) as algo.maxFlow calls it (algo_procedures.rs:3159): G->emin = a scalar of
// A's type holding the smallest stored value of A, emin_state = LAGraph_VALUE; left alone when it exists already.  The
// reduction runs on the device (fgpu_mat_min_val).  An A without entries has no smallest entry: the property stays unknown.
// A of a type other than GrB_FP64 / GrB_BOOL is GrB_NOT_IMPLEMENTED (UINT64 matrices carry edge ids, not weights).
int LAGraph_Cached_EMin(LAGraph_Graph G, char* msg) {
    clear_msg(msg);
    if (const int r = check_graph(G, msg)) return r;
    if (G->emin) return GrB_SUCCESS;
    const bool is_bool = G->A->m.type() == Type::Bool;
    if (!G->A->fp64 && !is_bool) return fail(msg, GrB_NOT_IMPLEMENTED, "LAGraph_Cached_EMin: A must be a GrB_FP64 or GrB_BOOL matrix");
    return guarded(msg, [&]() -> int {
        uint64_t bits = 0;
        int found = 0;
        check(fgpu_mat_min_val(fgshim::context()->raw(), G->A->m.snapshot(), &bits, &found), "LAGraph_Cached_EMin");
        if (!found) return GrB_SUCCESS;
        G->emin = new GB_Scalar_opaque{true, is_bool, is_bool ? fgshim::type_bool() : fgshim::type_fp64(), is_bool ? 1 : bits};
        G->emin_state = 0;   // LAGraph_VALUE
        return GrB_SUCCESS;
    });
}
#else
// ---- LAGraphX -----------------------------------------------------------------------------------------------------------
// LAGr_BreadthFirstSearch_Extended (lagraphx_bindings.rs:585-594) as algo.BFS calls it (algo_procedures.rs:1079-1088):
// level(i) = hops from src for every vertex reached within max_level (max_level < 0: no limit), parent(i) = the vertex i was
// discovered from, parent(src) = src; unreached vertices hold no entry.  `dest` >= 0 (stop once a destination is reached) is
// a form the reference never issues: refused rather than guessed.
int LAGr_BreadthFirstSearch_Extended(GrB_Vector* level, GrB_Vector* parent, LAGraph_Graph G, GrB_Index src, int64_t max_level,
                                     int64_t dest, bool many_expected, char* msg) {
    clear_msg(msg);
    (void)many_expected;                                  // a hint about the expected frontier size: the engine's push / pull rule decides
    if (level) *level = nullptr;
    if (parent) *parent = nullptr;
    if (const int r = check_graph(G, msg)) return r;
    if (!level && !parent) return GrB_SUCCESS;            // nothing to compute
    const uint64_t n = G->A->m.nrows();
    if (src >= n) return fail(msg, GrB_INVALID_INDEX, "invalid source node");
    if (dest >= 0) return fail(msg, GrB_NOT_IMPLEMENTED, "LAGr_BreadthFirstSearch_Extended: dest >= 0 is not provided");
    return guarded(msg, [&]() -> int {
        ResultVector<int32_t> lv;   // always computed: the search fills levels whether or not the caller takes them
        ResultVector<int64_t> pa;
        lv.alloc(fgshim::type_int32(), n, 1, "LAGr_BreadthFirstSearch");
        if (parent) pa.alloc(fgshim::type_int64(), n, 1, "LAGr_BreadthFirstSearch");
        // pull needs A'; a directed graph without a cached AT gets the engine's per-snapshot transpose (built once)
        Matrix at = symmetric(G) ? G->A->m : (G->AT ? G->AT->m : G->A->m.transpose());
        check(fgpu_bfs(fgshim::context()->raw(), G->A->m.snapshot(), at.snapshot(), src, max_level < 0 ? -1 : max_level, lv.data,
                       pa.data, nullptr),
              "LAGr_BreadthFirstSearch");
        if (level) *level = lv.release();
        if (parent) *parent = pa.release();
        return GrB_SUCCESS;
    });
}
// LAGraph_cdlp (lagraphx_bindings.rs:218-223) as algo.labelPropagation calls it (algo_procedures.rs:1207-1261): an undirected
// graph, or one whose G->is_symmetric_structure is cached TRUE; CDLP_handle receives a full GrB_INT64 vector, entry i = the
// label vertex i holds after at most itermax synchronous iterations from label(i) = i (fgpu_cdlp; include/fgpu.h states the
// rules — LAGraph numbers its labels from 1, the partition is the same).  LAGraph proper also handles directed graphs;
// algo.labelPropagation never sends one: a directed graph of unknown symmetry is refused with GrB_NOT_IMPLEMENTED and a
// message that names the requirement, as LAGr_ConnectedComponents does.
int LAGraph_cdlp(GrB_Vector* CDLP_handle, LAGraph_Graph G, int itermax, char* msg) {
    clear_msg(msg);
    if (!CDLP_handle) return fail(msg, GrB_NULL_POINTER, "CDLP_handle is NULL");
    *CDLP_handle = nullptr;
    if (const int r = check_graph(G, msg)) return r;
    if (!symmetric(G))
        return fail(msg, GrB_NOT_IMPLEMENTED,
                    "LAGraph_cdlp: symmetric structure required (an undirected graph, or G->is_symmetric_structure = true)");
    if (itermax < 0) return fail(msg, GrB_INVALID_VALUE, "itermax is negative");
    return guarded(msg, [&]() -> int {
        ResultVector<int64_t> out;
        out.alloc(fgshim::type_int64(), G->A->m.nrows(), 0, "LAGraph_cdlp");
        check(fgpu_cdlp(fgshim::context()->raw(), G->A->m.snapshot(), nullptr, itermax, out.data, nullptr), "LAGraph_cdlp");
        *CDLP_handle = out.release();
        return GrB_SUCCESS;
    });
}
// LAGr_HarmonicCentrality (lagraphx_bindings.rs:486-492) as algo.HarmonicCentrality calls it (algo_procedures.rs:2676-2774):
// reads only G->A, of any kind; scores receives a full GrB_FP64 vector and reachable_nodes (nullable) a full GrB_INT64 vector of
// G->A's dimension (fgpu_harmonic; include/fgpu.h states the rules, reachable does not count the vertex itself).  node_weights
// is NULL, or what the procedure sends: a full BOOL vector of true with one entry per vertex; weights of any other form are
// refused with GrB_NOT_IMPLEMENTED and a message.
static bool all_true(GrB_Vector w, uint64_t n) {
    if (!w->type || w->type->code != 0 || w->n != n) return false;
    if (w->data) {
        if (w->absent) return false;
        const uint8_t* b = (const uint8_t*)w->data;
        for (uint64_t i = 0; i < w->nstored; ++i)   // (1 byte for an iso array, n otherwise)
            if (!b[i]) return false;
        return w->nstored == 1 || w->nstored == n;
    }
    if (w->s.size() != n) return false;
    for (auto& kv : w->s)
        if (!kv.second) return false;
    return true;
}
int LAGr_HarmonicCentrality(GrB_Vector* scores, GrB_Vector* reachable_nodes, LAGraph_Graph G, GrB_Vector node_weights, char* msg) {
    clear_msg(msg);
    if (reachable_nodes) *reachable_nodes = nullptr;
    if (!scores) return fail(msg, GrB_NULL_POINTER, "scores is NULL");
    *scores = nullptr;
    if (const int r = check_graph(G, msg)) return r;
    const uint64_t n = G->A->m.nrows();
    if (node_weights && !all_true(node_weights, n))
        return fail(msg, GrB_NOT_IMPLEMENTED,
                    "LAGr_HarmonicCentrality: node_weights must be NULL or a full BOOL vector of true, one entry per vertex");
    return guarded(msg, [&]() -> int {
        ResultVector<double> sc;
        ResultVector<int64_t> re;
        sc.alloc(fgshim::type_fp64(), n, 0, "LAGr_HarmonicCentrality");
        re.alloc(fgshim::type_int64(), n, 0, "LAGr_HarmonicCentrality");
        check(fgpu_harmonic(fgshim::context()->raw(), G->A->m.snapshot(), nullptr, sc.data, re.data, nullptr, nullptr),
              "LAGr_HarmonicCentrality");
        *scores = sc.release();
        if (reachable_nodes) *reachable_nodes = re.release();
        return GrB_SUCCESS;
    });
}
// an n x n GrB_FP64 matrix of the triples (what LAGr_MaxFlow and LAGraph_msf hand out)
static std::unique_ptr<GB_Matrix_opaque> fp64_matrix_from(const falkor::EdgeList& e, uint64_t n) {
    std::unique_ptr<GB_Matrix_opaque> out(new GB_Matrix_opaque(Matrix(*fgshim::context(), Type::UInt64, n, n)));
    out->fp64 = true;
    if (e.n) {
        std::vector<uint64_t> bits(e.n);
        memcpy(bits.data(), e.vals.p, e.n * sizeof(uint64_t));
        out->m.build(std::vector<uint64_t>(e.rows.p, e.rows.p + e.n), std::vector<uint64_t>(e.cols.p, e.cols.p + e.n), &bits);
    }
    return out;
}
// LAGr_MaxFlow (lagraphx_bindings.rs:610-618) as algo.maxFlow calls it (algo_procedures.rs:3161-3170): G holds a GrB_FP64 (or
// GrB_BOOL: capacity 1.0) adjacency of capacities over compact node ids.  An Advanced method — G->AT and G->emin must be cached
// (LAGRAPH_NOT_CACHED otherwise, as LAGr_PageRank treats its properties; the engine builds its own residual network and reads
// neither, and an A without entries has no emin to cache).  *f = the value of a maximum src -> sink flow; *flow_mtx (nullable)
// an n x n GrB_FP64 matrix of the positive flows (fgpu_maxflow; include/fgpu.h states what that flow satisfies).  src or sink
// out of range is GrB_INVALID_INDEX, src == sink GrB_INVALID_VALUE.  res_mtx != NULL asks for the residual matrix as well — a
// form the procedure never sends: refused rather than guessed, as dest >= 0 is in the BFS.
int LAGr_MaxFlow(double* f, GrB_Matrix* flow_mtx, GrB_Matrix* res_mtx, LAGraph_Graph G, GrB_Index src, GrB_Index sink, char* msg) {
    clear_msg(msg);
    if (flow_mtx) *flow_mtx = nullptr;
    if (!f) return fail(msg, GrB_NULL_POINTER, "f is NULL");
    *f = 0;
    if (res_mtx) { *res_mtx = nullptr; return fail(msg, GrB_NOT_IMPLEMENTED, "LAGr_MaxFlow: res_mtx != NULL is not provided"); }
    if (const int r = check_graph(G, msg)) return r;
    if (!G->A->fp64 && G->A->m.type() != Type::Bool)
        return fail(msg, GrB_NOT_IMPLEMENTED, "LAGr_MaxFlow: A must be a GrB_FP64 or GrB_BOOL matrix");
    if (!(symmetric(G) ? G->A : G->AT)) return fail(msg, LAGRAPH_NOT_CACHED, "G->AT is required");
    const uint64_t n = G->A->m.nrows();
    if (!G->emin && G->A->m.nvals()) return fail(msg, LAGRAPH_NOT_CACHED, "G->emin is required");
    if (src >= n || sink >= n) return fail(msg, GrB_INVALID_INDEX, "invalid source / sink node");
    if (src == sink) return fail(msg, GrB_INVALID_VALUE, "source and sink must differ");
    return guarded(msg, [&]() -> int {
        falkor::EdgeList flow(*fgshim::context());
        double value = 0;
        falkor::maxflow(*fgshim::context(), G->A->m.snapshot(), src, sink, &value, flow);
        std::unique_ptr<GB_Matrix_opaque> out;
        if (flow_mtx) out = fp64_matrix_from(flow, n);
        *f = value;
        if (flow_mtx) *flow_mtx = out.release();
        return GrB_SUCCESS;
    });
}
// LAGraph_msf (lagraphx_bindings.rs:261-267) as algo.MSF calls it (algo_procedures.rs:1707-1717): A is a symmetric GrB_FP64
// matrix over compact node ids (a BOOL matrix means every weight is 1.0), sanitize = false.  forest_edges receives an n x n
// GrB_FP64 matrix holding every forest edge once, at (min, max), with its weight; componentId (nullable) a full GrB_INT64
// vector, entry i = the smallest vertex of i's tree (fgpu_msf; include/fgpu.h states the edge order that makes the forest
// unique).  sanitize = true asks LAGraph to symmetrise A first — a form the procedure never sends: refused rather than
// guessed, as dest >= 0 is in the BFS.
int LAGraph_msf(GrB_Matrix* forest_edges, GrB_Vector* componentId, GrB_Matrix A, bool sanitize, char* msg) {
    clear_msg(msg);
    if (componentId) *componentId = nullptr;
    if (!forest_edges) return fail(msg, GrB_NULL_POINTER, "forest_edges is NULL");
    *forest_edges = nullptr;
    if (!A) return fail(msg, GrB_NULL_POINTER, "A is NULL");
    if (sanitize) return fail(msg, GrB_NOT_IMPLEMENTED, "LAGraph_msf: sanitize = true is not provided (pass a symmetric matrix)");
    if (!A->fp64 && A->m.type() != Type::Bool)
        return fail(msg, GrB_NOT_IMPLEMENTED, "LAGraph_msf: A must be a GrB_FP64 or GrB_BOOL matrix");
    if (A->m.nrows() != A->m.ncols()) return fail(msg, GrB_DIMENSION_MISMATCH, "LAGraph_msf: A must be square");
    return guarded(msg, [&]() -> int {
        const uint64_t n = A->m.nrows();
        ResultVector<int64_t> comp;
        if (componentId) comp.alloc(fgshim::type_int64(), n, 0, "LAGraph_msf");
        falkor::EdgeList forest(*fgshim::context());
        falkor::msf(*fgshim::context(), A->m.snapshot(), nullptr, comp.data, forest);
        std::unique_ptr<GB_Matrix_opaque> f = fp64_matrix_from(forest, n);
        *forest_edges = f.release();
        if (componentId) *componentId = comp.release();
        return GrB_SUCCESS;
    });
}
#endif

}  // extern "C"
