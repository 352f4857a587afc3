// host.hpp — C++ host layer above the C ABI (include/fgpu.h): the part of FalkorDB that sits between
// the execution-plan operators and the GraphBLAS boundary, restated over libfgpu.
//
// The reference writes this layer in Rust (graph/src/graph/graphblas/{matrix,versioned_matrix,tensor}.rs,
// graph/src/graph/graph.rs, graph/src/runtime/ops/{cond_traverse,expand_into}.rs,
// graph/src/runtime/functions/algo_procedures.rs).  rustc is not part of the build image, so the
// same types are provided in C++17 with the reference's names, argument meaning and error behaviour;
// every method cites the lines it mirrors (file:line relative to /root/reference/graph/src).
//
// Nothing here computes on the CPU what the reference computes in GraphBLAS: products, merges,
// transposes, probes, builds and BFS all go through fgpu_* calls.  What stays on the host is what the
// reference keeps on the host too: handle ownership, pending-tuple logs, fold bookkeeping, the Tensor
// per-pair state machine, operator control flow.  There is no CPU fallback: constructing a Context
// without a HIP device throws.
#pragma once
#include <stdint.h>

#include <array>
#include <functional>
#include <map>
#include <set>
#include <memory>
#include <mutex>
#include <optional>
#include <stdexcept>
#include <string>
#include <tuple>
#include <unordered_map>
#include <unordered_set>
#include <utility>
#include <vector>

#include "../../include/fgpu.h"
#include "owned.hpp"

namespace falkor {

using u64 = uint64_t;

// GrB_Info other than GrB_SUCCESS / GrB_NO_VALUE.  The Rust wrappers debug_assert on these
// (matrix.rs passim); here they surface as exceptions (check(), owned.hpp) which the C surface (capi.cpp) turns back into codes.
struct GrbError : std::runtime_error {
    fgpu_info info;
    GrbError(fgpu_info i, const std::string& what) : std::runtime_error(what), info(i) {}
};

// matrix::init / matrix::shutdown (graphblas/matrix.rs:116-221): one engine context per process+device.
class Context {
   public:
    explicit Context(int device);
    ~Context();
    Context(const Context&) = delete;
    Context& operator=(const Context&) = delete;
    fgpu_ctx* raw() const { return ctx_; }

   private:
    fgpu_ctx* ctx_ = nullptr;
};

enum class Type { Bool, UInt64 };

// GrB_DESC_* subset the traversal path uses (matrix.rs:313-351)
enum class Descriptor { None, C, RC, RSC };

struct Entry {
    u64 row, col, val;  // val == 1 for BOOL
    bool operator==(const Entry& o) const { return row == o.row && col == o.col && val == o.val; }
};

// Byte stream primitives of the v19 encoders (the reference's Reader / Writer traits; serialize.cpp)
struct ByteWriter {
    std::vector<uint8_t> buf;
    void write_unsigned(u64 v);
    void write_signed(int64_t v);
    void write_buffer(const void* p, size_t n);
};
struct ByteReader {
    const uint8_t* p = nullptr;
    size_t n = 0, pos = 0;
    ByteReader(const uint8_t* data, size_t len) : p(data), n(len) {}
    u64 read_unsigned();
    int64_t read_signed();
    std::vector<uint8_t> read_buffer();
};
// The content of a GxB_Container as the graph stores matrices: sparse or hypersparse, row-major, iso BOOL or UINT64
struct ContainerData {
    u64 nrows = 0, ncols = 0, nvals = 0;
    int format = 2, orientation = 0;
    bool iso = false, jumbled = false, hyper = false, valued = false;
    std::vector<u64> p, h, i, x;   // row pointers (nvec + 1), stored rows (hypersparse), column ids, values
};
ContainerData parse_container(ByteReader& r);                 // Decode<19> for Matrix<T>, CPU part (matrix.rs:428-504)
void write_container(ByteWriter& w, const ContainerData& c);  // Encode<19> for Matrix<T> (matrix.rs:506-546)

// Matrix<T> (graphblas/matrix.rs:360-368): an Arc-shared handle; copies share the underlying matrix,
// `dup()` deep-copies.  The device holds the materialized state as an immutable fgpu_mat snapshot; writes
// queue in a host pending log (GraphBLAS pending tuples / zombies) until wait() folds them in with one
// device merge.
class Matrix {
   public:
    Matrix(Context& ctx, Type t, u64 nrows, u64 ncols);   // Matrix::new   matrix.rs:1151-1156, 1214-1235
    static Matrix adopt(Context& ctx, Type t, SnapshotRef&& snapshot);  // wrap an engine-made snapshot

    Type type() const;
    Context& ctx() const;
    u64 nrows() const;                                   // matrix.rs:706-712
    u64 ncols() const;                                   // matrix.rs:714-720
    u64 nvals() const;                                   // matrix.rs:722-729 (waits: GrB_Matrix_nvals does)
    bool pending() const;                                // matrix.rs:764-779
    bool is_synced() const;                              // matrix.rs:802-804
    void wait() const;                                   // matrix.rs:781-796

    void build(const std::vector<u64>& rows, const std::vector<u64>& cols,
               const std::vector<u64>* vals = nullptr);  // matrix.rs:1281-1303 (bool), 1186-1210 (u64)
    void set_element(u64 i, u64 j, u64 v = 1);           // matrix.rs:1174-1184, 1264-1279
    void remove_element(u64 i, u64 j);                   // matrix.rs:664-676
    std::optional<u64> get(u64 i, u64 j) const;          // matrix.rs:1158-1172, 1248-1262 (NO_VALUE -> nullopt)
    bool contains(u64 i, u64 j) const;                   // matrix.rs:731-737
    // batched form of get/contains: one device probe for the whole list (ExpandInto, label checks)
    void probe(const std::vector<u64>& rows, const std::vector<u64>& cols, std::vector<uint8_t>& present,
               std::vector<u64>* vals) const;
    std::vector<Entry> iter(u64 min_row, u64 max_row) const;  // matrix::Iter  matrix.rs:1471-1605

    Matrix dup() const;                                  // Dup  matrix.rs:370-385
    Matrix transpose() const;                            // matrix.rs:633-662
    void resize(u64 nrows, u64 ncols);                   // matrix.rs:576-598
    Matrix grown(u64 nrows, u64 ncols) const;            // matrix.rs:664-704
    void clear();                                        // matrix.rs:815-822
    void lmxm(const Matrix& b);                          // self = self * b     matrix.rs:930-947
    void rmxm(const Matrix& b);                          // self = b * self     matrix.rs:951-968
    void delta_lmxm(const Matrix& m, const Matrix& dp, const Matrix& dm);  // matrix.rs:1317-1402
    void remove_all(const Matrix& b);                    // self = self \ pattern(b)   matrix.rs:824-833
    void select(const Matrix& mask, const Matrix& a);    // self = a \ pattern(mask)   matrix.rs:835-845
    // self<mask> = a (+) b; a / b default to self.  Supported forms are the ones the Delta layer issues:
    // no mask, or (mask, RC).                              matrix.rs:852-874
    void element_wise_add(const Matrix* mask, const Matrix* a, const Matrix* b, Descriptor d);
    // self = pattern(a) & pattern(b), values of b           matrix.rs:876-896
    void element_wise_multiply(const Matrix* a, const Matrix* b);
    // self<mask> U= pattern(a): no mask, or (mask, C)        matrix.rs:906-924
    void set_pattern(const Matrix* mask, const Matrix& a, Descriptor d);
    u64 intersection_nvals(const Matrix& b) const;       // matrix.rs:743-761

    const fgpu_mat* snapshot() const;  // wait()ed device state, valid until the next mutation
    static Matrix decode(Context& ctx, ByteReader& r);   // Decode<19>  matrix.rs:428-504
    void encode(ByteWriter& w) const;                    // Encode<19>  matrix.rs:506-546

   private:
    struct State;
    std::shared_ptr<State> s_;
    explicit Matrix(std::shared_ptr<State> s) : s_(std::move(s)) {}
    void replace(SnapshotRef&& fresh) const;
};

// matrix::Iter<E> (matrix.rs:1471-1605): a reusable streaming cursor over the entries of rows [min, max] in
// ascending (row, col) order.  `seek` re-aims the same cursor (what CondTraverseOp::expand_row does once per input
// row, cond_traverse.rs:758-974) and keeps the matrix alive like the reference's Arc clone (:1472, 1485-1497).
// Entries come from the device in windows of rows (fgpu_mat_extract), not one FFI call per entry.
class MatrixIter {
   public:
    MatrixIter(const Matrix& m, u64 min_row, u64 max_row);   // Iter::new   matrix.rs:1500-1540
    void seek(u64 min_row, u64 max_row);                      // Iter::seek  matrix.rs:1542-1570
    std::optional<Entry> next();                              // Iterator::next  matrix.rs:1572-1605
   private:
    Matrix m_;
    u64 cur_ = 0, max_ = 0, window_ = 1024;
    bool depleted_ = true;
    std::vector<Entry> buf_;
    size_t pos_ = 0;
    void refill();
};

// fold policy (versioned_matrix.rs:140-200) — pure integer arithmetic, pinned by versioned_matrix.rs:1278-1330
constexpr u64 WRITE_FOLD_K = 20500000;
constexpr u64 READ_FOLD_K = 82000;
constexpr u64 MIN_FOLD_DELTA = 256;
bool fold_balance(u64 delta_nvals, u64 tx_added, u64 base_nvals, u64 k);   // :175-188
bool should_fold(u64 delta_nvals, u64 tx_added, u64 base_nvals);           // :152-158
bool should_fold_read(u64 delta_nvals, u64 tx_added, u64 base_nvals);      // :164-170
bool delta_dominates_base(u64 delta_nvals, u64 base_nvals);                // :195-200

// Delta<T> (versioned_matrix.rs:214-478): one delta layer plus its fold bookkeeping.
class Delta {
   public:
    Delta(Context& ctx, Type t, u64 nrows, u64 ncols);
    explicit Delta(Matrix m);
    Matrix& layer() { return m_; }
    const Matrix& layer() const { return m_; }
    Delta new_version(bool fold) const;                  // :337-349
    bool is_synced() const { return m_.is_synced(); }
    void wait() const { m_.wait(); }
    void resync();                                       // :355-358
    void latch(bool decision) { if (decision) fold_ = true; }             // :360-367
    bool fold_decision(bool (*policy)(u64, u64, u64), u64 base) const;     // :369-377
    bool folding() const { return fold_; }
    bool take_fold();                                    // :383-385
    void clear(u64 nrows, u64 ncols);                    // :387-398
    u64 count() const { return count_; }
    u64 nvals() const { return m_.nvals(); }
    void insert(u64 i, u64 j, u64 v = 1);                // :429-437
    void erase(u64 i, u64 j);                            // :414-422
    std::optional<u64> get(u64 i, u64 j) const { return m_.get(i, j); }
    bool contains(u64 i, u64 j) const { return m_.contains(i, j); }
    void tombstone_masked(const Matrix& mask, const Matrix& base);         // :439-447
    void remove_all(const Matrix& mask);                 // :451-458
    void replace(Matrix m) { m_ = std::move(m); }
    Delta transposed() const;                            // :320-335 (bookkeeping carried verbatim)

   private:
    Matrix m_;
    u64 count_ = 0, tx_nvals_ = 0;
    bool fold_ = false;
};

// the 3-way sorted merge of versioned_matrix::Iter (:1116-1253) over already-extracted layer rows
std::vector<Entry> merge_layers(const std::vector<Entry>& m, const std::vector<Entry>& dp,
                                const std::vector<Entry>& dm);

// VersionedMatrix<bool> — the Delta_Matrix (versioned_matrix.rs:480-1079): committed base m, pending
// additions dp, tombstones dm.  Invariants: dp & m = {}, dm subset of m, dp & dm = {}.
class VersionedMatrix {
   public:
    VersionedMatrix(Context& ctx, u64 nrows, u64 ncols);                   // :494-511
    static VersionedMatrix from_matrix(Matrix m);                          // :877-890
    const Matrix& m() const { return m_; }                                 // :514-528
    const Matrix& dp() const { return dp_.layer(); }
    const Matrix& dm() const { return dm_.layer(); }
    u64 nrows() const { return m_.nrows(); }
    u64 ncols() const { return m_.ncols(); }
    void wait() const;                                                     // :545-556
    void wait_all() const;                                                 // :562-566
    u64 nvals() const;                                                     // :629-632
    Matrix extract() const;                                                // :609-620
    std::optional<bool> get(u64 i, u64 j) const;                           // :819-835
    std::vector<Entry> iter(u64 min_row, u64 max_row) const;               // :647-654 + Iter :1116-1253
    void flush();                                                          // :892-938
    void set(u64 i, u64 j, bool v = true);                                 // :844-857
    void remove(u64 i, u64 j);                                             // :780-791
    void remove_mask(const Matrix& mask);                                  // :799-816
    void set_all(const std::vector<std::pair<u64, u64>>& entries, bool is_new);   // :1006-1035
    // bulk load (no reference counterpart: flush_for_bulk, graph.rs:2129-2140, ends folded and so does this): fold_all folds
    // whatever dp / dm hold into m now; union_base does that and then m = pattern(m) U pattern(arg), one device merge.  The
    // base is REPLACED, never mutated: dup()ed versions and extracted matrices keep the snapshot they share
    void fold_all();
    void union_base(const Matrix& pattern);
    // bulk DETACH DELETE (the label rows of Graph::delete_nodes, graph.rs:1753-1768, and the adjacency's share of
    // delete_implicit_edges, as ONE device pass): fold_all, then the base is replaced by fgpu_nodes_detach's result — without
    // the entries whose row (sides bit 0) or column (bit 1) is one of `nodes` (any order, duplicates allowed).  Returns the
    // number of entries removed; a node outside the dimension it indexes throws before anything changed.  No tombstone is left
    // to fold later, and dup()ed versions keep the base they share.
    u64 detach_base(const std::vector<u64>& nodes, int sides);
    VersionedMatrix dup() const;                                           // :1038-1051
    void fold_oversized();                                                 // :953-965
    void fold_latched();                                                   // :940-951
    void resize(u64 nrows, u64 ncols);                                     // :967-1004
    VersionedMatrix transpose() const;                                     // :1070-1079
    bool needs_flush() const { return needs_flush_; }
    const Delta& dp_delta() const { return dp_; }
    const Delta& dm_delta() const { return dm_; }

   private:
    VersionedMatrix(Matrix m, Delta dp, Delta dm) : m_(std::move(m)), dp_(std::move(dp)), dm_(std::move(dm)) {}
    Matrix m_;
    mutable Delta dp_, dm_;
    bool needs_flush_ = false;
};

constexpr u64 MULTI_EDGE = ~0ull;                        // tensor.rs:207
// What a bulk insert did (Tensor::bulk_insert / Graph::bulk_insert_edges): the batch went through the device build
// (device_edges = n) or, because one of its pairs already held an edge, through set_all_from_slices (fallback_edges = n);
// the other four are fgpu_edges_build's stats [0], [1], [4], [6] of the batch.
struct BulkStats {
    u64 device_edges = 0, fallback_edges = 0, distinct_pairs = 0, multi_pairs = 0, unsorted_runs = 0, host_sorted_runs = 0;
    // host clock, ns (a measurement hook, tools/bench_paths.py load): [0] the fgpu_edges_build call, [1] folding the layers
    // and adopting / merging the built pieces (or the whole fallback), [2] filling me, [3] the adjacency union
    u64 phase_ns[4] = {0, 0, 0, 0};
};
// What a bulk append did (Tensor::append_bulk / Graph::append_edges_bulk): edges = n, the batch's distinct and multi-edge pairs
// (fgpu_edges_build's stats [0], [1]), the pairs that collided with a stored one and how (fgpu_edges_union's stats [1..3]), the me
// rows written, and the runs the build had the host sort (its stats [6])
struct AppendStats {
    u64 edges = 0, distinct_pairs = 0, multi_pairs = 0, colliding = 0, promoted = 0, extended = 0, me_rows = 0, host_sorted_runs = 0;
    // host clock, ns (a measurement hook, tools/bench_paths.py append): [0] the fgpu_edges_build call, [1] the folds, the row
    // gather and the fgpu_edges_union call, [2] rewriting me, [3] the adjacency union
    u64 phase_ns[4] = {0, 0, 0, 0};
};
// What Tensor::detach_nodes did beside the list it returns (accumulated: a Graph adds every type's into one)
struct DetachCounts {
    u64 removed = 0;             // edges taken out of the tensor, the skipped ones included
    u64 multi_pairs = 0;         // multi-edge pairs among them (their me rows are erased)
    std::vector<u64> skipped;    // the removed ids that skip_ids kept out of the list
    u64 phase_ns[2] = {0, 0};    // host clock: [0] fold + fgpu_nodes_detach + adoption, [1] expanding and ordering the list
};
// What Graph::delete_nodes_bulk did, in the shape of BulkStats
struct DetachStats {
    u64 nodes = 0, edges_removed = 0, edges_listed = 0, label_entries = 0, adjacency_entries = 0, multi_pairs = 0;
    std::vector<u64> per_type;   // edges removed per relationship type (the skipped ones included)
    // host clock, ns (a measurement hook, tools/bench_paths.py detach): [0] the tensors' folds and fgpu_nodes_detach calls,
    // [1] expanding and ordering their lists, [2] the label matrix, [3] the adjacency
    u64 phase_ns[4] = {0, 0, 0, 0};
};
// What Tensor::remove_bulk did beside the emptied pairs it returns
struct RemoveCounts {
    std::vector<uint8_t> hit;    // per triple of the batch: it named a stored edge (every duplicate of one too)
    u64 hits = 0;                // the ones in `hit`
    u64 removed = 0;             // edges that left the tensor: hits, a repeated triple counted once
    u64 emptied_multi = 0;       // multi-edge pairs among the emptied ones
    u64 demoted = 0;             // multi-edge pairs left with one edge, stored inline again
    u64 phase_ns[3] = {0, 0, 0}; // host clock: [0] gathering the me rows, [1] fold + fgpu_edges_remove + adoption, [2] rewriting me
};
// What Graph::delete_edges_bulk did, in the shape of DetachStats
struct EdgeDeleteStats {
    u64 edges_named = 0, edges_removed = 0, pairs_emptied = 0, pairs_demoted = 0, adjacency_entries = 0;
    std::vector<u64> per_type;   // edges removed per relationship type
    // host clock, ns (a measurement hook, tools/bench_paths.py edel): [0] gathering the me rows, [1] the tensors' folds and
    // fgpu_edges_remove calls, [2] rewriting me, [3] the adjacency
    u64 phase_ns[4] = {0, 0, 0, 0};
};
constexpr u64 GrB_INDEX_MAX = (1ull << 60) - 1;          // tensor.rs:136
u64 compound_key(u64 src, u64 dst);                      // tensor.rs:154-163 (throws when an id needs > 32 bits)
u64 bulk_clock_ns();                                     // the host clock of BulkStats::phase_ns

// Tensor (tensor.rs:184-205): per-relationship-type edge storage with inline edge ids.  Forward layers
// (m, dp UINT64; dm BOOL) and the BOOL transpose `mt` live on the device.  `me` — all ids of the pairs
// that hold more than one edge, keyed by compound_key(src, dst) — is a GrB_INDEX_MAX-square hypersparse
// matrix in the reference; its keys do not fit the 32-bit device id space and it is only ever read one
// row at a time, so it is kept as an ordered host map with the same observable behaviour (ascending ids).
class Tensor {
   public:
    Tensor(Context& ctx, u64 nrows, u64 ncols);                            // tensor.rs:241-251
    u64 nrows() const { return m_.nrows(); }
    u64 ncols() const { return m_.ncols(); }
    void wait_fwd() const;                                                 // :265-282
    std::optional<u64> eff_get(u64 src, u64 dst) const;                    // :286-299
    std::vector<u64> get(u64 src, u64 dst) const;                          // :307-319 (ascending edge ids)
    // batched eff_get / get: three device probes for the whole list of pairs
    void get_batch(const std::vector<u64>& srcs, const std::vector<u64>& dsts,
                   std::vector<std::vector<u64>>& ids) const;
    void set_all_from_slices(const std::vector<u64>& srcs, const std::vector<u64>& dsts,
                             const std::vector<u64>& ids);                 // :333-455
    // One relationship type's bulk batch (the shape of Graph::create_relationships_bulk + flush_for_bulk, graph.rs:2062-2140):
    // fgpu_edges_build sorts and groups the batch, the layers are folded, and the built forward matrix / transposed pattern /
    // multi-edge runs become the tensor's base — adopted when the tensor is empty, merged in when the batch touches no pair
    // that holds an edge.  A batch that does goes through set_all_from_slices whole.  Ends folded (dp = dm = 0) on the device
    // path.  `built` (nullable) receives the batch's forward matrix on the device path, for the adjacency union.  An invalid
    // batch (fgpu_edges_build's rules) throws before anything changed.
    BulkStats bulk_insert(const std::vector<u64>& srcs, const std::vector<u64>& dsts, const std::vector<u64>& ids,
                          std::optional<Matrix>* built = nullptr);
    // (the same over the caller's arrays: a load of 2^26 tuples is 1.6 GB that need not be copied into vectors first)
    BulkStats bulk_insert(const u64* srcs, const u64* dsts, const u64* ids, u64 n, std::optional<Matrix>* built = nullptr);
    // A bulk batch onto a tensor that may hold edges on the batch's pairs (set_all_from_slices' result, tensor.rs:333-447, for the
    // whole batch on the device; it never falls back): fgpu_edges_build first, so an invalid batch throws before any layer
    // moved; the layers are folded as bulk_insert folds them; an empty tensor adopts the built pieces; otherwise, when the tensor
    // holds multi-edge pairs, ONE probe of m finds the batch's pairs whose value is MULTI_EDGE and their me rows go along, sorted
    // unique by key; ONE fgpu_edges_union gives the new bases, which are adopted (replaced, never mutated: a dup()ed version or
    // a matrix built earlier keeps its snapshot), and me takes the batch's rows of new multi-edge pairs and the merged rows of the
    // colliding ones.  Ends folded.  An id already stored on its pair (the union's FGPU_INVALID) throws with the effective state
    // unchanged.  `built` (nullable) receives the batch's forward matrix, for the adjacency union.
    AppendStats append_bulk(const u64* srcs, const u64* dsts, const u64* ids, u64 n, std::optional<Matrix>* built = nullptr);
    // This type's share of Graph::delete_implicit_edges (graph.rs:2386-2494) for the node set `nodes` (any order, duplicates
    // allowed), as one device pass: m / dp / dm and mt are folded, ONE fgpu_nodes_detach takes every entry incident to the nodes
    // out of m and mt and its results are adopted as the bases — the tensor ends folded (dp = dm = 0), no tombstone is left —
    // and the me rows of the removed multi-edge pairs are erased.  Returns (edge id, src, dst) in the reference's order
    // (:2405-2427): per node ascending, first its out edges by ascending dst, then its in edges from sources that are not
    // deleted themselves by ascending src; the ids of a multi-edge pair ascending.  A self-loop and an edge between two
    // deleted nodes are listed once, from the source.
    // Ids in `skip_ids` (the reference's explicit_rels, which delete_relationships handles) are LEFT OUT of the returned list,
    // but their entries are removed like the others: the reference leaves them to the explicit delete that follows, here that
    // later delete_edge finds the pair absent and does nothing — the state after both steps is the reference's.
    // A node at or past the dimension throws before anything changed.  Versions dup()ed earlier keep the bases they share.
    std::vector<std::array<u64, 3>> detach_nodes(const std::vector<u64>& nodes, const std::unordered_set<u64>& skip_ids = {},
                                                 DetachCounts* counts = nullptr);
    std::vector<std::pair<u64, u64>> remove_all(const std::vector<std::array<u64, 3>>& rels);  // :461-657
    // remove_all's slow path (tensor.rs:497-629) for a whole batch of (src, dst, id) triples, as one device pass: m / dp / dm and
    // mt are folded as detach_nodes folds them; when the tensor holds multi-edge pairs, ONE probe of m finds the batch's pairs
    // whose value is MULTI_EDGE and their me rows go along, sorted unique by key (no walk of the whole map); ONE
    // fgpu_edges_remove decides every triple; when anything hit its results are adopted as the bases — the tensor ends folded,
    // no tombstone is left — and the supplied me rows lose the taken ids, a row left with fewer than 2 is erased (its pair was
    // demoted or emptied on the device).  Returns the pairs left without an edge, ascending in (src, dst).  A removal applies
    // only where the id is there: an unknown id, an id of another pair and an absent pair change nothing, a repeated triple
    // counts once — unlike remove_all's no-multi fast path, which drops the pair whatever the id.  A coordinate at or past its
    // dimension throws before anything changed.  Versions dup()ed earlier keep the bases they share.
    std::vector<std::pair<u64, u64>> remove_bulk(const u64* srcs, const u64* dsts, const u64* ids, u64 n, RemoveCounts* counts = nullptr);
    // effective presence of every pair (eff_get(src, dst).has_value()): three device probes for the whole list
    void contains_batch(const std::vector<u64>& srcs, const std::vector<u64>& dsts, std::vector<uint8_t>& present) const;
    bool has_multi_edge() const { return !me_.empty(); }
    // me as an fgpu_multi for fgpu_expand_edges (nullptr while no pair holds several edges): built from the map on the first
    // batch that needs it — the map is key-ordered, which is the table's order — and dropped by every method that may write me.
    // Copies of the tensor (dup) share the table until one of them writes and drops its own reference
    const fgpu_multi* multi_table() const;
    void resize(u64 nrows, u64 ncols);                                     // :659-726 (me's keys are not touched)
    void flush();                                                          // :741-797
    void fold_oversized();                                                 // :815-833
    Matrix extract() const;                                                // :838-850
    Tensor dup() const;                                                    // :871-889
    const Matrix& fwd_m() const { return m_; }                             // :891-907
    const Matrix& fwd_dp() const { return dp_.layer(); }
    const Matrix& fwd_dm() const { return dm_.layer(); }
    const VersionedMatrix& matrix_t() const { return mt_; }                // :936-943
    std::vector<Entry> structural_iter(u64 min_row, u64 max_row) const;    // :909-921
    std::vector<Entry> iter_edges() const;                                 // :973-989 (src, dst, edge id)
    u64 edge_count() const;                                                // :955-967
    // Encode<19> / Decode<19> for Tensor (tensor.rs:1053-1209): three container payloads (effective forward matrix —
    // single-edge pairs store the id, multi-edge pairs `count | 1 << 63` — then empty dp and dm), the edge count, and
    // the tensor section: two groups (base, delta-plus) of (src, dst, id-list blob).  The blob is what C FalkorDB
    // writes with GxB_Vector_serialize — GraphBLAS' own serialisation of a BOOL vector whose INDICES are the edge ids;
    // it can only be produced / parsed by GraphBLAS itself, so it goes through `BlobCodec` (see serialize.cpp).  The
    // backward matrix is rebuilt after decode (rebuild_backward, as the reference's caller does).
    struct BlobCodec {
        std::function<std::vector<uint8_t>(const std::vector<u64>& ids)> encode;
        std::function<std::vector<u64>(const std::vector<uint8_t>& blob)> decode;
    };
    static const BlobCodec& plain_blob_codec();
    void encode(ByteWriter& w, const BlobCodec& codec = plain_blob_codec()) const;
    static Tensor decode(Context& ctx, ByteReader& r, const BlobCodec& codec = plain_blob_codec());
    void rebuild_backward();
    u64 multi_pairs() const { return me_.size(); }
    u64 me_nvals() const { u64 n = 0; for (auto& kv : me_) n += kv.second.size(); return n; }   // `me.nvals()` of the tests
    void wait() const { wait_fwd(); mt_.wait(); }                           // Tensor::wait: every layer materialised

   private:
    using MeRow = std::map<u64, std::vector<u64>>::iterator;
    struct BuiltBatch;   // what fgpu_edges_build made of a batch (tensor.cpp)
    // The steps the bulk mutations share.  fold_for_bulk: a bulk mutation starts folded (flush_for_bulk) — whatever dp / dm and
    // mt's deltas hold goes into the bases, which are all the device pass reads.  gather_me_rows: the me rows of the batch's
    // pairs that hold MULTI_EDGE, sorted unique by key, as fgpu_edges_union / fgpu_edges_remove take them (off starts as {0});
    // ONE probe of the folded base, then one find per such pair; `rows` (nullable) receives the map positions.  build_batch:
    // fgpu_edges_build of a batch, its pieces adopted.  adopt_bases: the results of a device pass become m and mt (replaced,
    // never mutated: a dup()ed version keeps its snapshot).
    void fold_for_bulk();
    void gather_me_rows(const u64* srcs, const u64* dsts, u64 n, std::vector<u64>& key, std::vector<u64>& off, std::vector<u64>& run,
                        std::vector<MeRow>* rows);
    BuiltBatch build_batch(const u64* srcs, const u64* dsts, const u64* ids, u64 n, const char* who) const;
    void adopt_bases(const Matrix& m, const Matrix& mt);
    void adopt_bases(SnapshotRef&& mo, SnapshotRef&& mto, bool changed);   // (engine-made outputs of a device pass)

    Matrix m_;
    mutable Delta dp_, dm_;
    VersionedMatrix mt_;
    std::map<u64, std::vector<u64>> me_;   // compound key -> ascending edge ids (pairs with >= 2 edges)
    mutable std::shared_ptr<MultiRef> multi_;   // me_ on the device (multi_table), or empty
    bool needs_flush_ = false;
};

using LabelId = u64;

// One vector index of a graph (index/mod.rs:1768-1823 keeps an HNSW graph per (label or type, attribute); here it is an
// fgpu_vecidx, searched exhaustively on the device).  Entities are node ids or relationship ids; an edge index remembers the
// endpoints of every relationship it holds, which is what db.idx.vector.queryRelationships yields beside the id.
struct VectorIndex {
    fgpu_ctx* ctx = nullptr;
    fgpu_vecidx* idx = nullptr;
    uint32_t dim = 0;
    int metric = FGPU_VEC_EUCLIDEAN;
    std::unordered_map<u64, std::pair<u64, u64>> ends;   // edge indexes: relationship id -> (src, dst)
    VectorIndex() = default;
    VectorIndex(const VectorIndex&) = delete;
    VectorIndex& operator=(const VectorIndex&) = delete;
    ~VectorIndex() { if (idx) fgpu_vecidx_free(idx); }
};
// rows of a vector query; a batch of nq queries has offsets[nq + 1] over the other columns, rows in query order
struct VectorHits {
    std::vector<u64> ids, srcs, dsts, offsets;
    std::vector<double> dist;
};
// the metric of a similarity name ("euclidean", "cosine", "ip"; NULL = euclidean); anything else throws the reference's text
// (index/mod.rs:1259-1270)
int vector_metric(const char* similarity);
// vec.euclideanDistance / vec.cosineDistance (runtime/vec_distance.rs) in FP64, D of fgpu_vecidx_knn; na != nb throws
// "Vector dimension mismatch, expected {na} but got {nb}" (spatial.rs:161-166)
double vec_distance(int metric, const float* a, u64 na, const float* b, u64 nb);

// The traversal-facing slice of graph.rs.
class Graph {
   public:
    Graph(Context& ctx, u64 node_cap, u64 label_cap = 64);
    Context& ctx() const { return *ctx_; }
    u64 node_cap() const { return n_; }
    VersionedMatrix& adjacency_matrix() { return adj_; }                   // graph.rs:2251
    const VersionedMatrix& adjacency_matrix() const { return adj_; }
    VersionedMatrix& node_labels_matrix() { return labels_; }              // graph.rs:1057-1066
    const VersionedMatrix& node_labels_matrix() const { return labels_; }
    std::vector<Tensor>& relationship_tensors() { return tensors_; }       // graph.rs:2256
    const std::vector<Tensor>& relationship_tensors() const { return tensors_; }
    LabelId add_label(const std::string& name);
    u64 add_type(const std::string& name);
    std::optional<LabelId> label_id(const std::string& name) const;
    std::optional<u64> type_id(const std::string& name) const;
    void label_node(u64 node, LabelId l) { labels_.set(node, l, true); }
    void delete_node(u64 node) {
        deleted_[node] = true;
        if (!vec_indexes_.empty()) drop_entity_vectors(false, std::nullopt, node);   // test_vecsim.py test09
    }
    bool is_node_deleted(u64 node) const { return !deleted_.empty() && deleted_.count(node) != 0; }
    u64 deleted_nodes_count() const { return deleted_.size(); }   // graph.rs deleted_nodes_count
    // graph.rs node_count: the ids below node_cap() that are not deleted (delete_node takes any id: one at or past the
    // capacity is in deleted_nodes_count() and is not a node)
    u64 live_nodes() const {
        u64 live = n_;
        for (auto& d : deleted_) live -= d.first < n_ ? 1 : 0;
        return live;
    }
    // create one edge of `type` (adjacency + tensor), the write-side minimum the tests need
    void create_edge(u64 type, u64 src, u64 dst, u64 edge_id);             // graph.rs:1493-1560 (effect only)
    void delete_edge(u64 type, u64 src, u64 dst, u64 edge_id);             // graph.rs:1623-1700 (effect only)
    void create_edges(u64 type, const std::vector<u64>& srcs, const std::vector<u64>& dsts,
                      const std::vector<u64>& ids);                        // bulk form of create_edge
    // the bulk LOAD of one type: Tensor::bulk_insert, then the adjacency's base U= the batch's pattern (on the fallback the
    // adjacency set_all of create_edges).  Matrices built or versions dup()ed earlier are untouched.
    BulkStats bulk_insert_edges(u64 type, const std::vector<u64>& srcs, const std::vector<u64>& dsts,
                                const std::vector<u64>& ids);
    BulkStats bulk_insert_edges(u64 type, const u64* srcs, const u64* dsts, const u64* ids, u64 n);
    // CREATE of one type's batch onto a graph that holds edges: Tensor::append_bulk — every edge through the device, whatever
    // pairs the batch touches — then the adjacency's base U= the batch's pattern.  An invalid batch (a node at or past the
    // capacity, the marker as an id, a triple twice, an id already stored on its pair) throws with the graph as it was.
    AppendStats append_edges_bulk(u64 type, const u64* srcs, const u64* dsts, const u64* ids, u64 n);
    // bulk DETACH DELETE (Pending::commit's Graph::delete_nodes + delete_implicit_edges, graph.rs:1698-1772, 2386-2494, as one
    // call): every node gets delete_node's effects; every tensor detach_nodes — the returned list is their lists in ascending
    // type id — and every removed edge leaves the vector indexes as delete_edge makes it; the node x label matrix loses the
    // nodes' rows (sides = 1) and the adjacency every entry incident to them (sides = 3).  That removes the (deleted, deleted)
    // pairs too, which the reference leaves in the adjacency as unreachable (:2381-2383): it is what the edge-by-edge path
    // produces and what the algo.* builders should see.  An empty `nodes` does nothing; a node at or past node_cap() throws
    // before anything changed.
    std::vector<std::array<u64, 3>> delete_nodes_bulk(const std::vector<u64>& nodes, const std::vector<u64>& skip_ids = {},
                                                      DetachStats* stats = nullptr);
    // bulk DELETE r (the shape of Graph::delete_relationships, graph.rs:2303-2372): the n edges (types, srcs, dsts, ids)[k] are
    // grouped by type and each group goes through Tensor::remove_bulk, in ascending type id; every named id leaves the vector
    // indexes of its type as delete_edge makes it; the pairs some tensor emptied and no tensor still holds leave the adjacency
    // through one remove_mask.  Returns the removed (edge id, src, dst): types ascending, input order within a type, only the
    // triples that named a stored edge, a repeated one once.  An unknown type or a node at or past node_cap() throws before
    // anything changed.
    std::vector<std::array<u64, 3>> delete_edges_bulk(const u64* types, const u64* srcs, const u64* dsts, const u64* ids, u64 n,
                                                      EdgeDeleteStats* stats = nullptr);
    void new_version();              // graph.rs:851-890: every matrix dup()s (fold decisions latch here)
    void fold_oversized_deltas();    // graph.rs:2155-2172, called at MVCC commit (mvcc_graph.rs:161-180)

    bool node_has_label_id(u64 node, LabelId l) const;                     // graph.rs:1057-1066
    // all labels known? (unknown label => the pattern can match nothing)  graph.rs:2554-2559
    std::optional<std::vector<LabelId>> resolve_label_ids(const std::vector<std::string>& labels) const;
    // N-bit bitmap of the nodes carrying every label of `ids` (all ones when ids is empty)
    std::vector<u64> label_bitmap(const std::vector<LabelId>& ids) const;
    Matrix build_relationship_matrix_unrestricted(const std::vector<u64>& type_ids) const;  // graph.rs:2520-2549
    Matrix build_adjacency_matrix(const std::vector<std::string>& types) const;             // graph.rs:3870-3894
    Matrix build_symmetric_adjacency_matrix(const std::vector<std::string>& types) const;   // graph.rs:3898-3907 (A + A')
    std::vector<u64> get_src_dest_relationships(u64 src, u64 dst, const std::vector<u64>& type_ids) const;  // :1797-1837

    // Vector indexes (vector_index.cpp), keyed by (label id, attribute) for nodes and (type id, attribute) for relationships.
    // The attribute store is out of scope: the caller feeds the vectors in, as the reference's indexer is fed by property
    // writes.  create on an indexed (owner, attribute) throws; drop returns whether there was one.
    void vector_index_create(bool is_edge, u64 owner, const std::string& attr, u64 dim, const char* similarity);
    bool vector_index_drop(bool is_edge, u64 owner, const std::string& attr);
    // upsert / remove one entity's vector; no index on (owner, attr) throws, n != dim throws the dimension mismatch text
    void vector_set_node(LabelId label, const std::string& attr, u64 node, const float* vec, u64 n);
    void vector_set_edge(u64 type, const std::string& attr, u64 src, u64 dst, u64 edge_id, const float* vec, u64 n);
    bool vector_unset_node(LabelId label, const std::string& attr, u64 node);
    bool vector_unset_edge(u64 type, const std::string& attr, u64 edge_id);
    // db.idx.vector.queryNodes / queryRelationships for nq queries of qn components each, ONE fgpu_vecidx_knn call
    // (graph.rs:3408-3457 answers one; NodeByVectorScanOp::next calls it per parent row).  k <= 0 throws "Invalid arguments
    // for procedure '...'", qn != dim "Vector dimension mismatch, expected {dim} but got {qn}"; an unknown label / type or no
    // index on (it, attr) gives no rows (indexer.rs:525-536).  Rows per query in ascending (distance, id).
    VectorHits vector_query(bool is_edge, const std::string& owner_name, const std::string& attr, int64_t k, const float* queries,
                            u64 qn, u64 nq) const;
    const VectorIndex* vector_index(bool is_edge, u64 owner, const std::string& attr) const;

   private:
    // delete_node / delete_edge: the entity leaves every index that holds it (of one owner when given)
    void drop_entity_vectors(bool is_edge, std::optional<u64> owner, u64 entity);
    std::map<std::tuple<bool, u64, std::string>, std::unique_ptr<VectorIndex>> vec_indexes_;
    Context* ctx_;
    u64 n_;
    VersionedMatrix adj_, labels_;
    std::vector<Tensor> tensors_;
    std::unordered_map<std::string, LabelId> label_ids_;
    std::unordered_map<std::string, u64> type_ids_;
    std::unordered_map<u64, bool> deleted_;

   public:
    // algo.BFS keeps its device plan (workspace, pinned control block, acceleration indexes) between calls for as
    // long as the adjacency it was built on is the same immutable snapshot — creating one costs more than the search
    struct BfsPlanCache {
        Matrix adj, adj_t;                 // keep the snapshots (and their cached indexes) alive
        std::string key;                   // relationship types the adjacency was built for
        // level[] / parent[] in pinned blocks of the context's pool: fgpu_bfs_fetch DMAs into them — the procedure reads the
        // vectors element by element afterwards (algo_procedures.rs:1096-1160), it never needs a copy.  Members are destroyed
        // in reverse order of declaration: the pinned blocks are declared BEFORE the plan so that the plan is freed first
        EngineBuf<int32_t> level_pin;
        EngineBuf<int64_t> parent_pin;
        u64 pin_rows = 0;
        PlanRef plan;
        // one search at a time runs on the cached plan AND reads its pinned result blocks: the reference's worker pool calls
        // algo.BFS on a shared const Graph from several threads (threadpool.rs:89-128); a second caller that finds the plan
        // busy takes the one-shot path with vectors of its own instead of waiting
        std::mutex mu;
        BfsPlanCache(Matrix a, Matrix at, fgpu_ctx* raw) : adj(std::move(a)), adj_t(std::move(at)), level_pin(raw), parent_pin(raw) {}
    };
    mutable std::shared_ptr<BfsPlanCache> bfs_cache_;
    mutable std::mutex bfs_cache_mu_;      // orders readers and replacers of bfs_cache_ (the entry itself has its own lock)
    // the same for a partitioned search over a gang of contexts: balanced splits, one column slab (+ transpose) and one
    // slab plan per device — building them costs far more than a search, so they live as long as the
    // adjacency snapshot, the relationship filter and the gang stay the same
    struct BfsGangCache {
        Matrix adj;                         // keeps the snapshot the slabs were cut from alive (and comparable)
        std::string key;
        std::vector<fgpu_ctx*> gang;
        std::vector<u64> splits;
        std::vector<SnapshotRef> slabs, slabs_t;
        std::vector<PlanRef> plans;
        std::mutex mu;
        explicit BfsGangCache(Matrix a) : adj(std::move(a)) {}
        // frees the device objects (idempotent).  Called by the destructor and by Context::~Context of ANY context of the
        // gang, BEFORE that context is finalised: the slabs and plans of a gang live in several contexts, and none of them
        // may be touched once one of those is gone
        void release() {
            std::lock_guard<std::mutex> g(mu);
            plans.clear(); slabs_t.clear(); slabs.clear(); gang.clear();   // in this order: plans, transposed slabs, slabs
        }
        ~BfsGangCache() { release(); }
    };
    static void register_gang_cache(const std::shared_ptr<BfsGangCache>& c);   // (matrix.cpp, next to Context::~Context)
    mutable std::shared_ptr<BfsGangCache> bfs_gang_cache_;
    // the eight stats of the last fgpu_pair_weights call an algorithm made on this graph (algo_msf, algo_sp_paths and the
    // pruning table of algo_sp_paths_rows build their weight matrix with it); all 0 before the first
    mutable std::array<u64, 8> pair_stats_{};
    mutable std::mutex pair_stats_mu_;

   public:
    std::array<u64, 8> pair_stats() const {
        std::lock_guard<std::mutex> lock(pair_stats_mu_);
        return pair_stats_;
    }
    void set_pair_stats(const u64* stats) const {
        std::lock_guard<std::mutex> lock(pair_stats_mu_);
        std::copy(stats, stats + 8, pair_stats_.begin());
    }
};

// A bound value of one batch row, reduced to what the traversal operators inspect.
struct Value {
    enum Kind { Unbound, Null, Node, Other } kind = Unbound;
    u64 id = 0;
    static Value node(u64 id) { return Value{Node, id}; }
    static Value null() { return Value{Null, 0}; }
};

struct Hop {                               // one (types, dst labels) step; hop 0 is the operator's own pattern
    std::vector<std::string> types;
    std::vector<std::string> dst_labels;
};

// Result columns of expand_batch, in emission order: the emitter gathers the parent columns by `active_row`
// and appends `dest` as a NodeIds column (+ `edge` as RelIds when a representative edge was bound),
// cond_traverse.rs:700-735.
struct ExpandedRows {
    std::vector<u64> active_row;   // index into the input batch
    std::vector<u64> dest;
    std::vector<u64> edge;         // empty unless bind_relationship
    // The batched path hands over the two columns as the DEVICE built them (fgpu_expand_pairs32): pinned blocks of the context's
    // pool filled by DMA — 16-bit row indices (a child batch holds at most 1024 rows, batch.rs:81; 32-bit ones when a host layer
    // coalesces more than 65536 rows into one call) and the destinations as the 32-bit node ids the device works in (every node
    // id of a traversed graph fits 32 bits: tensor.rs:154-163 demands it of the multi-edge keys); row_at / dest_at widen on
    // access, which is where the reference's NodeId(u64) is needed.  They are owned until clear(), and make the struct move-only;
    // materialize() copies them into the vectors above for the rare consumers that edit the columns in place.
    EngineBuf<uint16_t> row_pin;
    EngineBuf<uint32_t> row_pin32, dest_pin;
    size_t n_pin = 0;
    bool pinned() const { return dest_pin.p != nullptr; }
    size_t size() const { return pinned() ? n_pin : dest.size(); }
    u64 row_at(size_t i) const { return pinned() ? (row_pin.p ? (u64)row_pin.p[i] : (u64)row_pin32.p[i]) : active_row[i]; }
    u64 dest_at(size_t i) const { return pinned() ? (u64)dest_pin.p[i] : dest[i]; }
    void release_pinned() { row_pin.reset(); row_pin32.reset(); dest_pin.reset(); n_pin = 0; }
    void materialize();
    void clear() { active_row.clear(); dest.clear(); edge.clear(); release_pinned(); }
};

// CondTraverseOp (runtime/ops/cond_traverse.rs).  Only the matrix path and its eligibility rule are
// mirrored; the attribute filters of the per-row path need the attribute store (out of scope).
struct CondTraverseOp {
    std::vector<std::string> src_labels;
    std::vector<Hop> hops;               // hops[0] + chain (fuse_anonymous_traverse.rs:83-188)
    bool optional = false;
    bool bind_relationship = false;      // representative edge wanted (cond_traverse.rs:663-695)
    bool emit_relationship = false, bidirectional = false, has_sibling_edges = false, has_inline_attrs = false;
    // the pattern runs against the storage direction: the bound alias is the matrix DESTINATION (cond_traverse.rs:221-235).
    // The reference serves these per row only; expand_batch takes them over the transposed layers (an extension, row-equal)
    bool transposed = false;

    // cond_traverse.rs:308-316: the batched matrix path may run at all
    bool batched_eligible() const;
    // expand_batch (cond_traverse.rs:452-751).  Returns false when the batch must take the per-row path
    // (a non-node source on a non-optional traverse, :566-575); otherwise fills `rows` in emission order
    // and `null_rows` with the active rows an OPTIONAL traverse null-pads (:737-747).
    bool expand_batch(const Graph& g, const std::vector<Value>& src, const std::vector<Value>* to_bound,
                      ExpandedRows& rows, std::vector<u64>& null_rows, u64* flops = nullptr) const;
    // (scan source, final dest) pairs already emitted by an anonymous bidirectional CT whose child is one too
    // (cond_traverse.rs:176-186, 262-299); cleared for every new input batch (:1268-1270)
    struct BidirDedup { std::set<std::pair<u64, u64>> seen; };
    // expand_row + process_pairs (cond_traverse.rs:758-974, 978-1117) without attribute filters: forward pass (over
    // the transposed structure when only the matrix destination is bound), the reverse pass of a bidirectional
    // pattern (self-loops dropped there), label / endpoint checks, per-pair edge lookup (one representative edge
    // unless emit_relationship), cross-row (src, dst) dedup.  An endpoint bound to a non-node gives no rows: the
    // caller does not call.  `dedup_src` = the value of the dedup source alias on this row.
    void expand_row(const Graph& g, std::optional<u64> from_id, std::optional<u64> to_id, bool transposed,
                    const std::vector<u64>& used_edges, std::vector<std::array<u64, 3>>& out,
                    BidirDedup* dedup = nullptr, std::optional<u64> dedup_src = std::nullopt) const;

    // The batches batched_eligible() sends to expand_row, on the device (fgpu_expand_edges): a single hop without static inline
    // attributes that emits the relationship, is bidirectional or has sibling edge aliases.  Fused chains are never any of the
    // three (fuse_anonymous_traverse.rs:83-188), and `cross_row_dedup` — the (scan source, final dest) dedup of :262-299, whose
    // swap_remove order depends on what earlier rows emitted — stays per row.
    bool edges_batch_eligible(bool cross_row_dedup = false) const;
    // Rows of expand_batch_edges: (input row, from, to, edge id) in the order expand_row emits them row by row
    struct EdgeRows {
        std::vector<u64> row, from, to, edge;
        size_t size() const { return row.size(); }
        void push(u64 r, u64 f, u64 t, u64 e) { row.push_back(r); from.push_back(f); to.push_back(t); edge.push_back(e); }
        void clear() { row.clear(); from.clear(); to.clear(); edge.clear(); }
    };
    // expand_row for a whole input batch with ONE fgpu_expand_edges: types and labels resolved as expand_row resolves them; the
    // labels of a side every row has bound are checked with the batched probes of expand_batch, the other side's go along as
    // a bitmap; a row bound to a non-node is skipped (:796-805); a row with both endpoints unbound (the full-matrix walk) runs
    // through expand_row and is spliced in at its place.  `used` (nullable): k * n_used edge ids, row i's sibling-bound ids at
    // used[i * n_used ..] (pad with ~0): the device then runs in all-ids mode and the host drops the used ids and, without
    // emit_relationship, keeps the first survivor of each (row, pass, pair) — exact, because the ids arrive in the reference's
    // scan order.  OPTIONAL: the input rows without an emission go to `null_rows`.  Returns false, with nothing run, when
    // edges_batch_eligible() is false.  stats (nullable): fgpu_expand_edges' eight.
    bool expand_batch_edges(const Graph& g, const std::vector<Value>& from, const std::vector<Value>& to, bool transposed,
                            const u64* used, u64 n_used, EdgeRows& rows, std::vector<u64>& null_rows, u64* stats = nullptr,
                            bool cross_row_dedup = false) const;
};

// ExpandIntoOp (runtime/ops/expand_into.rs:121-258)
struct ExpandIntoOp {
    std::vector<std::string> types;
    bool bidirectional = false;
    bool emit_relationship = true;
    // one row: (src, dst, edge id) triples, types in order, ids ascending per type
    std::vector<std::array<u64, 3>> expand_row(const Graph& g, u64 src, u64 dst,
                                               const std::vector<u64>& used_edges = {}) const;
    // the whole batch with three device probes per type instead of per-pair calls
    void expand_batch(const Graph& g, const std::vector<u64>& srcs, const std::vector<u64>& dsts,
                      std::vector<std::vector<std::array<u64, 3>>>& out) const;
};

// SemiApply / AntiSemiApply (runtime/ops/semi_apply.rs:85-106): a row passes iff (the right branch emits at least one row for
// it) XOR anti.  The right branch is `pattern` fed by the argument batch — the planner's CondTraverse or ExpandInto over the
// pattern predicate (planner/mod.rs:1279-1392).  The reference runs the branch over the batch, emits every match and keeps
// the set of origin rows; a predicate is one bit per row, so the answer comes from one of three tiers, all row-equal:
//   Exists    nothing is expanded.  The matrix path (batched_eligible(), fused chains included) with no row's `to` bound is one
//             fgpu_expand_exists — types, labels and layers resolved as expand_batch resolves them; with every row's `to`
//             bound it is expand_batch's probe (the ExpandInto shape); a bidirectional single hop that emits no relationship
//             and has no sibling edges, `to` unbound, is two fgpu_expand_exists, over the forward and over the transposed
//             layers, OR-ed (the forward pass already sees the self-loops the reverse pass drops).
//   Collect   any other batch-eligible shape, and everything when device_exists is false: expand_batch / expand_batch_edges
//             and the rows that occur — the reference's own method, the baseline.
//   PerRow    otherwise, expand_row row by row.
// A row whose bound alias is Null or not a node emits nothing, so it does not match, and costs no device work.
struct SemiApplyOp {
    CondTraverseOp pattern;
    bool anti = false;
    bool device_exists = true;
    enum Tier { NoRows = 0, Exists = 1, Collect = 2, PerRow = 3 };
    struct Stats {
        int tier = NoRows;
        u64 calls = 0;                    // fgpu_expand_exists calls made
        u64 device[4] = {0, 0, 0, 0};     // their stats summed ([3]: the form of the last call)
    };
    // matched[i] = the branch emits for row i (before `anti`).  `to` nullable: no row has it bound.  `transposed` as
    // expand_row / expand_batch_edges take it: the bound alias `from` is the matrix destination
    void match_batch(const Graph& g, const std::vector<Value>& from, const std::vector<Value>* to, bool transposed,
                     std::vector<uint8_t>& matched, Stats* stats = nullptr) const;
    // the passing input rows, ascending
    void filter_batch(const Graph& g, const std::vector<Value>& from, const std::vector<Value>* to, bool transposed,
                      std::vector<u64>& passing, Stats* stats = nullptr) const;
};

// OrApplyMultiplexer (runtime/ops/or_apply_multiplexer.rs:85-123): every branch sees all rows; a row passes when any branch
// passes, an anti branch inverted by itself.  A branch is a pattern (its SemiApplyOp's own `anti` is not read: the branch's
// flag is) or a caller-supplied boolean column — a filter branch such as `p.id = 0`, which needs the attribute store.
struct OrApplyMultiplexerOp {
    struct Branch {
        std::optional<SemiApplyOp> semi;   // empty: `column`
        std::vector<uint8_t> column;       // one byte per row
        bool anti = false;
        bool transposed = false;
    };
    std::vector<Branch> branches;
    void filter_batch(const Graph& g, const std::vector<Value>& from, const std::vector<Value>* to, std::vector<u64>& passing,
                      std::vector<SemiApplyOp::Stats>* stats = nullptr) const;
};

// CondVarLenTraverse (runtime/ops/cond_var_len_traverse.rs:81-387): the per-row DFS of `(a)-[:T*min..max]->(b)` with
// Cypher trail semantics (a relationship is used at most once per path, nodes may repeat), in the reference's emission
// order: frames leave a LIFO stack, a frame's emissions follow its adjacency order (types in order; per type the
// outgoing edges by (dst, id) ascending, then the incoming ones by (src, id) ascending, a self-loop only once).
// The device is the DFS's pruning oracle when the destination is bound: the nodes that can still reach it within r more
// hops (r = 1 .. max_hops - 1; walks, a superset of trails) come from r boolean products on the device, and a branch that
// is not in the set for its remaining budget is never expanded — the emitted sequence is unchanged, only frames that
// could not emit disappear.  Edge-attribute / WHERE filters need the attribute store (out of scope).
struct VarLenRow {
    u64 from, to;
    std::vector<u64> path;   // emit_path: node, edge, node, ... in pattern order (from -> to); else empty
};
struct VarLenStats {
    u64 frames = 0;          // DFS frames expanded (adjacency lists walked)
    u64 pruned = 0;          // continuations the reach sets cut
    u64 reach_products = 0;  // device products spent on the reach sets
};
struct CondVarLenTraverseOp {
    std::vector<std::string> types;
    std::vector<std::string> dst_labels;   // of the pattern's far endpoint (the one the DFS walks towards)
    bool reversed = false;                 // the bound endpoint is the pattern's `to`: walk incoming edges
    bool bidirectional = false;
    uint32_t min_hops = 1, max_hops = 1;   // UINT32_MAX = unbounded
    bool emit_path = false;
    bool prune = true;                     // use the device reach sets when dest is bound
    // one input row: DFS from `start`; `dest` = the other endpoint when it is bound too
    void expand_row(const Graph& g, u64 start, std::optional<u64> dest, std::vector<VarLenRow>& out,
                    VarLenStats* stats = nullptr) const;

    // expand_row for a whole input batch on the device (fgpu_expand_trails): out holds, rows ascending, exactly what
    // expand_row(g, starts[i], dests[i]) gives for every i, and out_row[j] the input row of out[j].  dests: empty = none bound.
    // Types and destination labels are resolved as expand_row resolves them: unknown types are dropped (with none resolvable the
    // call still runs, for the 0-hop rows), an unknown destination label gives no rows and no device call; the label set goes
    // along as a bitmap.  A row whose start or dest is at or past node_cap(), or deleted, runs through expand_row and is spliced
    // in at its place.  The device holds at most device_budget frames + emissions per call: on FGPU_INSUFFICIENT_SPACE the batch
    // is split in two and each half retried; a single row that does not fit runs expand_row, with `prune` as set.  The device does
    // not prune for a bound destination (the reach sets stay expand_row's): it filters emissions, so a batch of bound rows over
    // long hop ranges pays for every frame — raise device_budget, or leave such rows to expand_row.
    // stats (nullable): frames = the frames of the device calls that answered plus the fallback rows' own; pruned and
    // reach_products count only the fallback rows.  device_calls (nullable): fgpu_expand_trails calls made, refused ones included.
    u64 device_budget = 1ull << 22;
    void expand_batch(const Graph& g, const std::vector<u64>& starts, const std::vector<std::optional<u64>>& dests,
                      std::vector<u64>& out_row, std::vector<VarLenRow>& out, VarLenStats* stats = nullptr,
                      u64* device_calls = nullptr) const;
};

// AllShortestPathsOp (runtime/ops/all_shortest_paths.rs:82-303): MATCH p = allShortestPaths((a)-[:types*..max]->(b)) with both
// endpoints bound.  The reference runs a hash-map BFS from `src` that records every predecessor, then a lazy LIFO DFS from `dst`
// over the predecessors.  Here the BFS is ONE fgpu_shortest_dag call over the pattern matrix — build_adjacency_matrix(types) and
// its transpose, or build_symmetric_adjacency_matrix(types) for both when bidirectional — which returns exactly the
// predecessor pairs the DFS can touch; their relationship ids come from batched tensor probes per type (Tensor::get_batch of
// (u, v), and of (v, u) when bidirectional: no adjacency row of a hub is walked), and the predecessor lists are rebuilt on the
// host in the reference's order: the DAG is walked level by level from src in queue order, per vertex in the adjacency order
// of get_node_relationships_by_type (types in order; per type outgoing by (dst, id), then incoming by (src, id), a self-loop
// once), every relationship of a multi-edge pair a predecessor entry of its own.
// Why the vertices the device never reported are not needed for that order: the reference's queue holds every reached
// vertex, but a vertex v of the DAG at depth d + 1 enters it when the FIRST vertex u at depth d with a relationship to v is
// expanded, and such a u lies on a shortest path src .. u -> v .. dst: it is in the DAG itself.  So the relative queue order of
// the DAG's vertices at a level depends only on the DAG's vertices one level up and on their adjacency order restricted to DAG
// neighbours, by induction from src.
// Edge-attribute filters need the attribute store (out of scope, as for the other operators); min_hops is always 1 (the
// parser refuses anything else, cypher.rs:1324-1331); the shortestPath() function (eval.rs:1296-1513) returns ONE particular path
// and is served by ShortestPathFn below, over a search of its own.
struct AllShortestPathsOp {
    std::vector<std::string> types;
    bool bidirectional = false;
    bool reversed = false;                 // AllShortestPaths::Reversed: the pattern is written right to left (:274, :286-288)
    uint32_t max_hops = UINT32_MAX;        // UINT32_MAX = unbounded (:123)
    // one input row, src / dst = the pattern's from / to node: the paths as relationship-id lists in the reference's emission
    // sequence and per-path edge order (non-cycles src -> dst, reversed again under `reversed`; cycles keep the predecessor
    // chain, :274-289).  limit > 0 stops after that many paths (the reference streams them: a diamond chain holds
    // exponentially many).  *length (nullable) = the paths' length, -1 without one.
    std::vector<std::vector<u64>> expand_row(const Graph& g, u64 src, u64 dst, u64 limit = 0, int64_t* length = nullptr) const;
    // a parent batch of rows, what the reference's operator is fed: out[i] and (*lengths)[i] are what expand_row(g, srcs[i],
    // dsts[i], limit) gives.  The pattern matrix and its transpose are built ONCE, the rows whose nodes are in range and alive
    // go to the device in ONE fgpu_shortest_dag_batch call (no resolvable type: none does), the relationship ids behind the
    // pairs of all rows come from one Tensor::get_batch per type and direction, and every row then takes expand_row's walk.
    // *device_calls (nullable) = the fgpu_shortest_dag_batch calls made: 0 or 1.
    std::vector<std::vector<std::vector<u64>>> expand_batch(const Graph& g, const std::vector<u64>& srcs, const std::vector<u64>& dsts,
                                                            u64 limit = 0, std::vector<int64_t>* lengths = nullptr,
                                                            u64* device_calls = nullptr) const;
};

// shortestPath((a)-[:types*min..max]->(b)) (runtime/eval.rs:1301-1513), an expression the reference evaluates once per row: a
// bidirectional BFS over hash maps that returns ONE path, fixed by the order of its frontiers, by the side it grows (fewer
// frontier vertices) and by the first discoverer of every vertex (the rules are restated in include/fgpu.h).  min_hops is 0 or
// 1 and there is no edge filter (the parser, cypher.rs:1802-1831); for (b)<-[*]-(a) the source is a.
struct ShortestPathFn {
    std::vector<std::string> types;
    bool directed = true;
    uint32_t min_hops = 1;                 // 0 or 1
    uint32_t max_hops = UINT32_MAX;        // UINT32_MAX = unbounded
    struct Path {
        bool null = true;
        std::vector<u64> nodes, edges;     // nodes: length + 1 ids; edges: see below (a pair without a relationship adds none)
    };
    // One row, the CPU mirror of the reference: the rows are walked through the versioned matrices' iterators in the iterator
    // sets of eval.rs:153-217 — no type named: the adjacency forward, every tensor's transpose backward; types named: the
    // existing ones' tensors and transposes, none existing: no iterator, so no path; undirected: both on both sides, sorted and
    // deduplicated — and the search is bfs_shortest_path.  A Null endpoint gives a null path, an endpoint that is not a node
    // throws GrbError "A shortestPath requires bound nodes"; min_hops == 0 with src == dst is the one-node path; a found path
    // shorter than min_hops is null.  The relationship of each consecutive pair (u, v) is the first id of
    // get_src_dest_relationships(u, v, types) (graph.rs:2496-2513: types in the order given, or the graph's; ids in Tensor::get's
    // order), else the first of (v, u) — tried in the directed case too — else none.
    Path eval_row(const Graph& g, const Value& src, const Value& dst) const;
    // A parent batch of rows: out[i] equals eval_row(g, srcs[i], dsts[i]).  F and B are built ONCE
    // (build_adjacency_matrix(types) and its transpose, or build_symmetric_adjacency_matrix(types) for both), every row whose two
    // nodes are below node_cap() and alive and differ goes to ONE fgpu_shortest_path_batch call (no resolvable type: none
    // does), the ids of all rows' pairs come from one Tensor::get_batch per type and direction, and the other rows go through
    // eval_row in place.  *device_calls (nullable) = the fgpu_shortest_path_batch calls made: 0 or 1.
    std::vector<Path> eval_batch(const Graph& g, const std::vector<Value>& srcs, const std::vector<Value>& dsts,
                                 u64* device_calls = nullptr) const;
};

// indegree(n [, types]) / outdegree(n [, types]) (runtime/functions/entity.rs:268-381, runtime.rs:1727-1796, graph.rs:1839-1887):
// an expression, evaluated per row by the reference as one versioned row iterator per node and tensor with every id of a
// multi-edge list walked.  Types as parse_degree_args + get_node_*degree_by_type resolve them: none named = every tensor; a
// name listed twice counts once (entity.rs:340, :367); an unknown name is dropped; names of which none is known answer 0.
// The value is the graph's own count, pending creations and deletions (dp / dm) included; what the reference's runtime adds
// for the query's uncommitted `Pending` overlay (runtime.rs:1737-1741) stays with the caller.  A node id at or past
// node_cap() throws std::out_of_range before any result; a deleted node's rows are empty once its relationships are gone, so
// it answers 0.
struct DegreeFn {
    bool incoming = false;
    std::vector<std::string> types;
    // one row: the reference's loop, the count of get_node_relationships_by_type in the one direction.  No device degree call.
    u64 eval_row(const Graph& g, u64 id) const;
    // a parent batch: out[i] = eval_row(g, ids[i]).  The layers and multi-edge tables of the resolved tensors go to ONE
    // fgpu_node_degrees call per 64 of them, summed across the groups.  *device_calls (nullable) = the calls made.
    std::vector<u64> eval_batch(const Graph& g, const std::vector<u64>& ids, u64* device_calls = nullptr) const;
    // every node id below node_cap(), through the call's whole-graph form: node_cap() values
    std::vector<u64> eval_all(const Graph& g, u64* device_calls = nullptr) const;
};

struct BfsResult {
    bool has_row = false;
    std::vector<u64> nodes, edges;
};
// algo.BFS (runtime/functions/algo_procedures.rs:1021-1160)
// `gang` (nullable): contexts of the GPUs to partition the search over (one nnz-balanced column slab each; gang[0] is
// normally the graph's own context); the level loop and the frontier exchange then run inside libfgpu.so
// (fgpu_bfs_dist_run).  Same results as the single-device call.
BfsResult algo_bfs(const Graph& g, std::optional<u64> source, int64_t max_depth,
                   const std::optional<std::string>& rel_type, bool want_edges,
                   const std::vector<Context*>* gang = nullptr);

// ---- planner slice: the rule that decides which queries reach the fused chain ---------------------------
// (planner/optimizer/fuse_anonymous_traverse.rs).  The model keeps only what the rule inspects.
struct PlanNodeRef {
    std::string alias;                 // "_anon*" = anonymous (fuse_anonymous_traverse.rs:38-40)
    std::vector<std::string> labels;
    bool attrs_empty = true;           // inline attribute map is `{}` (:55-63)
};
struct PlanRel {                       // QueryRelationship
    std::string alias;
    PlanNodeRef from, to;
    std::vector<std::string> types;
    bool bidirectional = false;
    bool var_len = false;              // min_hops.is_some()
    bool attrs_empty = true;           // :43-53
};
struct PlanOp {
    enum Kind { CondTraverse, Other, Pruned } kind = Other;
    int parent = -1;
    std::vector<int> children;
    // IR::CondTraverse (planner/mod.rs:183-213)
    PlanRel rel;
    bool emit_relationship = false, transposed = false, optional = false, bind_relationship = true;
    std::vector<std::string> sibling_edges;
    std::vector<PlanRel> chain;
    // any other IR node: its name and the aliases its expressions reference (reduce_expand_into.rs:22-75)
    std::string name;
    std::vector<std::string> references;
};
struct Plan {
    std::vector<PlanOp> ops;           // index = node id
    int root = -1;
};
bool can_fuse(const Plan& plan, int parent_idx, int child_idx);            // fuse_anonymous_traverse.rs:83-188
void fuse_anonymous_traverse(Plan& plan);                                   // :190-284
CondTraverseOp lower_cond_traverse(const PlanOp& op);                       // plan node -> runtime operator
Plan parse_plan(const std::string& text);                                   // text form: see planner.cpp
std::string print_plan(const Plan& plan);

struct PageRankResult {
    std::vector<u64> nodes;
    std::vector<double> scores;   // Column::Floats: the FP32 centrality widened (extract_vector_f64)
};
// algo.pageRank (runtime/functions/algo_procedures.rs:687-783): label / rel_type NULL = all
PageRankResult algo_pagerank(const Graph& g, const std::optional<std::string>& label,
                             const std::optional<std::string>& rel_type);

struct WccResult {
    std::vector<u64> nodes;
    std::vector<int64_t> component_ids;   // Column::Ints
};
// algo.WCC (runtime/functions/algo_procedures.rs:789-880): labels / types empty = all; several labels select the UNION of
// their nodes (collect_node_ids, :456-477)
WccResult algo_wcc(const Graph& g, const std::vector<std::string>& labels, const std::vector<std::string>& types);

struct CdlpResult {
    std::vector<u64> nodes;
    std::vector<int64_t> community_ids;   // Column::Ints
};
// algo.labelPropagation (runtime/functions/algo_procedures.rs:1168-1270): labels / types empty = all; several labels select
// the UNION of their nodes; max_iterations <= 0 throws "maxIterations must be a positive integer" (:1184-1193, default 10)
CdlpResult algo_cdlp(const Graph& g, const std::vector<std::string>& labels, const std::vector<std::string>& types,
                     int64_t max_iterations);

struct HarmonicResult {
    std::vector<u64> nodes;
    std::vector<double> scores;       // Column::Floats
    std::vector<int64_t> reachable;   // Column::Ints
};
// algo.HarmonicCentrality (runtime/functions/algo_procedures.rs:2623-2784): labels / types empty = all; several labels select
// the UNION of their nodes; an unknown relationship type throws "Relationship type '<t>' does not exist" (:2648-2652)
HarmonicResult algo_harmonic_centrality(const Graph& g, const std::vector<std::string>& labels,
                                        const std::vector<std::string>& types);

struct BetweennessResult {
    std::vector<u64> nodes;
    std::vector<double> scores;   // Column::Floats
};
// algo.betweenness' source rule (runtime/functions/algo_procedures.rs:898-975): samplingSize <= 0 throws; the value is cast
// `as i32` then `as usize`, the seed `as u64`; n_nodes <= size gives every index, otherwise `size` draws (seed 0: i % n_nodes,
// else an LCG), repeats dropped, first-seen order kept
std::vector<u64> betweenness_sources(u64 n_nodes, int64_t sampling_size, int64_t sampling_seed);
// algo.betweenness (runtime/functions/algo_procedures.rs:884-1017): labels / types empty = all; several labels select the
// UNION of their nodes, and a source index then means the k-th selected node in ascending id order
BetweennessResult algo_betweenness(const Graph& g, const std::vector<std::string>& labels, const std::vector<std::string>& types,
                                   int64_t sampling_size, int64_t sampling_seed);

// The (row, col, value) result arrays of one engine call (fgpu_msf's forest, fgpu_maxflow's flow): n triples in (row, col)
// order, owned here and returned to the context's result pool with the scope.
struct EdgeList {
    EngineBuf<u64> rows, cols;
    EngineBuf<double> vals;
    u64 n = 0;
    explicit EdgeList(const Context& ctx) : rows(ctx.raw()), cols(ctx.raw()), vals(ctx.raw()) {}
};
// fgpu_msf / fgpu_maxflow into an EdgeList of `ctx`; a failure throws as check() does, named after the LAGraph call
inline void msf(const Context& ctx, const fgpu_mat* w, const u64* active_bitmap, int64_t* component, EdgeList& forest) {
    check(fgpu_msf(ctx.raw(), w, active_bitmap, component, forest.rows.out(), forest.cols.out(), forest.vals.out(), &forest.n, nullptr),
          "LAGraph_msf");
}
inline void maxflow(const Context& ctx, const fgpu_mat* cap, u64 src, u64 sink, double* value, EdgeList& flow) {
    check(fgpu_maxflow(ctx.raw(), cap, src, sink, value, flow.rows.out(), flow.cols.out(), flow.vals.out(), &flow.n, nullptr), "LAGr_MaxFlow");
}
// fgpu_sssp into host arrays of nrows entries (the reference calls no library here: the name is the procedure's)
inline void sssp(const Context& ctx, const fgpu_mat* w, u64 src, double* dist, int64_t* parent) {
    check(fgpu_sssp(ctx.raw(), w, src, dist, parent, nullptr), "algo.SPpaths");
}

struct MsfResult {
    std::vector<std::vector<u64>> tree_nodes;   // per tree, ascending node ids
    std::vector<std::vector<u64>> tree_edges;   // per tree, the relationship id of every forest pair, in forest order
};
// algo.MSF (runtime/functions/algo_procedures.rs:1272-1857): labels / types empty = all; several labels select the UNION of
// their nodes; an unknown relationship type throws "Relationship type '<t>' does not exist" (:1287-1295).  The host mirror has
// no attribute store: the weight attribute arrives as (edge_ids[k], weights[k]), k < n_weights; edge_ids == nullptr means no
// weightAttribute (every score 1.0), an edge id that is not listed is the missing-attribute case and scores +inf under either
// objective (msf_score, :143-165).  Every unordered node pair keeps the relationship with the smallest score over the selected
// types and its multi-edges, ties to the smallest id (msf_keep_min_score, :237-255); the forest is fgpu_msf's.  Trees come in
// ascending order of their smallest node id; an isolated selected node is a tree without edges.
MsfResult algo_msf(const Graph& g, const std::vector<std::string>& labels, const std::vector<std::string>& types, bool maximize,
                   const u64* edge_ids, const double* weights, u64 n_weights);

struct MaxFlowResult {
    std::vector<u64> nodes;      // ascending endpoints of the relationships with non-zero flow
    std::vector<u64> edges;      // those relationships, in the order Tensor::iter_edges yields the type's edges
    std::vector<double> flows;   // their flows
    double max_flow = 0.0;
};
// algo.maxFlow (runtime/functions/algo_procedures.rs:2786-3248).  Exactly one relationship type, which must exist and hold no
// multi-edge; sources / targets non-empty and disjoint; labels empty = all nodes, else an edge counts when both its ends carry
// one of the labels.  The host mirror has no attribute store: the capacity attribute arrives as (edge_ids[k], caps[k]),
// k < n_caps, has_attribute says whether the graph knows the attribute name at all.  A relationship whose listed capacity is
// >= 0 uses it; any other relationship (not listed, negative, NaN) uses default_capacity when has_default, else the call fails.
// Capacities <= 0 are dropped before the solve; max >= min * (2^32 - 1) over the positive ones fails.  Node ids are used as
// they are when there is no label filter and no deleted node, else they are compacted (sorted distinct ends, sources and
// targets); several sources (targets) hang under a super-source (-sink) by arcs of 2^31 - 1, which never show in the result.
// The flow is fgpu_maxflow's: the value is unique, the assignment is one of the maximum flows.
MaxFlowResult algo_maxflow(const Graph& g, const std::vector<std::string>& labels, const std::vector<std::string>& types,
                           const std::vector<u64>& sources, const std::vector<u64>& targets, bool has_attribute,
                           const u64* edge_ids, const double* caps, u64 n_caps, bool has_default, double default_capacity);

enum class Direction { Outgoing, Incoming, Both };   // relDirection: 'outgoing' | 'incoming' | 'both'
struct SpPathResult {
    bool found = false;
    std::vector<u64> nodes, edges;   // the path source .. target and the relationship of every step
    double weight = 0, cost = 0;
};
// algo.SPpaths (runtime/functions/algo_procedures.rs:2548-2597), its fast branch ONLY: one cheapest path, no maxLen, no
// maxCost, source != target — what run_path_algo hands to dijkstra_single_path (:2563-2571, :2156-2257).  Every other shape
// (pathCount 0 or > 1, maxLen, maxCost) and all of algo.SSpaths enumerate simple paths on the host: algo_sp_paths_rows and
// algo_ss_paths below, the former pruned by fgpu_sssp_hops' table.
// types empty = every tensor; unknown names are dropped and a name listed twice counts once (get_node_relationships_by_type's
// filter_map).  source == target gives found = false, with or without a self-loop (:2559-2567); so does a source or target that
// is deleted or out of range.  The host mirror has no attribute store: weightProp arrives as (w_edge_ids[k], w_vals[k]),
// k < n_w, w_edge_ids == nullptr = not given; a relationship that is not listed weighs 1.0 (edge_numeric_attr, :2049-2062);
// costProp likewise with 0.0.  A relationship whose weight is NaN or +-inf can never be relaxed in the reference and is left
// out.  The reference documents negative weights as unsupported with undefined results; here one throws std::invalid_argument
// naming the relationship.  The search runs over one matrix entry per ordered pair (from, to) in traversal direction — src ->
// dst (Outgoing), dst -> src (Incoming), both (Both), self-loops dropped — that carries the smallest weight over the selected
// types and their multi-edges, ties to the smallest relationship id (the engine's rule, as algo_msf's; the reference keeps
// whichever its iteration meets first): a BOOL matrix without weightProp, binary64 bit patterns otherwise.  The path is
// fgpu_sssp's parent chain from target back to source; edges[k] is the kept relationship of pair k, weight = dist[target], cost
// the costs of those relationships folded source -> target in that order (:2250-2254).
SpPathResult algo_sp_paths(const Graph& g, u64 source, u64 target, const std::vector<std::string>& types, Direction dir,
                           const u64* w_edge_ids, const double* w_vals, u64 n_w,
                           const u64* c_edge_ids, const double* c_vals, u64 n_c);

// fgpu_sssp_hops into a host array of (max_hops + 1) * nrows entries
inline void sssp_hops(const Context& ctx, const fgpu_mat* w, u64 src, int32_t max_hops, double* table) {
    check(fgpu_sssp_hops(ctx.raw(), w, src, max_hops, table, nullptr), "algo.SPpaths");
}

// Every shape of algo.SPpaths, and algo.SSpaths: run_path_algo (:2548-2597) whole.
struct PathQuery {
    std::vector<std::string> types;            // relTypes: empty = every tensor; unknown names are dropped, a name listed twice
                                               // contributes its relationships twice (get_node_relationships_by_type's filter_map)
    Direction dir = Direction::Outgoing;       // relDirection
    uint32_t max_len = UINT32_MAX;             // maxLen (UINT32_MAX = not given)
    std::optional<double> max_cost;            // maxCost
    int64_t path_count = 1;                    // pathCount: 1 the cheapest, 0 all of minimum weight, k > 1 the k cheapest
    const u64* w_edge_ids = nullptr;           // weightProp / costProp as algo_sp_paths takes them
    const double* w_vals = nullptr;
    u64 n_w = 0;
    const u64* c_edge_ids = nullptr;
    const double* c_vals = nullptr;
    u64 n_c = 0;
    bool prune = true;                         // algo_sp_paths_rows: skip what the hop-bounded table rules out
    u64 max_examined = 0;                      // budget of popped successors, 0 = none (stands for the reference's timeout poll)
};
struct PathRow {
    std::vector<u64> nodes, edges;             // source .. end, and the relationship of every step
    double weight = 0, cost = 0;
};
struct PathEnumStats {
    u64 examined = 0;                          // successors popped
    u64 pruned_hops = 0, pruned_weight = 0;    // skipped: cannot end at the target within maxLen / only above the bound
    int32_t table_rows = -1;                   // rows of the table the walk was pruned with; -1 none, 0 = fgpu_sssp's one row
};
// algo_sp_paths_rows: the fast shape (pathCount 1, no maxLen, no maxCost, source != target) is algo_sp_paths.  Everything else
// mirrors enumerate_paths + record_found_path + the final stable sort by cmp_found_path (:2350-2514, :2594-2595) step by step:
// successors in get_node_relationships_by_type's order popped from the back, prefix sums kept per edge, the non-finite tests
// on next_weight and next_cost, nothing extended past the target, the k-list insertion by partition_point (a new path goes in
// front of its equals; a candidate that is not Less than the last kept one is dropped).  pathCount < 0 throws
// std::invalid_argument("pathCount must be a non-negative integer") (:1940); a negative weight among the selected
// relationships throws as algo_sp_paths does; a spent max_examined throws std::runtime_error.
//
// Pruning (q.prune).  The reference's walk enters every prefix under the current weight bound, also those that can never END
// at the target within maxLen.  Which those are is a matrix question: Wrev = the min-weight matrix per ordered pair in the
// REVERSE traversal direction (algo_sp_paths' builder with Outgoing and Incoming swapped), and
//   table[r][v] = fgpu_sssp_hops(Wrev, target, maxLen)[r][v] = the cheapest way from v to the target in at most r arcs
// when maxLen <= 32 and the table is at most 1 GiB; otherwise the one row fgpu_sssp(Wrev, target) gives.  That row knows no
// hop budget: it is a valid (weaker) LOWER bound on what is left to the target under every budget, so it may prune, but below
// maxLen = n - 1 it is not the weight of a qualifying path (the cheapest route may need more than maxLen arcs) — there it
// neither seeds the bound nor answers bfs_find_bound's question, which a host BFS within maxLen answers instead.  With m = min(maxLen, n - 1) + 1, slack = 8 m 2^-53, and, for a successor `next`
// pushed as arc number len, L = table[maxLen - len][next]:
//   - L == +inf: no simple path through this prefix ends at the target in time — skipped (pruned_hops);
//   - (next_weight + L) (1 - slack) > bound: every completion weighs more than the bound — skipped (pruned_weight);
//   - the bound starts at table[maxLen][source] (1 + slack) when pathCount is 0 or 1, there is no maxCost and the table is
//     hop-exact (the hop table, or the one row with maxLen >= n - 1), else at +inf;
//   - table[maxLen][source] == +inf returns no rows (bfs_find_bound's None, :2579-2581), and so does, under the one row with
//     maxLen < n - 1, a target the host BFS does not reach within maxLen.
// Why the rows are the reference's.  (1) A skipped branch holds only paths that do not reach the target within maxLen, or
// whose forward-folded weight exceeds the bound of that moment; the reference cuts each of the latter at some prefix before or
// at the target (its `next_weight > bound` test), and bounds only fall: the sequence of record_found_path calls that change
// anything is the same.  (2) The result does not depend on the seed as long as the seed is at least the forward-folded weight
// of a cheapest qualifying path: pathCount 1 keeps the first path in DFS order of the cmp-minimal class, pathCount 0 keeps all
// paths of minimum weight in DFS order, and both sets lie under either seed.  (3) The slack covers the two folds: the table
// adds a route's weights from the target outward, the walk from the source outward.  For k <= m non-negative terms each fold
// is within a factor (1 +- g) of the exact sum S, g = (k - 1) u / (1 - (k - 1) u), u = 2^-53 (Higham, Accuracy and Stability,
// Lemma 3.1; no cancellation: all terms >= 0), so fold_a <= S (1 + g) <= fold_b (1 + g) / (1 - g) <= fold_b (1 + 3 m u) for
// m u < 1/8.  A completion of weight fold_fwd <= bound therefore has (next_weight + L) <= fold_fwd (1 + 3 m u)(1 + u), below
// bound / (1 - 8 m u); the seed likewise stays above the forward fold of the table's own cheapest route.
// A source or target that is deleted or out of range gives no rows.
std::vector<PathRow> algo_sp_paths_rows(const Graph& g, u64 source, u64 target, const PathQuery& q, PathEnumStats* stats = nullptr);
// algo.SSpaths: the same walk with no target — every non-empty simple path from source qualifies.  There is nothing to bound
// against, so no device call is made (table_rows stays -1, q.prune is ignored).
std::vector<PathRow> algo_ss_paths(const Graph& g, u64 source, const PathQuery& q, PathEnumStats* stats = nullptr);

}  // namespace falkor
