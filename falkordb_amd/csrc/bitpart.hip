// bitpart.hip — the dense COUNTING hop of the bit-parallel k-hop chain with the rows of X partitioned BY XCD.
//
// What bounds the plain dense pull (bitexpand.hip bp_pull_kernel<.., dense, count>), measured in round 5
// (tools/micro/gatherq.hip, profiles/r05a_gatherq*.{txt,json}): a gather that misses the XCD's L2 costs one 128-byte LINE of
// the Infinity-Cache / HBM path whatever it wanted from it (4 B, a 64-byte row, a 128-byte row: 1 TCC_EA0_RDREQ each), and
// that path serves ~57 G lines/s (MALL-resident) / ~49.5 G lines/s (HBM) — 7.3 / 6.3 TB/s — saturated from 16 wavefronts x 1
// gather per CU, from ~100 of the 256 CUs, with no second path (scalar loads: 25 G rows/s, LDS-DMA: the same queue).  The hop
// ran AT that limit (6.0 GB of lines per launch in 1.01 ms at RMAT-22): it is bound by the NUMBER OF MISSED LINES.  Every XCD
// gathers from the whole of X, so the eight 4 MiB L2s hold the same hottest rows (simulated LRU hit rate 0.35, measured
// traffic within 5 % of the simulation's).  Here workgroup b only gathers rows of partition b & 7 — workgroups are dealt to
// the XCDs round-robin — so X is cached ONCE across the chip (32 MiB instead of 4): simulated hit rate 0.75, X traffic 5.4 ->
// 2.1 GB at RMAT-22.  A row v of A' then receives a PARTIAL row from each of the (up to 8) partitions its in-neighbours fall
// into: partial rows are written once, compact and in order (~1 GB written + read at RMAT-22: sequential traffic, not
// gathers), and a fold kernel ORs them per vertex and counts / check-sums the complete row exactly where the plain pull did.
//
// Round 4's BpHotPlan was the same idea restricted to "hot" (v, u) pairs, a wavefront per (row, partition) segment of 4-8
// entries: item-bound.  Here the entries of a partition, sorted by row, are ONE STREAM: a (partition, row) pair with entries
// is a run of the stream (its first entry carries a flag in bit 31 of the column id), run k of the whole stream produces
// partial row k, and the pull is a segmented OR-reduction over chunks of the stream (<= XP_SPAN entries and <= XP_RUNS runs,
// cut once per snapshot) — a wavefront per chunk, 64 entries per trip (a coalesced 4-byte load per lane), QL consecutive
// entries per slot, their rows of X gathered QL at a time with the NEXT trip's gathers already in flight; a slot ORs the
// entries of one run in registers and flushes into the chunk's tile of runs in LDS (ds_or_b64) when the run changes; the
// tile leaves as whole rows when the chunk ends.  The chunk loop holds NO global store: on gfx9 stores share vmcnt with
// loads and may complete out of order with them, so one pending store makes hipcc wait for vmcnt(0) — the gathers just
// issued — at every use of a load (the first version wrote finished runs every trip: 723 us).
// No row is long or short: an in-hub with 20 K entries in a partition is a few dozen chunks of one run each, whose pieces
// meet in the (pre-zeroed) partial row through atomics — the only atomics of the kernel, at most two rows per chunk.
#include <algorithm>

#include "bitexpand.hpp"

namespace fgpu {

// partition(u) = u / prange with prange = ceil(ncols / 8) rounded up to 16 rows (whole 128-byte lines from 8-byte rows up): eight
// CONTIGUOUS ranges of X.  (The first version took bits 4..6 of u — every 8th block of 16 rows: the rows of a partition then
// share three address bits, the L2's channel interleave uses address bits of that order, and a partition reached only a
// fraction of its XCD's 16 channels: measured hit rate ~0.45 where the LRU simulation of a whole L2 gives 0.75.)
constexpr u32 XP_FIRST = 0x80000000u;   // bit 31 of a packed entry: first entry of its (partition, row) run
constexpr u32 XP_SPAN = 768;       // a chunk spans < XP_SPAN of the key (entry index + XP_RUNW x run index) inside its partition:
constexpr u32 XP_RUNW = 8;         //   <= XP_SPAN entries and <= XP_RUNS runs (the rows of its LDS tile)
constexpr int XP_FOLD_THREADS = 512;   // 8 wavefronts share one copy of the checksum tables
constexpr u32 XP_RUNS = XP_SPAN / XP_RUNW;
constexpr u32 XP_NO_VTX = 0xFFFFFFFFu; // gvtx of a padded slot of the last dense group (rows < 0xFFFFFFC0)

struct BpXPlan {
    bool usable = false;
    u32 n = 0, ng = 0;             // rows of A' (destinations), 64-row groups of the fold (of vertex ids, or of ranks: `dense`)
    // dense groups (expand_xp_dense = 1): a row of A' without an entry never has a piece, and at RMAT-22 that is 52 % of the rows,
    // spread evenly (scrambled ids) — in every group of 64 vertex ids about 33 lanes do the index work, and then the look-ups, of
    // a row that is zero by construction.  The rows that HAVE an entry are ranked in vertex order, the group tables below are
    // built over 64 consecutive RANKS, and gvtx names the vertex of a slot where the fold needs it (hash, label, touched bit).
    int cut = 0;                   // the chunk cut the plan was built under and HOLDS (1: whole double trips, xp_cut_cells; 0: the key cut)
    int dense = 0;                 // the form the plan was built under (0: group g = vertices 64 g .. 64 g + 63, gvtx stays null)
    u32 nd = 0;                    // rows of A' with at least one entry (dense form; ng = ceil(nd / 64))
    DevBuf<u32> gvtx;              // [ng * 64] vertex of slot 64 g + r, XP_NO_VTX past rank nd - 1 (a padded slot: no piece, no vertex)
    u64 nentries = 0;
    u32 nprows = 0;                // partial rows = runs = non-empty (partition, row) pairs
    u32 nchunks = 0;
    DevBuf<u32> pcol;              // the entries, partition-major, rows ascending inside a partition: XP_FIRST | column id
    u32 pstart[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};   // first entry of partition k
    u32 cbase[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};    // first chunk of partition k
    DevBuf<u32> pstart_dev;        // [9] + cbase [9]
    DevBuf<u32> cstart;            // first entry of the chunk
    DevBuf<u32> crun0;             // run (= partial row) of the chunk's first entry
    DevBuf<uint8_t> cshared;       // 1: that run began in an earlier chunk (its pieces meet through atomics)
    DevBuf<u32> zrows;             // the partial rows that receive pieces from several chunks (zeroed before every hop)
    u32 nzrows = 0;
    DevBuf<u64> ne;                // [8][ng] bit r: (partition, row 64 g + r — dense: the row of slot 64 g + r) has entries in the stream
    DevBuf<u32> pbase;             // [8][ng] partial row of the group's first non-empty row
    // direct entries (expand_xp_direct = 1): a (partition, row) run of ONE entry is left out of the stream — its partial row would
    // be a copy of one row of X, gathered, flushed through the tile, written and read back — and the fold reads that row of X
    // itself.  At RMAT-22 these are 43 % of the runs (the partial rows) and 5 % of the entries, most of them hot rows of X.
    int direct = 0;                // the mode the plan was built under (0: every run is streamed, de / dbase / dcol stay null)
    u64 ndirect = 0;
    DevBuf<u64> de;                // [8][ng] bit r: (partition, row 64 g + r) is one direct entry
    DevBuf<u32> dbase;             // [8][ng] index in dcol of the group's first direct entry
    DevBuf<u32> dcol;              // the direct entries' columns (slots of X, like pcol's), partition-major, rows ascending
    // slot of X's row u in the state this plan gathers from (nullptr: slot = u).  Rows are ranked by how often they are gathered
    // (out-degree of u in m, descending) and dealt to the partitions in turn — slot = (rank % 8) x range + rank / 8 — so every
    // partition holds an eighth of the hot rows, packed hot-first: a 128-byte line then carries two rows (64-byte rows) of about
    // the same heat, where vertex order puts a hot row next to a random one — the L2's capacity for hot rows doubles
    // (simulated: hit rate 0.75 -> 0.85 at RMAT-22).  The hop that PRODUCES the state writes row v at slot perm[v] (bitexpand.hip).
    DevBuf<u32> perm;
    // the top hub's out-rows (bp_xplan_hub below).  h = the row of m with the most entries (smallest id on a tie); out(h) = the
    // rows of A' that have h as an in-neighbour.  When row slot(h) of X is all ones, every row of out(h) of Y is all ones
    // with no gather at all, and the hop runs under `hub`: the plan of A' with the rows out(h) emptied, gathering from the SAME
    // layout of X (it is built with this plan's perm and keeps none of its own).  Only the full plan of a triple carries these.
    BpXPlanPtr hub;                // null: no reduced plan (share of out(h) under XP_HUB_MIN_SHARE, or its build failed: not retried)
    u32 hub_v = 0, hub_slot = 0;   // h and its slot in X (perm[h], or h)
    u32 hub_deg = 0;               // |out(h)|
    u64 hub_dsum = 0;              // sum of cs_dest_hash(v) over out(h), mod 2^64
    DevBuf<u32> hub_rows;          // out(h), as m lists it
    DevBuf<u64> hub_in;            // bit u: u has an edge to h in m (ncols bits): what a scan orders its sources by (spgemm.hip)
    u64 hub_gone = 0;              // entries of A' in the rows out(h)
    // the hub set H (bp_xplan_hub_set_build below): h and the rows of m with at least a quarter of its entries, at most
    // XP_HUB_SET_MAX of them, by (entries descending, id ascending) — H[0] = h.  When EVERY row slot(H[i]) of X is all ones the hop
    // runs under `hub2`, the plan of A' with the rows of the union of out(H[i]) emptied (same layout of X again), and the closed
    // form covers that union.  Kept only beside a level-1 plan.
    BpXPlanPtr hub2;               // null: no second level (|H| < 2, the extra rows' share under XP_HUB_SET_MIN_SHARE, build failed)
    u32 hset_n = 0;                // |H|
    u32 hset_v[32] = {};           // H
    DevBuf<u32> hset_slots;        // [hset_n] slot of H[i] in X
    u32 hset_deg = 0;              // rows in the union of out(H[i]), each once
    u64 hset_dsum = 0;             // sum of cs_dest_hash over them
    DevBuf<u32> hset_rows;         // the union, ascending
    DevBuf<u32> hub_mask;          // [ncols of A'] bit i of word u: (u, H[i]) is an entry of m
    const BpXPlan* full = nullptr; // on a reduced plan: the full plan that owns it
};
const u32* bp_xplan_perm(const BpXPlan* p) { return p ? p->perm.p : nullptr; }
void BpXPlanDelete::operator()(BpXPlan* p) const { delete p; }

// ---- plan build (once per snapshot) ----------------------------------------------------------------------------------------
// The entries of A' arrive partitioned by the slot range of their column (partition_csr_entries, transpose.hip: one
// LDS-staged stable partition pass, (slot, row) pairs — the walk that did this with one atomic and one scattered 4-byte store
// per entry took 3.5 + 4.1 ms at RMAT-22, three times the transpose itself).  What is left: the flag on the first entry of
// every (partition, row) run, and where every run starts — off[x * n + v] for ALL rows v, those without entries included,
// which a position that opens a run fills for the rows since the previous run.
__global__ __launch_bounds__(256) void xp_runs_kernel(const uint2* __restrict__ pairs, const u32* __restrict__ pstart, u32 n, u32 nnz,
                                                      u32* __restrict__ pcol, u32* __restrict__ off) {
    __shared__ u32 s_ps[9];
    if (threadIdx.x < 9) s_ps[threadIdx.x] = pstart[threadIdx.x];
    __syncthreads();
    const u32 lane = lane_id();
    const u32 wave = (blockIdx.x * 256 + threadIdx.x) >> 6, nwaves = (gridDim.x * 256) >> 6;
    for (u32 p0 = wave * 64; p0 < nnz; p0 += nwaves * 64) {
        const u32 p = p0 + lane;
        u32 g0 = 0, g1 = 0;                       // rows (g0 .. g1] of partition x start at p
        size_t base = 0;
        if (p < nnz) {
            u32 x = 0;
#pragma unroll
            for (u32 k = 1; k < 8; ++k) x += p >= s_ps[k] ? 1u : 0u;
            const uint2 e = pairs[p];
            const bool head = p == s_ps[x];
            const u32 prev = head ? 0xFFFFFFFFu : pairs[p - 1].y;
            const bool first = head || e.y != prev;
            pcol[p] = e.x | (first ? XP_FIRST : 0u);
            if (first) { g0 = prev + 1u; g1 = e.y + 1u; base = (size_t)x * n; }   // (prev + 1 wraps to 0 at the head)
        }
        for (int j = 0; j < 2 && g0 < g1; ++j, ++g0) off[base + g0] = p;          // the usual case: the row itself, one empty row
        u64 more = __ballot(g0 < g1);
        while (more) {                            // a long stretch of rows without entries: the whole wavefront fills it
            const int l = (int)__builtin_ctzll(more);
            more &= more - 1ull;
            const u32 a = (u32)__builtin_amdgcn_readlane((int)g0, l), b = (u32)__builtin_amdgcn_readlane((int)g1, l);
            const u32 at = (u32)__builtin_amdgcn_readlane((int)p, l);
            const u64 bs = ((u64)(u32)__builtin_amdgcn_readlane((int)(u32)((u64)base >> 32), l) << 32) |
                           (u64)(u32)__builtin_amdgcn_readlane((int)(u32)base, l);
            for (u32 r = a + lane; r < b; r += 64) off[bs + r] = at;
        }
    }
}
// the rows after a partition's last run (all of them when it has none) start where the partition ends
__global__ __launch_bounds__(256) void xp_run_tails_kernel(const uint2* __restrict__ pairs, const u32* __restrict__ pstart, u32 n,
                                                           u32* __restrict__ off) {
    const u32 x = blockIdx.y;
    const u32 b = pstart[x], e = pstart[x + 1];
    const u32 from = e > b ? pairs[e - 1].y + 1u : 0u;
    for (u32 r = from + blockIdx.x * 256 + threadIdx.x; r < n; r += gridDim.x * 256) off[(size_t)x * n + r] = e;
    if (x == 7 && blockIdx.x == 0 && threadIdx.x == 0) off[(size_t)8 * n] = pstart[8];
}
__global__ void xp_nonempty_kernel(const u32* __restrict__ off, u64 total, u32* __restrict__ nz) {
    for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i <= total; i += (u64)gridDim.x * 256) nz[i] = (i < total && off[i + 1] != off[i]) ? 1u : 0u;
}
// the dense form's slots: flag[v] = row v of A' has an entry (flag[n] = 0), and — after the exclusive scan of the flags —
// gvtx[rank] = v.  (The slots of the last group past rank nd - 1 keep XP_NO_VTX from the memset.)
__global__ void xp_has_entry_kernel(const u32* __restrict__ rowptr, u32 n, u32* __restrict__ flag) {
    for (u32 v = blockIdx.x * 256 + threadIdx.x; v <= n; v += gridDim.x * 256) flag[v] = v < n && rowptr[v + 1] != rowptr[v] ? 1u : 0u;
}
__global__ void xp_slots_kernel(const u32* __restrict__ rank, u32 n, u32* __restrict__ gvtx) {
    for (u32 v = blockIdx.x * 256 + threadIdx.x; v < n; v += gridDim.x * 256)
        if (rank[v + 1] != rank[v]) gvtx[rank[v]] = v;
}
// a wavefront per (partition, group): the non-empty bitmap and the partial row of the group's first non-empty row.  Slot
// 64 g + r is vertex 64 g + r (gvtx null, nslots = n) or the row of that rank (nslots = nd): the rows between two ranked
// rows have no run in any partition, so the run index at the group's first row is the group's base in both forms.
__global__ __launch_bounds__(256) void xp_groups_kernel(const u32* __restrict__ off, const u32* __restrict__ ridx, u32 n, u32 ng,
                                                        const u32* __restrict__ gvtx, u32 nslots, u64* __restrict__ ne,
                                                        u32* __restrict__ pbase) {
    const u32 lane = lane_id();
    const u32 wave = blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = gridDim.x * 4;
    for (u32 t = wave; t < 8 * ng; t += nwaves) {
        const u32 x = t / ng, g = t % ng;
        const u32 s = g * 64 + lane;
        const bool live = s < nslots;
        const u32 v = !live ? 0u : gvtx ? gvtx[s] : s;        // (lane 0 is always live)
        const size_t i = (size_t)x * n + v;
        const u64 nw = __ballot(live && off[i + 1] != off[i]);
        if (lane == 0) {
            ne[t] = nw;
            pbase[t] = ridx[i];
        }
    }
}
// chunk table: a thread per (partition, row) run.  Inside partition x the key of an entry is (its index in the partition) +
// XP_RUNW x (its run's index in the partition); chunk id = key / XP_SPAN, non-decreasing along the stream and never skipping
// an id (the key grows by <= XP_RUNW + 1 per entry).  A run announces every chunk that BEGINS inside it (or on its first
// entry): the chunk's first entry, the run's index, and whether the run began before the chunk.
__global__ void xp_chunks_kernel(const u32* __restrict__ off, const u32* __restrict__ ridx, u32 n, const u32* __restrict__ pstart,
                                 u32* __restrict__ cstart, u32* __restrict__ crun0, uint8_t* __restrict__ cshared) {
    const u32* cbase = pstart + 9;
    const u32* rbase = pstart + 18;
    const u64 total = 8ull * n;
    for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i < total; i += (u64)gridDim.x * 256) {
        const u32 b = off[i], e = off[i + 1];
        if (b == e) continue;
        const u32 x = (u32)(i / n);
        const u32 ps = pstart[x];
        const u64 rr = ridx[i] - rbase[x];                   // run index inside the partition
        const u64 kb = (u64)(b - ps) + XP_RUNW * rr;         // key of the run's first entry
        const u64 ke = (u64)(e - 1 - ps) + XP_RUNW * rr;     // ... of its last
        const long long prev = b == ps ? -1ll : (long long)((kb - 1 - XP_RUNW) / XP_SPAN);   // chunk of the entry before the run
        long long c = (long long)(kb / XP_SPAN);
        if (c <= prev) c = prev + 1;
        for (; c <= (long long)(ke / XP_SPAN); ++c) {
            const u64 first_key = (u64)c * XP_SPAN;          // smallest key of chunk c
            const u32 st = first_key > kb ? ps + (u32)(first_key - XP_RUNW * rr) : b;
            cstart[cbase[x] + c] = st;
            crun0[cbase[x] + c] = ridx[i];
            cshared[cbase[x] + c] = st != b;
        }
    }
}

// ---- the cut on whole double trips (expand_xp_cut = 1) ----------------------------------------------------------------------------
// The stream kernel consumes two trips of 64 entries per iteration, so a chunk of 128 k + r entries runs on copies of its last
// entry for the 128 - r slots that are missing (bitpart.hip xp_stream_kernel).  Here every chunk but a partition's last holds a
// multiple of 128 entries: a partition is counted off in CELLS of 128 entries and SUPER-CELLS of five cells from its first
// entry; a super-cell that touches at most XP_RUNS runs (the rows of the tile) is one chunk, any other is cut into its cells.
// With the single-entry runs taken out (expand_xp_direct = 1) a cell touches at most 65 runs; without, a cell may exceed the
// tile, and such a plan keeps the key cut whole (xp_cut_cells reports it).  Almost every boundary now falls inside a run:
// its pieces meet through cshared / zrows / atomic_or4 as the pieces of an in-hub's run always did.
constexpr u32 XP_CELL = 128, XP_SUPER = 5;
struct XpCells { u32 ps[9], cb[9], sb[9]; };   // first entry, first cell, first super-cell of partition k
__device__ __forceinline__ u32 xp_part_of(const u32 (&base)[9], u32 i) {
    u32 x = 0;
#pragma unroll
    for (u32 k = 1; k < 8; ++k) x += i >= base[k] ? 1u : 0u;
    return x;
}
// a wavefront per cell: the run starts (XP_FIRST flags) among its entries, and whether its first entry is one
__global__ __launch_bounds__(256) void xp_cell_flags_kernel(const u32* __restrict__ pcol, XpCells pc, u32* __restrict__ cnt,
                                                            uint8_t* __restrict__ first) {
    const u32 lane = lane_id();
    const u32 wave = blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = gridDim.x * 4;
    for (u32 c = wave; c <= pc.cb[8]; c += nwaves) {
        u32 k = 0, f = 0;
        if (c < pc.cb[8]) {
            const u32 x = xp_part_of(pc.cb, c);
            const u32 b = pc.ps[x] + XP_CELL * (c - pc.cb[x]), e = pc.ps[x + 1];
            const u64 lo = __ballot(b + lane < e && (pcol[b + lane < e ? b + lane : b] & XP_FIRST));
            const u64 hi = __ballot(b + 64 + lane < e && (pcol[b + 64 + lane < e ? b + 64 + lane : b] & XP_FIRST));
            k = (u32)__popcll(lo) + (u32)__popcll(hi);
            f = (u32)(lo & 1ull);
        }
        if (lane == 0) {
            cnt[c] = k;                                      // (cnt[cells] = 0: the exclusive scan leaves the total there)
            if (c < pc.cb[8]) first[c] = (uint8_t)f;
        }
    }
}
// runs a stretch of cells [c0, c1) touches: the run starts inside it, and the run its first entry continues
__device__ __forceinline__ u32 xp_cells_touch(const u32* g, const uint8_t* first, u32 c0, u32 c1) { return g[c1] - g[c0] + (first[c0] ? 0u : 1u); }
// a thread per super-cell: the chunks it becomes (1, or its cells), and the most runs any CELL that must stand alone touches
__global__ void xp_super_count_kernel(const u32* __restrict__ g, const uint8_t* __restrict__ first, XpCells pc, u32* __restrict__ nch,
                                      u32* __restrict__ worst) {
    for (u32 s = blockIdx.x * 256 + threadIdx.x; s <= pc.sb[8]; s += gridDim.x * 256) {
        u32 k = 0;
        if (s < pc.sb[8]) {
            const u32 x = xp_part_of(pc.sb, s);
            const u32 c0 = pc.cb[x] + XP_SUPER * (s - pc.sb[x]), c1 = c0 + XP_SUPER < pc.cb[x + 1] ? c0 + XP_SUPER : pc.cb[x + 1];
            k = 1;
            if (xp_cells_touch(g, first, c0, c1) > XP_RUNS) {
                k = c1 - c0;
                u32 w = 0;
                for (u32 c = c0; c < c1; ++c) w = max(w, xp_cells_touch(g, first, c, c + 1));
                if (w > XP_RUNS) atomicMax(worst, w);
            }
        }
        nch[s] = k;
    }
}
// what the host needs of the two scans, in one read-back: the first chunk of partition k (k = 8: the chunks) and the worst cell
__global__ void xp_cut_info_kernel(const u32* __restrict__ cbase, XpCells pc, const u32* __restrict__ worst, u32* __restrict__ info) {
    if (threadIdx.x < 9) info[threadIdx.x] = cbase[pc.sb[threadIdx.x]];
    if (threadIdx.x == 9) info[9] = *worst;
}
__global__ void xp_super_fill_kernel(const u32* __restrict__ g, const uint8_t* __restrict__ first, XpCells pc, const u32* __restrict__ cbase,
                                     u32* __restrict__ cstart, u32* __restrict__ crun0, uint8_t* __restrict__ cshared) {
    for (u32 s = blockIdx.x * 256 + threadIdx.x; s < pc.sb[8]; s += gridDim.x * 256) {
        const u32 x = xp_part_of(pc.sb, s);
        const u32 c0 = pc.cb[x] + XP_SUPER * (s - pc.sb[x]);
        const u32 at = cbase[s], k = cbase[s + 1] - at;
        for (u32 i = 0; i < k; ++i) {
            const u32 c = c0 + i;
            cstart[at + i] = pc.ps[x] + XP_CELL * (c - pc.cb[x]);
            crun0[at + i] = g[c] + first[c] - 1u;            // run starts up to and including the chunk's first entry, less one
            cshared[at + i] = first[c] ? 0 : 1;
        }
    }
}

// direct entries (expand_xp_direct = 1).  keep[p] = 0 when entry p is a run of its own: it opens a run and the next entry opens
// another (a partition's first entry opens one) or the stream ends.  The exclusive scan of keep maps every position of the old
// stream to the new one — of an entry that stays: its slot; of one that goes: the next staying entry's — so the run starts
// off[] and the partition starts remap through it, and p - pos[p] numbers the direct entries in stream order.
__global__ void xp_keep_kernel(const u32* __restrict__ pcol, u32 nnz, u32* __restrict__ keep) {
    for (u32 p = blockIdx.x * 256 + threadIdx.x; p <= nnz; p += gridDim.x * 256)
        keep[p] = p < nnz && !((pcol[p] & XP_FIRST) && (p + 1 == nnz || (pcol[p + 1] & XP_FIRST))) ? 1u : 0u;
}
__global__ void xp_split_kernel(const u32* __restrict__ pcol, const u32* __restrict__ pos, u32 nnz, u32* __restrict__ kept,
                                u32* __restrict__ dcol) {
    for (u32 p = blockIdx.x * 256 + threadIdx.x; p < nnz; p += gridDim.x * 256) {
        const u32 w = pcol[p], q = pos[p];
        if (pos[p + 1] != q) kept[q] = w;
        else dcol[p - q] = w & ~XP_FIRST;
    }
}
// a wavefront per (partition, group), over the OLD run starts: the direct bitmap and the direct index of the group's first row
__global__ __launch_bounds__(256) void xp_direct_groups_kernel(const u32* __restrict__ off, const u32* __restrict__ pos, u32 n, u32 ng,
                                                               const u32* __restrict__ gvtx, u32 nslots, u64* __restrict__ de,
                                                               u32* __restrict__ dbase) {
    const u32 lane = lane_id();
    const u32 wave = blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = gridDim.x * 4;
    for (u32 t = wave; t < 8 * ng; t += nwaves) {
        const u32 x = t / ng, g = t % ng;
        const u32 s = g * 64 + lane;                         // (slots as in xp_groups_kernel)
        const bool live = s < nslots;
        const u32 v = !live ? 0u : gvtx ? gvtx[s] : s;
        const size_t i = (size_t)x * n + v;
        const u64 dw = __ballot(live && off[i + 1] - off[i] == 1u);
        if (lane == 0) {
            const u32 o = off[i];
            de[t] = dw;
            dbase[t] = o - pos[o];
        }
    }
}
// the run starts and the partition starts, moved to the stream of the staying entries (in place: a thread per word)
__global__ void xp_remap_kernel(u32* __restrict__ off, u64 total, const u32* __restrict__ pos, u32* __restrict__ pstart) {
    const u64 i0 = (u64)blockIdx.x * 256 + threadIdx.x;
    if (i0 < 9) pstart[i0] = pos[pstart[i0]];
    for (u64 i = i0; i <= total; i += (u64)gridDim.x * 256) off[i] = pos[off[i]];
}

__global__ void xp_shared_rows_kernel(const u32* __restrict__ crun0, const uint8_t* __restrict__ cshared, u32 nchunks,
                                      u32* __restrict__ zrows, u32* __restrict__ count) {
    const u32 c = blockIdx.x * 256 + threadIdx.x;
    if (c < nchunks && cshared[c]) zrows[atomicAdd(count, 1u)] = crun0[c];   // (a run over several chunks is listed once per chunk: harmless)
}

// rows of X ranked by out-degree, descending (ties by id): key = 65535 - min(degree, 65535), value = the row; the stable
// counting sort of transpose.hip orders them, and rank r goes to slot (r % 8) * prange + r / 8 — the ranks dealt to the 8
// partitions.  (One atomic per row on a histogram of degrees, then one on its cursor, was what this used to be: the two or
// three buckets of the small degrees take millions of same-address atomics at ~5.6 ns each — 60 ms of the 63 ms a new
// snapshot of RMAT-22 cost before its first batch.)
__global__ void xp_deg_key_kernel(const u32* __restrict__ rowptr, u32 n, u32* __restrict__ key, u32* __restrict__ val) {
    for (u32 u = blockIdx.x * 256 + threadIdx.x; u < n; u += gridDim.x * 256) {
        const u32 d = rowptr[u + 1] - rowptr[u];
        key[u] = 65535u - (d < 65535u ? d : 65535u);
        val[u] = u;
    }
}
__global__ void xp_rank_kernel(const u32* __restrict__ by_rank, u32 n, u32 prange, u32* __restrict__ perm) {
    for (u32 r = blockIdx.x * 256 + threadIdx.x; r < n; r += gridDim.x * 256) perm[by_rank[r]] = (r & 7u) * prange + (r >> 3);
}

// the chunk table of the cut on whole double trips.  hp = pstart[9] | cbase[9] | ..: fills cbase and the plan's three arrays and
// sets *done — or leaves everything alone and *done false when a cell touches more runs than the tile has rows
static fgpu_info xp_cut_cells(fgpu_ctx* ctx, BpXPlan* xp, u32 (&hp)[27], bool* done) {
    *done = false;
    hipStream_t st = ctx->stream();
    XpCells pc;
    pc.cb[0] = pc.sb[0] = 0;
    for (int k = 0; k <= 8; ++k) pc.ps[k] = hp[k];
    for (int k = 0; k < 8; ++k) {
        const u32 len = hp[k + 1] - hp[k];
        pc.cb[k + 1] = pc.cb[k] + cdiv(len, XP_CELL);
        pc.sb[k + 1] = pc.sb[k] + cdiv(len, XP_CELL * XP_SUPER);
    }
    const u32 ncells = pc.cb[8], nsuper = pc.sb[8];
    DevBuf<u32> g, nch, worst, info;
    DevBuf<uint8_t> first;
    FGPU_TRY(g.alloc(ctx, (size_t)ncells + 1));
    FGPU_TRY(first.alloc(ctx, (size_t)ncells + 1));
    FGPU_TRY(nch.alloc(ctx, (size_t)nsuper + 1));
    FGPU_TRY(worst.alloc(ctx, 1));
    FGPU_TRY(info.alloc(ctx, 10));
    FGPU_HIP(hipMemsetAsync(worst.p, 0, sizeof(u32), st));
    u32 grid = cdiv((u64)ncells + 1, 4);
    if (grid > (u32)ctx->cus * 16) grid = ctx->cus * 16;
    FGPU_TRY(launch(xp_cell_flags_kernel, dim3(grid), dim3(256), 0, st, (const u32*)xp->pcol.p, pc, g.p, first.p));
    FGPU_TRY(scan_u32(ctx, g.p, g.p, (u64)ncells + 1, nullptr));
    grid = cdiv((u64)nsuper + 1, 256);
    FGPU_TRY(launch(xp_super_count_kernel, dim3(grid), dim3(256), 0, st, (const u32*)g.p, (const uint8_t*)first.p, pc, nch.p, worst.p));
    FGPU_TRY(scan_u32(ctx, nch.p, nch.p, (u64)nsuper + 1, nullptr));
    // one read-back: the first chunk of every partition (the scan at its first super-cell) and the worst cell
    u32 got[10];
    FGPU_TRY(launch(xp_cut_info_kernel, dim3(1), dim3(64), 0, st, (const u32*)nch.p, pc, (const u32*)worst.p, info.p));
    FGPU_TRY(read_words(ctx, info.p, 10, got));
    if (got[9] > XP_RUNS) return FGPU_OK;
    for (int k = 0; k <= 8; ++k) hp[9 + k] = got[k];
    xp->nchunks = hp[17];
    FGPU_TRY(xp->cstart.alloc(ctx, ((size_t)xp->nchunks + 1)));   // (+ 1 as under the key cut: never an empty allocation)
    FGPU_TRY(xp->crun0.alloc(ctx, ((size_t)xp->nchunks + 1)));
    FGPU_TRY(xp->cshared.alloc(ctx, (size_t)xp->nchunks + 8));   // (the stream kernel reads the byte after a partition's last chunk)
    FGPU_HIP(hipMemsetAsync(xp->cshared.p, 0, (size_t)xp->nchunks + 8, st));
    FGPU_TRY(launch(xp_super_fill_kernel, dim3(grid), dim3(256), 0, st, (const u32*)g.p, (const uint8_t*)first.p, pc, (const u32*)nch.p,
                    xp->cstart.p, xp->crun0.p, xp->cshared.p));
    *done = true;                                            // (the build synchronises the stream before it hands the plan out)
    return FGPU_OK;
}

// what the builder reads of A': the cached transpose, or a temporary copy of it with some rows emptied
struct XpSource {
    const u32 *rowptr, *colidx;
    u64 nrows, ncols, nnz;
};
// builds the plan of `t` (= m') under one (direct, dense, cut) triple; the caller holds m->idx_mu.  *out is set when the plan is
// complete on the device; an error frees whatever was built so far.  `layout` (nullable): the plan whose layout of X this one
// gathers from too — its perm is used as it is and the new plan keeps none
static fgpu_info bp_xplan_build(fgpu_ctx* ctx, const fgpu_mat* m, const XpSource* t, int direct, int dense, int cut, const BpXPlan* layout,
                                BpXPlanPtr* out) {
    BpXPlanPtr xp(new (std::nothrow) BpXPlan());
    FGPU_REQUIRE(xp, FGPU_OOM, "out of host memory");
    const u32 n = (u32)t->nrows;
    u32 ng = (n + 63) / 64, nslots = n;
    xp->n = n; xp->nentries = t->nnz; xp->direct = direct; xp->dense = dense;
    hipStream_t st = ctx->stream();
    if (dense) {   // the rows with an entry, ranked in vertex order: slot = rank, groups of 64 slots
        DevBuf<u32> rank;
        FGPU_TRY(rank.alloc(ctx, (size_t)n + 1));
        FGPU_TRY(launch(xp_has_entry_kernel, dim3(ctx->cus * 8), dim3(256), 0, st, (const u32*)t->rowptr, n, rank.p));
        FGPU_TRY(scan_u32(ctx, rank.p, rank.p, (u64)n + 1, nullptr));
        FGPU_TRY(read_u32(ctx, rank.p + n, &xp->nd));
        FGPU_REQUIRE(xp->nd >= 1 && xp->nd <= n, FGPU_INVALID, "partitioned pull: %u of %u rows have an entry", xp->nd, n);
        nslots = xp->nd;
        ng = (nslots + 63) / 64;
        FGPU_TRY(xp->gvtx.alloc(ctx, (size_t)ng * 64));
        FGPU_HIP(hipMemsetAsync(xp->gvtx.p, 0xFF, (size_t)ng * 64 * sizeof(u32), st));    // XP_NO_VTX
        FGPU_TRY(launch(xp_slots_kernel, dim3(ctx->cus * 8), dim3(256), 0, st, (const u32*)rank.p, n, xp->gvtx.p));
    }
    xp->ng = ng;
    const u64 total = 8ull * n;
    DevBuf<u32> off, ridx;
    FGPU_TRY(off.alloc(ctx, total + 1));
    FGPU_TRY(ridx.alloc(ctx, total + 1));
    const u32 prange = (u32)((((t->ncols + 7) / 8) + 15) & ~15ull);
    const u32* perm = layout ? layout->perm.p : nullptr;
    if (!layout && ctx->opt.expand_xcd_relabel && !m->is_hyper() && m->nrows == t->ncols && t->ncols % 128 == 0 && (u64)prange * 8 == t->ncols) {
        // rank the rows of X by out-degree (descending, ties by id) and deal the ranks to the partitions
        const u32 nu = (u32)t->ncols;
        DevBuf<u32> dkey, dval, by_rank, kptr;
        FGPU_TRY(dkey.alloc(ctx, nu));
        FGPU_TRY(dval.alloc(ctx, nu));
        FGPU_TRY(by_rank.alloc(ctx, nu));
        FGPU_TRY(kptr.alloc(ctx, 65536 + 1));
        FGPU_TRY(xp->perm.alloc(ctx, (size_t)nu));
        FGPU_TRY(launch(xp_deg_key_kernel, dim3(ctx->cus * 8), dim3(256), 0, st, (const u32*)m->rowptr, nu, dkey.p, dval.p));
        FGPU_TRY(sort_u32_pairs_by_key(ctx, dkey.p, dval.p, nu, 65536, by_rank.p, kptr.p));
        FGPU_TRY(launch(xp_rank_kernel, dim3(ctx->cus * 8), dim3(256), 0, st, (const u32*)by_rank.p, nu, prange, xp->perm.p));
        perm = xp->perm.p;
    }
    FGPU_TRY(xp->pstart_dev.alloc(ctx, 27));
    FGPU_TRY(xp->pcol.alloc(ctx, ((size_t)t->nnz + 64)));
    {
        DevBuf<uint2> pairs;
        FGPU_TRY(pairs.alloc(ctx, t->nnz));
        FGPU_TRY(partition_csr_entries(ctx, t->colidx, t->rowptr, n, t->nnz, perm, prange, 8, pairs.p, xp->pstart_dev.p));
        u32 rgrid = cdiv(t->nnz, 256 * 4);
        if (rgrid > (u32)ctx->cus * 16) rgrid = ctx->cus * 16;
        FGPU_TRY(launch(xp_runs_kernel, dim3(rgrid), dim3(256), 0, st, (const uint2*)pairs.p, (const u32*)xp->pstart_dev.p, n, (u32)t->nnz,
                        xp->pcol.p, off.p));
        FGPU_TRY(launch(xp_run_tails_kernel, dim3(64, 8), dim3(256), 0, st, (const uint2*)pairs.p, (const u32*)xp->pstart_dev.p, n, off.p));
    }
    if (direct) {   // the single-entry runs leave the stream; everything below is built over the runs that stay
        const u32 nnz = (u32)t->nnz;
        DevBuf<u32> pos;
        FGPU_TRY(pos.alloc(ctx, (size_t)nnz + 1));
        u32 egrid = cdiv((u64)nnz + 1, 256 * 4);
        if (egrid > (u32)ctx->cus * 16) egrid = ctx->cus * 16;
        FGPU_TRY(launch(xp_keep_kernel, dim3(egrid), dim3(256), 0, st, (const u32*)xp->pcol.p, nnz, pos.p));
        FGPU_TRY(scan_u32(ctx, pos.p, pos.p, (u64)nnz + 1, nullptr));
        u32 nkept = 0;
        FGPU_TRY(read_u32(ctx, pos.p + nnz, &nkept));
        xp->ndirect = nnz - nkept;
        DevBuf<u32> kept;
        FGPU_TRY(kept.alloc(ctx, (size_t)nkept + 64));
        FGPU_TRY(xp->dcol.alloc(ctx, ((size_t)xp->ndirect + 1)));
        FGPU_HIP(hipMemsetAsync(xp->dcol.p, 0, sizeof(u32), st));   // (index 0 is what the fold loads for a row without one)
        FGPU_TRY(launch(xp_split_kernel, dim3(egrid), dim3(256), 0, st, (const u32*)xp->pcol.p, (const u32*)pos.p, nnz, kept.p, xp->dcol.p));
        xp->pcol = std::move(kept);   // (the full stream goes now)
        FGPU_TRY(xp->de.alloc(ctx, (size_t)8 * ng));
        FGPU_TRY(xp->dbase.alloc(ctx, ((size_t)8 * ng + 1)));
        u32 ggrid = cdiv((u64)8 * ng, 4);
        if (ggrid > (u32)ctx->cus * 16) ggrid = ctx->cus * 16;
        FGPU_TRY(launch(xp_direct_groups_kernel, dim3(ggrid), dim3(256), 0, st, (const u32*)off.p, (const u32*)pos.p, n, ng,
                        (const u32*)xp->gvtx.p, nslots, xp->de.p, xp->dbase.p));
        FGPU_TRY(launch(xp_remap_kernel, dim3(ctx->cus * 16), dim3(256), 0, st, off.p, total, (const u32*)pos.p, xp->pstart_dev.p));
    }
    FGPU_TRY(launch(xp_nonempty_kernel, dim3(ctx->cus * 16), dim3(256), 0, st, (const u32*)off.p, total, ridx.p));
    FGPU_TRY(scan_u32(ctx, ridx.p, ridx.p, total + 1, nullptr));
    FGPU_TRY(read_u32(ctx, ridx.p + total, &xp->nprows));
    u32 hp[27];                                              // pstart[9] | cbase[9] | first run of partition k [9]
    FGPU_TRY(read_words(ctx, xp->pstart_dev.p, 9, hp));
    for (int k = 0; k <= 8; ++k) FGPU_TRY(read_u32(ctx, ridx.p + (size_t)k * n, &hp[18 + k]));
    bool cells = false;
    if (cut) FGPU_TRY(xp_cut_cells(ctx, xp.get(), hp, &cells));
    xp->cut = cells ? 1 : 0;
    if (!cells) {
        hp[9] = 0;
        for (int k = 0; k < 8; ++k) {
            const u64 len = hp[k + 1] - hp[k], runs = hp[19 + k] - hp[18 + k];
            hp[10 + k] = hp[9 + k] + (len ? (u32)((len - 1 + (u64)XP_RUNW * (runs - 1)) / XP_SPAN) + 1u : 0u);
        }
    }
    for (int k = 0; k <= 8; ++k) { xp->pstart[k] = hp[k]; xp->cbase[k] = hp[9 + k]; }
    xp->nchunks = xp->cbase[8];
    FGPU_TRY(ctx->h2d(xp->pstart_dev.p, hp, 27 * sizeof(u32)));
    FGPU_TRY(xp->ne.alloc(ctx, (size_t)8 * ng));
    FGPU_TRY(xp->pbase.alloc(ctx, ((size_t)8 * ng + 1)));
    u32 ggrid = cdiv((u64)8 * ng, 4);
    if (ggrid > (u32)ctx->cus * 16) ggrid = ctx->cus * 16;
    FGPU_TRY(launch(xp_groups_kernel, dim3(ggrid), dim3(256), 0, st, (const u32*)off.p, (const u32*)ridx.p, n, ng,
                    (const u32*)xp->gvtx.p, nslots, xp->ne.p, xp->pbase.p));
    if (!cells) {
        FGPU_TRY(xp->cstart.alloc(ctx, ((size_t)xp->nchunks + 1)));
        FGPU_TRY(xp->crun0.alloc(ctx, ((size_t)xp->nchunks + 1)));
        FGPU_TRY(xp->cshared.alloc(ctx, (size_t)xp->nchunks + 8));
        FGPU_HIP(hipMemsetAsync(xp->cshared.p, 0, (size_t)xp->nchunks + 8, st));
        FGPU_TRY(launch(xp_chunks_kernel, dim3(ctx->cus * 16), dim3(256), 0, st, (const u32*)off.p, (const u32*)ridx.p, n,
                        (const u32*)xp->pstart_dev.p, xp->cstart.p, xp->crun0.p, xp->cshared.p));
    }
    {   // the shared rows, compacted once (a few thousand among ~10^5 chunks)
        DevBuf<u32> zc;
        FGPU_TRY(zc.alloc(ctx, 1));
        FGPU_HIP(hipMemsetAsync(zc.p, 0, sizeof(u32), st));
        FGPU_TRY(xp->zrows.alloc(ctx, ((size_t)xp->nchunks + 1)));
        FGPU_TRY(launch(xp_shared_rows_kernel, dim3(cdiv(xp->nchunks ? xp->nchunks : 1, 256)), dim3(256), 0, st, (const u32*)xp->crun0.p,
                        (const uint8_t*)xp->cshared.p, xp->nchunks, xp->zrows.p, zc.p));
        FGPU_TRY(read_u32(ctx, zc.p, &xp->nzrows));
        // ... and the spare row after the last run: the all-zero partial row the fold reads for (row, partition) pairs without one
        FGPU_TRY(ctx->h2d(xp->zrows.p + xp->nzrows, &xp->nprows, sizeof(u32)));
        xp->nzrows += 1;
    }
    FGPU_HIP(hipStreamSynchronize(st));
    xp->usable = true;
    *out = std::move(xp);
    return FGPU_OK;
}

// ---- the top hub's out-rows (once per plan) -----------------------------------------------------------------------------------
// At RMAT-22 the vertex of largest out-degree h has 97 939 out-neighbours, and those rows of A' — 4.9 % of the rows with
// entries — hold 56 % of the entries: every one of them gathers row h of X among its in-neighbours' rows.  When that row is
// all ones (every source of the pass reaches h in the hops before) their result is known before the hop starts, and the hop
// runs under a second plan from which they are gone (bitexpand.hip bp_hop_count decides, on the device's own state).
// The threshold is a design constant: the second plan costs (1 - share) of a plan's memory, and below a quarter of the entries it
// buys little.
constexpr u32 XP_HUB_MIN_SHARE_DEN = 4;   // out(h) must hold at least 1 / 4 of the entries of A'
// best = max over the rows of (entries << 32 | ~row): the most entries, the smallest id on a tie.  (Not by_rank[0] of the
// relabel sort: its key stops at 65 535 entries, above which rows tie by id alone.)
__global__ __launch_bounds__(256) void xp_hub_pick_kernel(const u32* __restrict__ rowptr, u32 nrows, unsigned long long* __restrict__ best) {
    u64 k = 0;
    for (u32 u = blockIdx.x * 256 + threadIdx.x; u < nrows; u += gridDim.x * 256) {
        const u64 key = ((u64)(rowptr[u + 1] - rowptr[u]) << 32) | (u64)(~u);
        k = key > k ? key : k;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const u64 o = (u64)__shfl_xor((long long)k, d, 64);
        k = o > k ? o : k;
    }
    if (lane_id() == 0 && k) atomicMax(best, (unsigned long long)k);
}
// out(h) = row h of m: the list, a flag per row of A' (drop[v] = 1), and sums[0] = entries of those rows, sums[1] = the sum of
// their destination hashes
__global__ __launch_bounds__(256) void xp_hub_rows_kernel(const u32* __restrict__ mrowptr, const u32* __restrict__ mcol, u32 h, u32 n,
                                                          const u32* __restrict__ trowptr, u32* __restrict__ list, u32* __restrict__ drop,
                                                          unsigned long long* __restrict__ sums) {
    const u32 b = mrowptr[h], deg = mrowptr[h + 1] - b;
    u64 ent = 0, ds = 0;
    for (u32 i = blockIdx.x * 256 + threadIdx.x; i < deg; i += gridDim.x * 256) {
        const u32 v = mcol[b + i];
        list[i] = v;
        if (v < n) {                                          // (a column of m is a row of A')
            drop[v] = 1u;
            ent += trowptr[v + 1] - trowptr[v];
        }
        ds += cs_dest_hash(v);
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        ent += (u64)__shfl_xor((long long)ent, d, 64);
        ds += (u64)__shfl_xor((long long)ds, d, 64);
    }
    if (lane_id() == 0) {
        if (ent) atomicAdd(sums, (unsigned long long)ent);
        atomicAdd(sums + 1, (unsigned long long)ds);
    }
}
// kd[v] = entries row v keeps (kd[n] = 0: the scan leaves the total there)
__global__ void xp_hub_kept_kernel(const u32* __restrict__ trowptr, const u32* __restrict__ drop, u32 n, u32* __restrict__ kd) {
    for (u32 v = blockIdx.x * 256 + threadIdx.x; v <= n; v += gridDim.x * 256) kd[v] = v < n && !drop[v] ? trowptr[v + 1] - trowptr[v] : 0u;
}
// the kept rows' column ids, compacted: a wavefront per row
__global__ __launch_bounds__(256) void xp_hub_compact_kernel(const u32* __restrict__ trowptr, const u32* __restrict__ tcol,
                                                             const u32* __restrict__ rp, u32 n, u32* __restrict__ col) {
    const u32 lane = lane_id();
    const u32 wave = (blockIdx.x * 256 + threadIdx.x) >> 6, nwaves = (gridDim.x * 256) >> 6;
    for (u32 v = wave; v < n; v += nwaves) {
        const u32 o = rp[v], k = rp[v + 1] - o, b = trowptr[v];
        for (u32 i = lane; i < k; i += 64) col[o + i] = tcol[b + i];
    }
}
// bit u of `bits`: u is an in-neighbour of h (row h of A')
__global__ void xp_hub_in_kernel(const u32* __restrict__ trowptr, const u32* __restrict__ tcol, u32 h, u64* __restrict__ bits) {
    const u32 b = trowptr[h], e = trowptr[h + 1];
    for (u32 q = b + blockIdx.x * 256 + threadIdx.x; q < e; q += gridDim.x * 256)
        atomicOr((unsigned long long*)&bits[tcol[q] >> 6], 1ull << (tcol[q] & 63u));
}

// names the hub of the finished full plan `xp` and, when its out-rows hold their share of A', builds the reduced plan beside it
static fgpu_info bp_xplan_hub_build(fgpu_ctx* ctx, const fgpu_mat* m, const fgpu_mat* t, int direct, int dense, int cut, BpXPlan* xp) {
    if (m->is_hyper() || m->nrows >= 0xFFFFFFFFull || m->ncols != t->nrows || m->nrows != t->ncols) return FGPU_OK;
    hipStream_t st = ctx->stream();
    const u32 n = (u32)t->nrows, nu = (u32)m->nrows;
    DevBuf<u64> sums;                                        // [0] the pick, [1] entries of out(h), [2] their hash sum
    FGPU_TRY(sums.alloc(ctx, 3));
    FGPU_HIP(hipMemsetAsync(sums.p, 0, 3 * sizeof(u64), st));
    u32 grid = cdiv(nu, 256);
    if (grid > (u32)ctx->cus * 8) grid = ctx->cus * 8;
    FGPU_TRY(launch(xp_hub_pick_kernel, dim3(grid), dim3(256), 0, st, (const u32*)m->rowptr, nu, (unsigned long long*)sums.p));
    u64 best = 0;
    FGPU_TRY(read_u64(ctx, sums.p, &best));
    const u32 deg = (u32)(best >> 32), h = ~(u32)best;
    if (!deg || h >= nu) return FGPU_OK;
    DevBuf<u32> list, drop, kd, rp, col;
    FGPU_TRY(list.alloc(ctx, deg));
    FGPU_TRY(drop.alloc(ctx, (size_t)n + 1));
    FGPU_HIP(hipMemsetAsync(drop.p, 0, ((size_t)n + 1) * sizeof(u32), st));
    grid = cdiv(deg, 256);
    if (grid > (u32)ctx->cus * 4) grid = ctx->cus * 4;
    FGPU_TRY(launch(xp_hub_rows_kernel, dim3(grid), dim3(256), 0, st, (const u32*)m->rowptr, (const u32*)m->colidx, h, n,
                    (const u32*)t->rowptr, list.p, drop.p, (unsigned long long*)(sums.p + 1)));
    u32 got[4];
    FGPU_TRY(read_words(ctx, (const u32*)(sums.p + 1), 4, got));
    const u64 gone = (u64)got[0] | ((u64)got[1] << 32);
    if (gone * XP_HUB_MIN_SHARE_DEN < t->nnz || gone >= t->nnz) return FGPU_OK;   // (too small a share, or nothing would be left)
    // t': the rows out(h) emptied — row pointers from a scan of the kept degrees, column ids compacted
    FGPU_TRY(kd.alloc(ctx, (size_t)n + 1));
    FGPU_TRY(rp.alloc(ctx, (size_t)n + 1));
    FGPU_TRY(launch(xp_hub_kept_kernel, dim3(ctx->cus * 8), dim3(256), 0, st, (const u32*)t->rowptr, (const u32*)drop.p, n, kd.p));
    FGPU_TRY(scan_u32(ctx, kd.p, rp.p, (u64)n + 1, nullptr));
    u32 kept = 0;                                            // (t' is sized by what the scan says, whatever the sum above said)
    FGPU_TRY(read_u32(ctx, rp.p + n, &kept));
    FGPU_REQUIRE(kept >= 1 && (u64)kept + gone == t->nnz, FGPU_INVALID, "partitioned pull: the hub's rows hold %llu of %llu entries, %u stay",
                 (unsigned long long)gone, (unsigned long long)t->nnz, kept);
    FGPU_TRY(col.alloc(ctx, kept));
    FGPU_TRY(launch(xp_hub_compact_kernel, dim3(ctx->cus * 16), dim3(256), 0, st, (const u32*)t->rowptr, (const u32*)t->colidx,
                    (const u32*)rp.p, n, col.p));
    const XpSource src = {rp.p, col.p, t->nrows, t->ncols, kept};
    BpXPlanPtr reduced;
    FGPU_TRY(bp_xplan_build(ctx, m, &src, direct, dense, cut, xp, &reduced));   // (synchronised: t' may go)
    const size_t nwords = ((size_t)t->ncols + 63) / 64;
    FGPU_TRY(xp->hub_in.alloc(ctx, nwords + 1));
    FGPU_HIP(hipMemsetAsync(xp->hub_in.p, 0, (nwords + 1) * sizeof(u64), st));
    if (h < n) FGPU_TRY(launch(xp_hub_in_kernel, dim3(64), dim3(256), 0, st, (const u32*)t->rowptr, (const u32*)t->colidx, h, xp->hub_in.p));
    u32 slot = h;
    if (xp->perm.p) FGPU_TRY(read_u32(ctx, xp->perm.p + h, &slot));
    FGPU_HIP(hipStreamSynchronize(st));
    xp->hub_v = h; xp->hub_slot = slot; xp->hub_deg = deg;
    xp->hub_dsum = (u64)got[2] | ((u64)got[3] << 32);
    xp->hub_gone = gone;
    xp->hub_rows = std::move(list);
    reduced->full = xp;
    xp->hub = std::move(reduced);
    return FGPU_OK;
}

// ---- the hub set: the tier of hubs under the top one (once per plan, after the first reduced plan) -------------------------------
// R-MAT has one top hub and then a tier of `scale` hubs of about 0.39 of its degree (at RMAT-22: hubs 2 .. 23, 38 K entries each,
// before a third tier at 14 K).  With the rows of the union of their out-rows gone as well a plan holds 16 % of the entries of A'
// instead of 44 %, and 55 % of the live sources of a label scan reach ALL 23 in exactly two hops.  The plans nest: a pass runs
// under the deepest one whose hubs its state saturates (bitexpand.hip bp_hub_rows).  The quarter separates the second tier from
// the third; the eighth is what the extra rows must hold for a third plan's memory to pay.
constexpr u32 XP_HUB_SET_DEG_DEN = 4;         // H: the rows of m with at least 1 / 4 of the top hub's entries ...
constexpr u32 XP_HUB_SET_MAX = 32;            // ... the 32 largest of them (a bit each of hub_mask's words)
constexpr u32 XP_HUB_SET_MIN_SHARE_DEN = 8;   // the union's rows outside out(h) must hold at least 1 / 8 of the entries of A'
constexpr u32 XP_HUB_SET_LIST = 1024;         // first bound of the list of qualifying rows (listed again at its true length beyond)
static_assert(XP_HUB_SET_MAX == 32, "hub_mask is a u32 per vertex, BpXPlan::hset_v holds 32");
// every row of m with at least `mindeg` entries as (entries << 32 | ~row), in no order, up to `cap`; *cnt = how many there are
__global__ __launch_bounds__(256) void xp_hub_set_list_kernel(const u32* __restrict__ rowptr, u32 nrows, u32 mindeg, u32 cap,
                                                              u64* __restrict__ keys, u32* __restrict__ cnt) {
    for (u32 u = blockIdx.x * 256 + threadIdx.x; u < nrows; u += gridDim.x * 256) {
        const u32 d = rowptr[u + 1] - rowptr[u];
        if (d >= mindeg) {
            const u32 i = atomicAdd(cnt, 1u);
            if (i < cap) keys[i] = ((u64)d << 32) | (u64)(~u);
        }
    }
}
// drop[v] = 1 for every v of out(hs[blockIdx.y]) (hubs share out-neighbours: the same value from whoever stores it)
__global__ __launch_bounds__(256) void xp_hub_set_rows_kernel(const u32* __restrict__ mrowptr, const u32* __restrict__ mcol,
                                                              const u32* __restrict__ hs, u32 n, u32* __restrict__ drop) {
    const u32 h = hs[blockIdx.y];
    const u32 b = mrowptr[h], deg = mrowptr[h + 1] - b;
    for (u32 i = blockIdx.x * 256 + threadIdx.x; i < deg; i += gridDim.x * 256) {
        const u32 v = mcol[b + i];
        if (v < n) drop[v] = 1u;
    }
}
// over the flagged rows, each once: sums[0] = their entries in A', sums[1] = the sum of their destination hashes
__global__ __launch_bounds__(256) void xp_hub_set_sums_kernel(const u32* __restrict__ trowptr, const u32* __restrict__ drop, u32 n,
                                                              unsigned long long* __restrict__ sums) {
    u64 ent = 0, ds = 0;
    for (u32 v = blockIdx.x * 256 + threadIdx.x; v < n; v += gridDim.x * 256)
        if (drop[v]) {
            ent += trowptr[v + 1] - trowptr[v];
            ds += cs_dest_hash(v);
        }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        ent += (u64)__shfl_xor((long long)ent, d, 64);
        ds += (u64)__shfl_xor((long long)ds, d, 64);
    }
    if (lane_id() == 0) {
        if (ent) atomicAdd(sums, (unsigned long long)ent);
        if (ds) atomicAdd(sums + 1, (unsigned long long)ds);
    }
}
// the flagged rows, ascending: pos = the exclusive scan of the flags
__global__ void xp_hub_set_compact_kernel(const u32* __restrict__ drop, const u32* __restrict__ pos, u32 n, u32* __restrict__ list) {
    for (u32 v = blockIdx.x * 256 + threadIdx.x; v < n; v += gridDim.x * 256)
        if (drop[v]) list[pos[v]] = v;
}
// mask[u] |= 1 << i for every in-neighbour u of hs[i] (row hs[i] of A'), i = blockIdx.y
__global__ __launch_bounds__(256) void xp_hub_set_mask_kernel(const u32* __restrict__ trowptr, const u32* __restrict__ tcol,
                                                              const u32* __restrict__ hs, u32 n, u32 ncols, u32* __restrict__ mask) {
    const u32 h = hs[blockIdx.y];
    if (h >= n) return;
    const u32 b = trowptr[h], e = trowptr[h + 1];
    for (u32 q = b + blockIdx.x * 256 + threadIdx.x; q < e; q += gridDim.x * 256) {
        const u32 u = tcol[q];
        if (u < ncols) atomicOr(&mask[u], 1u << blockIdx.y);
    }
}
__global__ void xp_hub_set_slots_kernel(const u32* __restrict__ hs, const u32* __restrict__ perm, u32 nh, u32* __restrict__ slots) {
    if (threadIdx.x < nh) slots[threadIdx.x] = perm ? perm[hs[threadIdx.x]] : hs[threadIdx.x];
}

// names the hub set of a plan that has its first reduced plan and, when the union's extra rows hold their share, builds the
// second one beside it
static fgpu_info bp_xplan_hub_set_build(fgpu_ctx* ctx, const fgpu_mat* m, const fgpu_mat* t, int direct, int dense, int cut, BpXPlan* xp) {
    if (!xp->hub || !xp->hub->usable || !xp->hub_deg) return FGPU_OK;
    hipStream_t st = ctx->stream();
    const u32 n = (u32)t->nrows, nu = (u32)m->nrows;
    const u32 mindeg = cdiv(xp->hub_deg, XP_HUB_SET_DEG_DEN);
    DevBuf<u64> keys;
    DevBuf<u32> cnt;
    FGPU_TRY(cnt.alloc(ctx, 1));
    u32 grid = cdiv(nu, 256);
    if (grid > (u32)ctx->cus * 8) grid = ctx->cus * 8;
    u32 cap = XP_HUB_SET_LIST, found = 0;
    for (int round = 0; round < 2; ++round) {                // (which rows a full list holds is up to the atomics: list them all)
        FGPU_TRY(keys.alloc(ctx, cap));
        FGPU_HIP(hipMemsetAsync(cnt.p, 0, sizeof(u32), st));
        FGPU_TRY(launch(xp_hub_set_list_kernel, dim3(grid), dim3(256), 0, st, (const u32*)m->rowptr, nu, mindeg, cap, keys.p, cnt.p));
        FGPU_TRY(read_u32(ctx, cnt.p, &found));
        if (found <= cap) break;
        cap = found;
    }
    if (found < 2 || found > cap) return FGPU_OK;
    std::vector<u64> hk(found);
    FGPU_TRY(ctx->d2h(hk.data(), keys.p, (size_t)found * sizeof(u64)));
    std::sort(hk.begin(), hk.end(), [](u64 a, u64 b) { return a > b; });   // entries descending, ids ascending
    const u32 nh = found < XP_HUB_SET_MAX ? found : XP_HUB_SET_MAX;
    u32 hv[XP_HUB_SET_MAX] = {};
    for (u32 i = 0; i < nh; ++i) hv[i] = ~(u32)hk[i];
    if (hv[0] != xp->hub_v) return FGPU_OK;
    DevBuf<u32> hs, drop, pos, list, kd, rp, col, slots, mask;
    DevBuf<u64> sums;
    FGPU_TRY(hs.alloc(ctx, XP_HUB_SET_MAX));
    FGPU_TRY(ctx->h2d(hs.p, hv, sizeof(hv)));
    FGPU_TRY(drop.alloc(ctx, (size_t)n + 1));
    FGPU_HIP(hipMemsetAsync(drop.p, 0, ((size_t)n + 1) * sizeof(u32), st));
    FGPU_TRY(sums.alloc(ctx, 2));
    FGPU_HIP(hipMemsetAsync(sums.p, 0, 2 * sizeof(u64), st));
    grid = cdiv(xp->hub_deg, 256);                           // (no row of m is longer than the top hub's)
    if (grid > (u32)ctx->cus * 4) grid = ctx->cus * 4;
    FGPU_TRY(launch(xp_hub_set_rows_kernel, dim3(grid, nh), dim3(256), 0, st, (const u32*)m->rowptr, (const u32*)m->colidx,
                    (const u32*)hs.p, n, drop.p));
    FGPU_TRY(launch(xp_hub_set_sums_kernel, dim3(ctx->cus * 8), dim3(256), 0, st, (const u32*)t->rowptr, (const u32*)drop.p, n,
                    (unsigned long long*)sums.p));
    u32 got[4];
    FGPU_TRY(read_words(ctx, (const u32*)sums.p, 4, got));
    const u64 gone = (u64)got[0] | ((u64)got[1] << 32);
    if (gone < xp->hub_gone || gone >= t->nnz) return FGPU_OK;                    // (nothing would be left)
    if ((gone - xp->hub_gone) * XP_HUB_SET_MIN_SHARE_DEN < t->nnz) return FGPU_OK;  // (too small a share beyond out(h))
    // the union, each row once
    FGPU_TRY(pos.alloc(ctx, (size_t)n + 1));
    FGPU_TRY(scan_u32(ctx, drop.p, pos.p, (u64)n + 1, nullptr));
    u32 nrows_u = 0;
    FGPU_TRY(read_u32(ctx, pos.p + n, &nrows_u));
    FGPU_REQUIRE(nrows_u >= xp->hub_deg && nrows_u <= n, FGPU_INVALID, "partitioned pull: the hub set's union holds %u rows, the top hub's %u",
                 nrows_u, xp->hub_deg);
    FGPU_TRY(list.alloc(ctx, nrows_u));
    FGPU_TRY(launch(xp_hub_set_compact_kernel, dim3(ctx->cus * 8), dim3(256), 0, st, (const u32*)drop.p, (const u32*)pos.p, n, list.p));
    // t'': the union's rows emptied, as bp_xplan_hub_build empties out(h)
    FGPU_TRY(kd.alloc(ctx, (size_t)n + 1));
    FGPU_TRY(rp.alloc(ctx, (size_t)n + 1));
    FGPU_TRY(launch(xp_hub_kept_kernel, dim3(ctx->cus * 8), dim3(256), 0, st, (const u32*)t->rowptr, (const u32*)drop.p, n, kd.p));
    FGPU_TRY(scan_u32(ctx, kd.p, rp.p, (u64)n + 1, nullptr));
    u32 kept = 0;
    FGPU_TRY(read_u32(ctx, rp.p + n, &kept));
    FGPU_REQUIRE(kept >= 1 && (u64)kept + gone == t->nnz, FGPU_INVALID, "partitioned pull: the hub set's rows hold %llu of %llu entries, %u stay",
                 (unsigned long long)gone, (unsigned long long)t->nnz, kept);
    FGPU_TRY(col.alloc(ctx, kept));
    FGPU_TRY(launch(xp_hub_compact_kernel, dim3(ctx->cus * 16), dim3(256), 0, st, (const u32*)t->rowptr, (const u32*)t->colidx,
                    (const u32*)rp.p, n, col.p));
    const XpSource src = {rp.p, col.p, t->nrows, t->ncols, kept};
    BpXPlanPtr reduced;
    FGPU_TRY(bp_xplan_build(ctx, m, &src, direct, dense, cut, xp, &reduced));   // (synchronised: t'' may go)
    FGPU_TRY(mask.alloc(ctx, (size_t)t->ncols + 1));
    FGPU_HIP(hipMemsetAsync(mask.p, 0, ((size_t)t->ncols + 1) * sizeof(u32), st));
    FGPU_TRY(launch(xp_hub_set_mask_kernel, dim3(64, nh), dim3(256), 0, st, (const u32*)t->rowptr, (const u32*)t->colidx,
                    (const u32*)hs.p, n, (u32)t->ncols, mask.p));
    FGPU_TRY(slots.alloc(ctx, XP_HUB_SET_MAX));
    FGPU_TRY(launch(xp_hub_set_slots_kernel, dim3(1), dim3(64), 0, st, (const u32*)hs.p, (const u32*)xp->perm.p, nh, slots.p));
    FGPU_HIP(hipStreamSynchronize(st));
    xp->hset_n = nh;
    memcpy(xp->hset_v, hv, sizeof(hv));
    xp->hset_slots = std::move(slots);
    xp->hset_deg = nrows_u;
    xp->hset_dsum = (u64)got[2] | ((u64)got[3] << 32);
    xp->hset_rows = std::move(list);
    xp->hub_mask = std::move(mask);
    reduced->full = xp;
    xp->hub2 = std::move(reduced);
    return FGPU_OK;
}
bool bp_xplan_hub(const BpXPlan* xp, BpXHub* out) {
    if (!xp || !xp->hub || !xp->hub->usable) return false;
    *out = BpXHub{xp->hub.get(), xp->hub_slot, xp->hub_deg, xp->hub_dsum, xp->hub_rows.p, xp->hub_in.p};
    if (xp->hub2 && xp->hub2->usable) {
        out->set_plan = xp->hub2.get();
        out->set_n = xp->hset_n;
        out->set_slots = xp->hset_slots.p;
        out->set_deg = xp->hset_deg;
        out->set_dsum = xp->hset_dsum;
        out->set_rows = xp->hset_rows.p;
        out->hub_mask = xp->hub_mask.p;
    }
    return true;
}

// The plan is an optional accelerator: when its build fails (its temporaries are large — 64 bytes per vertex and 8 per entry) the
// half-built plan is freed, an empty one is attached as "not usable" (no second attempt per snapshot), the error is dropped
// and the hop falls back to the plain pull.  (idx_mu is held from the look-up to the attachment: no reader
// can tell this from attaching the plan first and finishing it afterwards.)
// A plan is kept per (expand_xp_direct, expand_xp_dense, expand_xp_cut) triple (a plan built under one is never handed to a hop expecting
// another); the fold takes the form of its plan.
fgpu_info bp_xplan(fgpu_ctx* ctx, const fgpu_mat* m, const fgpu_mat* t, const BpXPlan** out) {
    *out = nullptr;
    if (!ctx->opt.expand_xcd || !t || t->is_hyper()) return FGPU_OK;
    if (t->ncols >= (1ull << 31) || t->nrows >= 0xFFFFFFC0ull || t->nnz < 4096 || t->nnz >= 0x7FFFFFFFull) return FGPU_OK;
    const int direct = ctx->opt.expand_xp_direct ? 1 : 0, dense = ctx->opt.expand_xp_dense ? 1 : 0, cut = ctx->opt.expand_xp_cut ? 1 : 0;
    std::lock_guard<std::mutex> idx_guard(m->idx_mu);
    BpXPlanPtr& slot = t->bp_xplan[direct + 2 * dense + 4 * cut];
    if (!slot) {
        BpXPlanPtr xp;
        const XpSource src = {t->rowptr, t->colidx, t->nrows, t->ncols, t->nnz};
        if (bp_xplan_build(ctx, m, &src, direct, dense, cut, nullptr, &xp) != FGPU_OK) {
            xp.reset(new (std::nothrow) BpXPlan());
            FGPU_REQUIRE(xp, FGPU_OOM, "out of host memory");
            (void)hipGetLastError();
            set_error("%s", "");
        } else if (bp_xplan_hub_build(ctx, m, t, direct, dense, cut, xp.get()) != FGPU_OK) {
            // (the reduced plan is an accelerator of the accelerator: the full plan stays usable, and there is no second attempt)
            xp->hub.reset();
            (void)hipStreamSynchronize(ctx->stream());
            (void)hipGetLastError();
            set_error("%s", "");
        } else if (bp_xplan_hub_set_build(ctx, m, t, direct, dense, cut, xp.get()) != FGPU_OK) {
            // (likewise one level down: the full plan and the first reduced plan stay exactly as they are)
            xp->hub2.reset();
            (void)hipStreamSynchronize(ctx->stream());
            (void)hipGetLastError();
            set_error("%s", "");
        }
        slot = std::move(xp);
    }
    if (slot->usable) *out = slot.get();
    return FGPU_OK;
}

// the chunk table read back (fgpu_mat_xp_chunks): [chunks, cut the plan holds, pstart[9], cbase[9]], then cstart, crun0 and cshared
// (a word each) of every chunk
fgpu_info bp_xplan_chunks(fgpu_ctx* ctx, const BpXPlan* xp, uint32_t** out, uint64_t* nwords) {
    const size_t nc = xp->nchunks, total = 20 + 3 * nc;
    uint32_t* w = (uint32_t*)ctx->result_alloc(total * sizeof(uint32_t));
    FGPU_REQUIRE(w, FGPU_OOM, "out of host memory");
    w[0] = xp->nchunks; w[1] = (u32)xp->cut;
    for (int k = 0; k <= 8; ++k) { w[2 + k] = xp->pstart[k]; w[11 + k] = xp->cbase[k]; }
    uint32_t* sh = w + 20 + 2 * nc;
    fgpu_info i = nc ? ctx->d2h(w + 20, xp->cstart.p, nc * sizeof(u32)) : FGPU_OK;
    if (i == FGPU_OK && nc) i = ctx->d2h(w + 20 + nc, xp->crun0.p, nc * sizeof(u32));
    if (i == FGPU_OK && nc) i = ctx->d2h(sh, xp->cshared.p, nc);      // the bytes, packed at the head of their words' space ...
    if (i != FGPU_OK) { ctx->host_free(w); return i; }
    for (size_t c = nc; c-- > 0;) sh[c] = reinterpret_cast<const uint8_t*>(sh)[c];   // ... widened from the last one down
    *out = w; *nwords = total;
    return FGPU_OK;
}

// ---- per hop ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint4 or4(uint4 a, uint4 b) { return make_uint4(a.x | b.x, a.y | b.y, a.z | b.z, a.w | b.w); }
__device__ __forceinline__ bool any4(uint4 a) { return (a.x | a.y | a.z | a.w) != 0u; }
__device__ __forceinline__ void atomic_or4(uint4* dst, uint4 v) {
    unsigned long long* d = reinterpret_cast<unsigned long long*>(dst);
    if (v.x | v.y) atomicOr(d, ((unsigned long long)v.y << 32) | v.x);
    if (v.z | v.w) atomicOr(d + 1, ((unsigned long long)v.w << 32) | v.z);
}

// streaming hints (option expand_nt; A/B): a partial row is written once and read once by the fold, an entry of the column-id stream is
// read once per hop — neither should displace the partition's hot rows of X from its XCD's L2
typedef unsigned int xp_u32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ uint4 xp_load_nt(const uint4* p) {
    const xp_u32x4 v = __builtin_nontemporal_load(reinterpret_cast<const xp_u32x4*>(p));
    return make_uint4(v.x, v.y, v.z, v.w);
}
__device__ __forceinline__ void xp_store_nt(uint4* p, uint4 v) {
    xp_u32x4 t;
    t.x = v.x; t.y = v.y; t.z = v.z; t.w = v.w;
    __builtin_nontemporal_store(t, reinterpret_cast<xp_u32x4*>(p));
}

// partial rows that receive pieces from several chunks start from zero
__global__ __launch_bounds__(256) void xp_zero_rows_kernel(const u32* __restrict__ rows, u32 nrows, u32 ql, uint4* __restrict__ partial) {
    const u32 per = 256 / ql;
    for (u32 i = blockIdx.x * per + threadIdx.x / ql; i < nrows; i += gridDim.x * per)
        partial[(size_t)rows[i] * ql + threadIdx.x % ql] = make_uint4(0, 0, 0, 0);
}

// the stream pull: QL lanes of 16 bytes per row of X (ws = 2 QL words), 64 / QL slots per wavefront, QL consecutive entries
// per slot and trip.  WIDE = false: the state is at most 4 GiB, a row's byte offset fits 32 bits (one multiply-add per gather
// address instead of 64-bit arithmetic: the kernel issues ~100 instructions per 64 entries and is not far from VALU-bound).
// LA (expand_xp_lookahead): the loads that run ahead of the trip being consumed do not stop at the chunk's end.  A wavefront takes
// chunks j, j + nwaves, ... of its partition and knows on entering chunk j where chunk j + nwaves lies, so the column words and
// the gathers that the chunk's LAST iteration issues ahead (two trips and one trip ahead of the trip it consumes) are the first
// two trips of that next chunk, which then finds them in registers: the three loads that open a chunk run once per wavefront.
// Without LA the same three statements reach past the chunk's end and gather 64 copies of its last entry, which are thrown away
// when the chunk ends — at RMAT-22 a tenth of the gather slots the kernel issues.  With no next chunk the copies stay.
template <int QL, bool WIDE, int NT, bool LA>
__global__ __launch_bounds__(256) void xp_stream_kernel(const u32* __restrict__ pcol, const u32* __restrict__ pstart,
                                                        const u32* __restrict__ cstart, const u32* __restrict__ crun0,
                                                        const uint8_t* __restrict__ cshared, const uint4* __restrict__ x,
                                                        uint4* __restrict__ partial) {
    constexpr int SLOTS = 64 / QL;
    extern __shared__ uint4 s_tile[];                        // per wavefront XP_RUNS rows (the runs of one chunk) x QL quads
    const u32 lane = lane_id(), wl = lane % QL, slot = lane / QL, wib = threadIdx.x >> 6;
    uint4* tile = s_tile + (size_t)wib * XP_RUNS * QL;
    unsigned long long* tile64 = reinterpret_cast<unsigned long long*>(tile) + wl * 2;
    for (u32 i = lane; i < XP_RUNS * QL; i += 64) tile[i] = make_uint4(0, 0, 0, 0);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    const u32 part = blockIdx.x & 7u;
    const u32 wave = (u32)__builtin_amdgcn_readfirstlane((int)((blockIdx.x >> 3) * 4 + wib));
    const u32 nwaves = (gridDim.x >> 3) * 4;
    const u32 pe = pstart[part + 1];
    const u32 c0 = pstart[9 + part], nch = pstart[10 + part] - c0;
    const u64 upto = (2ull << (slot * QL)) - 1ull;            // entries 0 .. the slot's first one
    const char* xb = reinterpret_cast<const char*>(x) + wl * 16;
    // entry I + lane, held below LIM (a load past the end repeats the last entry: no branch around a load)
#define XP_COL(I, LIM) ((NT & 2) ? __builtin_nontemporal_load(&pcol[(I) + lane < (LIM) ? (I) + lane : (LIM) - 1]) : pcol[(I) + lane < (LIM) ? (I) + lane : (LIM) - 1])
#define XP_GATHER(XV, CW)                                                                                   \
    _Pragma("unroll") for (int k = 0; k < QL; ++k) {                                                        \
        const u32 uk = (u32)__shfl((int)(CW), (int)(slot * QL + k), 64) & ~XP_FIRST;                        \
        if (WIDE) XV[k] = *reinterpret_cast<const uint4*>(xb + (size_t)uk * (QL * 16));                     \
        else XV[k] = *reinterpret_cast<const uint4*>(xb + (u32)(uk * (u32)(QL * 16)));                      \
    }
    // what the table says of chunk j: its entries [B, E), the run (= partial row) of the first one, and whether that run began in
    // an earlier chunk / the run of the last one goes on in the next (the pieces of such a run meet through atomics)
    struct Chunk { u32 B, E, R0; bool first_atomic, last_atomic; };
    // a chunk's shared byte, read as the aligned word that holds it: a scalar load like the other table entries.  (As a byte it is a
    // vector load, and hipcc waits for vmcnt(0) — the gathers in flight — where it makes the value uniform, at the chunk's head.
    // The table is a block of its own with 8 spare zero bytes behind the last chunk's: the word of byte nchunks lies inside it.)
    const u32* shared32 = reinterpret_cast<const u32*>(cshared);
    auto shared_at = [&](u32 c) { return (((u32)__builtin_amdgcn_readfirstlane((int)shared32[c >> 2]) >> ((c & 3u) * 8u)) & 0xFFu) != 0u; };
    auto chunk_at = [&](u32 j) {
        Chunk c;
        c.B = (u32)__builtin_amdgcn_readfirstlane((int)cstart[c0 + j]);
        c.E = j + 1 < nch ? (u32)__builtin_amdgcn_readfirstlane((int)cstart[c0 + j + 1]) : pe;
        c.R0 = (u32)__builtin_amdgcn_readfirstlane((int)crun0[c0 + j]);
        c.first_atomic = shared_at(c0 + j);
        c.last_atomic = shared_at(c0 + j + 1) & (j + 1 < nch);   // (loaded whatever j is and masked: no branch around a load)
        return c;
    };
    if (wave >= nch) return;
    u32 cwE = 0, cwO = 0;
    uint4 xvE[QL], xvO[QL];
    Chunk cur{};
    if (LA) {   // the wavefront's first chunk opens the pipeline; every later one is opened by the chunk before it
        cur = chunk_at(wave);
        cwE = XP_COL(cur.B, cur.E);
        cwO = XP_COL(cur.B + 64, cur.E);
        XP_GATHER(xvE, cwE)
    }
    for (u32 j = wave; j < nch; j += nwaves) {
        // the wavefront's next chunk, read with this one's table entries, a whole chunk before the last iteration needs it.
        // (Without one the loads repeat this chunk's — no branch around a load — and the look-ahead stays at E - 1.)
        const bool more = LA && j + nwaves < nch;
        const Chunk nxt = LA ? chunk_at(more ? j + nwaves : j) : cur;
        if (!LA) cur = chunk_at(j);
        const u32 B = cur.B, E = cur.E, R0 = cur.R0;
        const bool first_atomic = cur.first_atomic, last_atomic = cur.last_atomic;
        const u32 aheadB = more ? nxt.B : E - 1u, aheadE = more ? nxt.E : E;
        u32 base = 0;                                        // runs of the chunk begun before the current trip (tile row of a carried run)
        // One trip: `mask` = the run starts among its 64 entries (lane = entry), `xv` = the rows of X of this slot's QL
        // consecutive entries.  Entries past the chunk's end are copies of its last entry (the loads clamp): no run starts on
        // them, so they OR the last run's own bits into it once more — no validity test anywhere.
        auto trip = [&](u64 mask, const uint4 (&xv)[QL]) {
            const u32 fb = (u32)(mask >> (slot * QL));       // bit k: entry k of this slot starts a run
            u32 row = base + (u32)__popcll(mask & upto);     // tile row (= run of the chunk) of the slot's first entry
            uint4 acc = xv[0];
#pragma unroll
            for (int k = 1; k < QL; ++k) {
                if ((fb >> k) & 1u) {
                    atomicOr(&tile64[(size_t)row * QL * 2], ((unsigned long long)acc.y << 32) | acc.x);
                    atomicOr(&tile64[(size_t)row * QL * 2 + 1], ((unsigned long long)acc.w << 32) | acc.z);
                    ++row;
                    acc = xv[k];
                } else {
                    acc = or4(acc, xv[k]);
                }
            }
            atomicOr(&tile64[(size_t)row * QL * 2], ((unsigned long long)acc.y << 32) | acc.x);
            atomicOr(&tile64[(size_t)row * QL * 2 + 1], ((unsigned long long)acc.w << 32) | acc.z);
            base += (u32)__popcll(mask);
        };
        // software pipeline, two trips per iteration (ping-pong registers: a rotation by moves would wait for the loads it
        // moves): the column words run TWO trips ahead of the trip being consumed and the gathers ONE, and every wait is for
        // loads OLDER than the ones that should stay in flight (vmcnt counts in issue order: a column word loaded after the
        // previous trip's gathers would drain them).  Loads past the chunk's end repeat its last entry (no branch around a
        // load); without LA that is an extra round of gathers per chunk, which hits the row it has just gathered.
        if (!LA) {
            cwE = XP_COL(B, E);
            cwO = XP_COL(B + 64, E);
            XP_GATHER(xvE, cwE)
        }
        for (u32 t = B; t < E; t += 128) {
            // run starts in entry order (lane = entry); the chunk's first entry never opens a NEW tile row
            const u64 maskE = __ballot(t + lane < E && (cwE & XP_FIRST) && !(t == B && lane == 0));
            // LA, the chunk's last iteration (uniform): trips t + 128 and t + 192 are trips 0 and 1 of the next chunk — two scalar
            // selects in front of the same two loads
            const bool ahead = LA && t + 128 >= E;
            const u32 at = ahead ? aheadB : t + 128, lim = ahead ? aheadE : E;
            cwE = XP_COL(at, lim);
            XP_GATHER(xvO, cwO)
            trip(maskE, xvE);
            // (no early exit when the chunk ends in an even trip: the odd one then runs on copies of the last entry — a branch
            // here makes hipcc merge the wait states of the two paths at the loop head into vmcnt(0))
            const u64 maskO = __ballot(t + 64 + lane < E && (cwO & XP_FIRST));
            cwO = XP_COL(at + 64, lim);
            XP_GATHER(xvE, cwE)
            trip(maskO, xvO);
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        // the chunk's runs leave the tile: run R0 + r, SLOTS rows per step; the first / last one through atomics when other chunks
        // hold pieces of it
        const u32 nr = base + 1;
        for (u32 r0 = 0; r0 < nr; r0 += SLOTS) {
            const u32 r = r0 + slot;
            if (r < nr) {
                const uint4 v4 = tile[r * QL + wl];
                uint4* dst = partial + (size_t)(R0 + r) * QL + wl;
                if ((r == 0 && first_atomic) || (r + 1 == nr && last_atomic)) atomic_or4(dst, v4);
                else if (NT & 1) xp_store_nt(dst, v4);
                else *dst = v4;
                tile[r * QL + wl] = make_uint4(0, 0, 0, 0);
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        if (LA) cur = nxt;
    }
#undef XP_COL
#undef XP_GATHER
}

// the fold: Y[v] = OR over the partitions of v's partial rows, then exactly what the plain pull does with a finished row —
// a touched row (a delta layer names it) goes to its slot of the side buffer, any other is counted (MODE 2: and its checksum
// terms summed through the nibble tables in LDS) and never written.  A wavefront per 64-row group, 64 / QL rows per step,
// the (up to) 8 partial rows of a vertex in flight together.  DIRECT: a (partition, row) pair that is one direct entry reads
// that entry's row of X in place of a partial row — the columns of the group's direct entries are loaded once per group, a
// lane per row, and every step takes its rows' ones by a shuffle, so a step still issues its 8 loads together, each from an
// address picked without a branch (partial row, row of X or the zero row).
__device__ __forceinline__ u64 xp_uniform64(u64 v) {
    return ((u64)(u32)__builtin_amdgcn_readfirstlane((int)(u32)(v >> 32)) << 32) | (u64)(u32)__builtin_amdgcn_readfirstlane((int)(u32)v);
}
// DENSE: the groups are 64 consecutive slots of the plan's gvtx (the rows that have an entry), and lane r's slot names its
// vertex — what the hash, the label bit and the touched bit are taken from.  The touched and label words then differ by lane:
// each lane gathers its own (only when a bitmap exists: wave-uniform, and not on the clean path), a ballot turns the bits into
// the group's 64-bit words that the rest of the fold tests as before, and the side-buffer slot of a touched row, which no
// longer follows from the group's word, is computed by the row's lane and taken by a shuffle.  A padded slot has no piece and
// reads nothing through its gvtx entry.
struct XpLaneRow {
    u32 vh;    // the vertex of this lane's row (0 on a padded slot: multiplied by an all-zero row)
    u32 sl;    // its side-buffer slot when it is touched
    u64 tw, lb;   // (wave-uniform) the group's touched rows and rows inside the label
};
__device__ __forceinline__ XpLaneRow xp_lane_row(u32 v, const BpFinal& fin) {
    XpLaneRow o;
    const bool live = v != XP_NO_VTX;
    const u32 vw = live ? v >> 6 : 0u, vb = v & 63u;
    o.vh = live ? v : 0u;
    o.sl = 0;
    o.tw = 0ull;
    o.lb = ~0ull;
    if (fin.tbits) {
        const u64 t = fin.tbits[vw];
        o.sl = fin.tpref[vw] + (u32)__popcll(t & ((1ull << vb) - 1ull));
        o.tw = __ballot(live && ((t >> vb) & 1ull));
    }
    if (fin.label) o.lb = __ballot(live && ((fin.label[vw] >> vb) & 1ull));
    return o;
}
template <int QL, int MODE, bool NT, bool DIRECT, bool DENSE>
__global__ __launch_bounds__(XP_FOLD_THREADS) void xp_fold_kernel(const u64* __restrict__ ne, const u32* __restrict__ pbase, u32 ng,
                                                      const uint4* __restrict__ partial, BpFinal fin, uint4* __restrict__ side,
                                                      u32 zrow /* an all-zero partial row */, const u64* __restrict__ de,
                                                      const u32* __restrict__ dbase, const u32* __restrict__ dcol,
                                                      const uint4* __restrict__ x, const u32* __restrict__ gvtx) {
    constexpr int SLOTS = 64 / QL;
    extern __shared__ u64 s_tab[];
    if (MODE == 2) {
        for (u32 i = threadIdx.x; i < fin.w * 256; i += blockDim.x) s_tab[i] = fin.tab[i];
        __syncthreads();
    }
    const u32 lane = lane_id(), wl = lane % QL, slot = lane / QL;
    const u32 wave = (u32)__builtin_amdgcn_readfirstlane((int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6));
    const u32 nwaves = (gridDim.x * blockDim.x) >> 6;
    constexpr u32 STR = 2 * QL + 1;                          // stage row stride in words (odd: the transposed reads spread over the banks)
    u64* stg = s_tab + (MODE == 2 ? (size_t)fin.w * 256 : 0) + (size_t)(threadIdx.x >> 6) * (32 * STR);   // MODE 2: 32 staged rows a wavefront
    u64 f_cnt = 0, f_sum = 0;
    for (u32 g = wave; g < ng; g += nwaves) {
        u64 nw[8], dw[8];
        u32 pb[8], dc[8];
        u64 any = 0ull;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            nw[k] = xp_uniform64(ne[(size_t)k * ng + g]);   // (wave-uniform: kept in scalar registers whatever the loads were)
            pb[k] = (u32)__builtin_amdgcn_readfirstlane((int)pbase[(size_t)k * ng + g]);
            any |= nw[k];
        }
        const u32 gv = DENSE ? gvtx[(size_t)g * 64 + lane] : 0u;   // lane r: the vertex of row r (one coalesced load with the header)
        if (DIRECT) {
            // lane k < 8 loads partition k's direct word and base (two loads, one round trip) and every lane takes them by
            // shuffles: they stay in vector registers — as 24 more scalars next to nw / pb they ran the kernel out of SGPRs, and
            // hipcc then issued the group's header loads one round trip at a time (a fold 45 % slower)
            const size_t kl = (size_t)(lane & 7u) * ng + g;
            const u64 dl = de[kl];
            const u32 bl = dbase[kl];
            u64 dany = 0ull;
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                dw[k] = ((u64)(u32)__shfl((int)(u32)(dl >> 32), k, 64) << 32) | (u64)(u32)__shfl((int)(u32)dl, k, 64);
                dc[k] = (u32)__shfl((int)bl, k, 64);
                dany |= dw[k];
            }
            any |= xp_uniform64(dany);
        }
        if (!any) continue;
        if (DIRECT) {
            const u64 lanes_below = (1ull << lane) - 1ull;
#pragma unroll
            for (int k = 0; k < 8; ++k)     // lane r: the column of (partition k, row 64 g + r) when that is a direct entry
                dc[k] = dcol[((dw[k] >> lane) & 1ull) ? dc[k] + (u32)__popcll(dw[k] & lanes_below) : 0u];
        }
        u64 tw, lb;
        u32 tp = 0;
        XpLaneRow lr = {0u, 0u, 0ull, 0ull};
        if (DENSE) {
            lr = xp_lane_row(gv, fin);
            tw = xp_uniform64(lr.tw);
            lb = xp_uniform64(lr.lb);
        } else {
            tw = fin.tbits ? xp_uniform64(fin.tbits[g]) : 0ull;      // (clean layers: no touched rows, no bitmap)
            tp = fin.tbits ? (u32)__builtin_amdgcn_readfirstlane((int)fin.tpref[g]) : 0u;
            lb = fin.label ? xp_uniform64(fin.label[g]) : ~0ull;
        }
        // Where the time goes (PMC, round 6, checksum on): not the partial rows — two steps of loads in flight changed nothing —
        // but LDS: 83 % of the LDS-active cycles were bank conflicts.  With a row's words spread over QL lanes, one look-up
        // instruction reads 2 QL different tables, and entry e of EVERY table sits in the same bank pair: 64 random 8-byte reads
        // over 16 bank pairs.  The look-ups now run after a half group (32 rows) is staged in LDS with a lane per ROW: an
        // instruction then reads ONE table per half wavefront (16 addresses, broadcast, no conflict).  The index arithmetic of a
        // step is scalar where it is the same for the step; a row without a piece in partition k loads the plan's zero row.
#pragma unroll 1
        for (u32 hf0 = 0; hf0 < 64; hf0 += (SLOTS >= 64 ? 64 : 32)) {        // (SLOTS = 64: one step is the whole group)
        u32 staged = 0;                                       // (wave-uniform) rows of this half staged for the look-ups
#pragma unroll 1
        for (u32 r0 = hf0; r0 < hf0 + 32 && r0 < 64; r0 += SLOTS) {
            if (((any >> r0) & (SLOTS == 64 ? ~0ull : ((1ull << (SLOTS % 64)) - 1ull))) == 0ull) continue;   // (wave-uniform)
            const u32 r = r0 + slot;
            const u64 below = (1ull << r) - 1ull;
            const u64 before = (1ull << r0) - 1ull;          // (wave-uniform)
            uint4 pv[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                u32 idx;
                if (SLOTS <= 32) {
                    const u32 fld = (u32)(nw[k] >> r0) & (SLOTS >= 32 ? 0xFFFFFFFFu : ((1u << (SLOTS % 32)) - 1u));   // scalar
                    const u32 first = pb[k] + (u32)__popcll(nw[k] & before);                                         // scalar
                    idx = ((fld >> slot) & 1u) ? first + (u32)__popc(fld & ((1u << slot) - 1u)) : zrow;
                } else {
                    idx = ((nw[k] >> r) & 1ull) ? pb[k] + (u32)__popcll(nw[k] & below) : zrow;
                }
                const uint4* src = partial + (size_t)idx * QL + wl;
                if (DIRECT) {
                    const u32 u = (u32)__shfl((int)dc[k], (int)r, 64);
                    src = ((dw[k] >> r) & 1ull) ? x + (size_t)u * QL + wl : src;
                }
                pv[k] = NT ? xp_load_nt(src) : *src;
            }
            uint4 a = or4(or4(or4(pv[0], pv[1]), or4(pv[2], pv[3])), or4(or4(pv[4], pv[5]), or4(pv[6], pv[7])));
            const bool touched = (tw >> r) & 1ull;
            const bool counted = !touched && ((lb >> r) & 1ull);
            const u32 slr = DENSE && tw ? (u32)__shfl((int)lr.sl, (int)r, 64) : 0u;   // (every lane: before the branch)
            if (touched && any4(a)) {
                const u32 sl = DENSE ? slr : tp + (u32)__popcll(tw & below);
                side[(size_t)sl * QL + wl] = a;              // the only writer of this slot before the delta fix-ups
            }
            const u32 pc = (u32)(__popc(a.x) + __popc(a.y) + __popc(a.z) + __popc(a.w));
            f_cnt += counted ? (u64)pc : 0ull;
            if (MODE == 2) {
                // (an all-zero word looks up entry 0 of its tables — zero — so nothing needs a test: words at or past fin.w are
                // zero by construction and their tables, past the end of s_tab, are never multiplied in)
                const u64 w0 = counted ? (((u64)a.y << 32) | a.x) : 0ull, w1 = counted ? (((u64)a.w << 32) | a.z) : 0ull;
                if (QL >= 2) {
                    u64* srow = stg + (size_t)(r & 31u) * STR + 2 * wl;
                    srow[0] = w0;
                    srow[1] = w1;
                    staged |= (u32)((SLOTS >= 32 ? 0xFFFFFFFFull : ((1ull << (SLOTS % 32)) - 1ull)) << (r0 & 31u));
                } else {
                    const u32 k0 = 2 * wl < fin.w ? 2 * wl : 0u, k1 = 2 * wl + 1 < fin.w ? 2 * wl + 1 : 0u;
                    const u64* t0 = s_tab + (size_t)k0 * 256;
                    const u64* t1 = s_tab + (size_t)k1 * 256;
                    u64 rs = 0;
#pragma unroll
                    for (int j = 0; j < 16; ++j) rs += t0[j * 16 + (u32)((w0 >> (4 * j)) & 15ull)];
#pragma unroll
                    for (int j = 0; j < 16; ++j) rs += t1[j * 16 + (u32)((w1 >> (4 * j)) & 15ull)];
                    f_sum += rs * cs_dest_hash(DENSE ? (u32)__shfl((int)lr.vh, (int)r, 64) : g * 64 + r);
                }
            }
        }
        if (MODE == 2 && QL >= 2 && staged) {
            // the half group's look-ups, a lane per row: lanes 0-31 take the first QL words of rows hf0 .. hf0 + 31, lanes 32-63
            // the other QL — every instruction reads one table per half wavefront
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            const u32 row = lane & 31u, hw = lane >> 5;
            const bool on = (staged >> row) & 1u;
            u64 rs = 0;
#pragma unroll 2
            for (u32 kk = 0; kk < (u32)QL; ++kk) {
                const u32 k = hw * QL + kk;
                const u64 w = on ? stg[(size_t)row * STR + k] : 0ull;
                const u64* tk = s_tab + (size_t)(k < fin.w ? k : 0u) * 256;
#pragma unroll
                for (int j = 0; j < 16; ++j) rs += tk[j * 16 + (u32)((w >> (4 * j)) & 15ull)];
            }
            rs += (u64)__shfl_xor((long long)rs, 32, 64);                 // the two halves of a row
            const u32 vr = DENSE ? (u32)__shfl((int)lr.vh, (int)(hf0 + row), 64) : g * 64 + hf0 + row;
            if (hw == 0 && on) f_sum += rs * cs_dest_hash(vr);
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");       // (read before the next half overwrites the stage)
            __builtin_amdgcn_wave_barrier();
        }
        }
    }
    bp_block_add2(f_cnt, MODE == 2 ? f_sum : 0ull, fin.acc);
}

// the fold by PIECE (expand_xp_fold = 1).  The slot fold above builds, at every step and on all 64 lanes, an index and an address
// for each of the 8 partitions — the QL lanes of a slot the same one QL times — and loads 8 rows per destination whether they
// exist or not: at RMAT-22 three of four are the plan's zero row, and the kernel is bound by instruction issue (VALU busy ~3/4 of
// its time, profiles/NOTES_r12.md), not by memory.  Here the index work is done ONCE per group with a lane per ROW: lane r finds
// which of (partition k, row 64 g + r) is a partial row, a direct entry or nothing, and where its pieces start in the group's
// list — the counts it needs are the popcounts it has just taken, so there is no scan.  The half group's lanes write their
// pieces (partial row, or XP_PIECE_X | slot of X; the row beside it) into a list in LDS, a slot of QL lanes takes one list
// entry, loads it — XP_INFL entries in flight per slot, from addresses picked without a branch — and ORs it into the row's
// words of the LDS stage (ds_or_b64), and the second phase of the slot fold, a lane per row, counts / looks up the staged words
// and leaves the stage zero.  Slots past the list's end load its first entry again and do not OR it in.
constexpr u32 XP_PIECE_X = 0x80000000u;   // bit 31 of a list entry: a row of X (partial rows < nnz < 2^31, slots of X < ncols < 2^31)
constexpr u32 XP_HALF_PIECES = 32 * 8;    // a half group's list: 32 rows x 8 partitions
constexpr int XP_INFL = 4;
template <int QL, int MODE, bool NT, bool DIRECT, bool DENSE>
__global__ __launch_bounds__(XP_FOLD_THREADS) void xp_fold_pieces_kernel(const u64* __restrict__ ne, const u32* __restrict__ pbase, u32 ng,
                                                             const uint4* __restrict__ partial, BpFinal fin, uint4* __restrict__ side,
                                                             const u64* __restrict__ de, const u32* __restrict__ dbase,
                                                             const u32* __restrict__ dcol, const uint4* __restrict__ x,
                                                             const u32* __restrict__ gvtx /* DENSE: see xp_fold_kernel */) {
    constexpr u32 SLOTS = 64 / QL;
    constexpr u32 STR = 2 * QL + 1;                          // stage row stride in words (odd: a lane per row reads without conflicts)
    constexpr u32 NW = XP_FOLD_THREADS / 64;
    extern __shared__ u64 s_tab[];
    const u32 ntab = MODE == 2 ? fin.w * 256 : 0u;
    const u32 lane = lane_id(), wl = lane % QL, slot = lane / QL, wib = threadIdx.x >> 6;
    u64* stg = s_tab + ntab + (size_t)wib * (32 * STR);      // 32 staged rows a wavefront, zero between the halves
    u32* lst = reinterpret_cast<u32*>(s_tab + ntab + (size_t)NW * (32 * STR)) + (size_t)wib * XP_HALF_PIECES;
    uint8_t* lrow = reinterpret_cast<uint8_t*>(s_tab + ntab + (size_t)NW * (32 * STR)) + (size_t)NW * XP_HALF_PIECES * sizeof(u32) +
                    (size_t)wib * XP_HALF_PIECES;
    if (MODE == 2)
        for (u32 i = threadIdx.x; i < ntab; i += blockDim.x) s_tab[i] = fin.tab[i];
    for (u32 i = lane; i < 32 * STR; i += 64) stg[i] = 0ull;
    __syncthreads();
    const u32 wave = (u32)__builtin_amdgcn_readfirstlane((int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6));
    const u32 nwaves = (gridDim.x * blockDim.x) >> 6;
    const u64 lanes_below = (1ull << lane) - 1ull;
    const u32 row = lane & 31u, hw = lane >> 5;              // second phase: lanes 0-31 the first QL words of a row, 32-63 the others
    u64 f_cnt = 0, f_sum = 0;
    for (u32 g = wave; g < ng; g += nwaves) {
        u64 nw[8], dw[8];
        u32 pb[8], ent[8];
        u64 any = 0ull;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            nw[k] = xp_uniform64(ne[(size_t)k * ng + g]);
            pb[k] = (u32)__builtin_amdgcn_readfirstlane((int)pbase[(size_t)k * ng + g]);
            any |= nw[k];
        }
        const u32 gv = DENSE ? gvtx[(size_t)g * 64 + lane] : 0u;   // lane r: the vertex of row r (one coalesced load with the header)
        if (DIRECT) {   // (lane k < 8 loads partition k's direct word and base: see xp_fold_kernel)
            const size_t kl = (size_t)(lane & 7u) * ng + g;
            const u64 dl = de[kl];
            const u32 bl = dbase[kl];
            u64 dany = 0ull;
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                dw[k] = ((u64)(u32)__shfl((int)(u32)(dl >> 32), k, 64) << 32) | (u64)(u32)__shfl((int)(u32)dl, k, 64);
                ent[k] = (u32)__shfl((int)bl, k, 64);
                dany |= dw[k];
            }
            any |= xp_uniform64(dany);
        }
        if (!any) continue;
        // lane r: its pieces, and how many the rows before it have (a run is a partial row OR a direct entry, never both)
        u32 have = 0, pref = 0;
        if (DIRECT) {
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const u32 db = (u32)__popcll(dw[k] & lanes_below);
                const u32 dbit = (u32)(dw[k] >> lane) & 1u;
                ent[k] = dcol[dbit ? ent[k] + db : 0u] | XP_PIECE_X;
                have |= dbit << k;
                pref += db;
            }
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const u32 nb = (u32)__popcll(nw[k] & lanes_below);
            const u32 bit = (u32)(nw[k] >> lane) & 1u;
            if (DIRECT) ent[k] = bit ? pb[k] + nb : ent[k];
            else ent[k] = pb[k] + nb;
            have |= bit << k;
            pref += nb;
        }
        u64 tw, lb;
        u32 tp = 0;
        XpLaneRow lr = {0u, 0u, 0ull, 0ull};
        if (DENSE) {
            lr = xp_lane_row(gv, fin);
            tw = xp_uniform64(lr.tw);
            lb = xp_uniform64(lr.lb);
        } else {
            tw = fin.tbits ? xp_uniform64(fin.tbits[g]) : 0ull;      // (clean layers: no touched rows, no bitmap)
            tp = fin.tbits ? (u32)__builtin_amdgcn_readfirstlane((int)fin.tpref[g]) : 0u;
            lb = fin.label ? xp_uniform64(fin.label[g]) : ~0ull;
        }
        const u32 tot0 = (u32)__builtin_amdgcn_readlane((int)pref, 32);   // pieces of rows 0 .. 31
        const u32 tot = (u32)__builtin_amdgcn_readlane((int)(pref + (u32)__popc(have)), 63);
#pragma unroll 1
        for (u32 hf = 0; hf < 2; ++hf) {
            const u32 np = hf ? tot - tot0 : tot0;           // (wave-uniform) pieces of this half
            if (!np) continue;
            if (hw == hf) {
                u32 pos = pref - (hf ? tot0 : 0u);
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    if ((have >> k) & 1u) {
                        lst[pos] = ent[k];
                        lrow[pos] = (uint8_t)row;
                        ++pos;
                    }
                }
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
#pragma unroll 1
            for (u32 j0 = 0; j0 < np; j0 += SLOTS * XP_INFL) {
                // (the list reads, then the loads, then the ORs — each kind issued together: left to itself hipcc interleaves them
                // and waits for every list read before the load that uses it)
                uint4 pv[XP_INFL];
                u32 pe[XP_INFL], pr[XP_INFL];
#pragma unroll
                for (int u = 0; u < XP_INFL; ++u) {
                    const u32 j = j0 + (u32)u * SLOTS + slot;
                    const u32 jc = j < np ? j : 0u;
                    pe[u] = lst[jc];
                    pr[u] = (u32)lrow[jc];
                }
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int u = 0; u < XP_INFL; ++u) {
                    const uint4* src = partial + (size_t)pe[u] * QL + wl;
                    if (DIRECT) src = (pe[u] & XP_PIECE_X) ? x + (size_t)(pe[u] & ~XP_PIECE_X) * QL + wl : src;
                    pv[u] = NT ? xp_load_nt(src) : *src;
                }
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int u = 0; u < XP_INFL; ++u) {
                    if (j0 + (u32)u * SLOTS + slot < np) {
                        unsigned long long* d = reinterpret_cast<unsigned long long*>(stg) + (size_t)pr[u] * STR + 2 * wl;
                        atomicOr(d, ((unsigned long long)pv[u].y << 32) | pv[u].x);
                        atomicOr(d + 1, ((unsigned long long)pv[u].w << 32) | pv[u].z);
                    }
                }
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            // rows a delta layer names leave for their slot of the side buffer (few: a slot pass over the half)
            const u32 twh = (u32)((tw & any) >> (32 * hf));
            if (twh) {
                for (u32 r0 = 0; r0 < 32; r0 += SLOTS) {
                    const u32 r = r0 + slot;
                    const u32 slr = DENSE ? (u32)__shfl((int)lr.sl, (int)((32 * hf + r) & 63u), 64) : 0u;   // (every lane: before the branch)
                    if (r < 32 && ((twh >> r) & 1u)) {
                        const u64 w0 = stg[(size_t)r * STR + 2 * wl], w1 = stg[(size_t)r * STR + 2 * wl + 1];
                        if (w0 | w1) {
                            const u32 sl = DENSE ? slr : tp + (u32)__popcll(tw & ((1ull << (32 * hf + r)) - 1ull));
                            side[(size_t)sl * QL + wl] = make_uint4((u32)w0, (u32)(w0 >> 32), (u32)w1, (u32)(w1 >> 32));   // the only writer of this slot
                        }
                    }
                }
            }
            // a lane per row: count, look up, clear
            const u32 rg = 32 * hf + row;
            const bool counted = !((tw >> rg) & 1ull) && ((lb >> rg) & 1ull);
            u64 rs = 0;
            u32 pc = 0;
#pragma unroll 2
            for (u32 kk = 0; kk < (u32)QL; ++kk) {
                const u32 k = hw * QL + kk;
                const u64 sw = stg[(size_t)row * STR + k];
                stg[(size_t)row * STR + k] = 0ull;
                const u64 w = counted ? sw : 0ull;
                pc += (u32)__popcll(w);
                if (MODE == 2) {
                    // (an all-zero word looks up entry 0 of its tables — zero; words at or past fin.w are zero by construction)
                    // the 16 reads of a word are issued together and summed as a tree: as a chain into one sum hipcc waits for every
                    // read before it issues the next, and a wavefront spends a look-up's LDS latency 16 times per word; without the
                    // scheduling barrier it still pairs them up to save registers
                    const u64* tk = s_tab + (size_t)(k < fin.w ? k : 0u) * 256;
                    u64 tv[16];
#pragma unroll
                    for (int j = 0; j < 16; ++j) tv[j] = tk[j * 16 + (u32)((w >> (4 * j)) & 15ull)];
                    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                    for (int d = 8; d >= 1; d >>= 1)
#pragma unroll
                        for (int j = 0; j < d; ++j) tv[j] += tv[j + d];
                    rs += tv[0];
                }
            }
            f_cnt += (u64)pc;
            if (MODE == 2) {
                rs += (u64)__shfl_xor((long long)rs, 32, 64);                 // the two halves of a row
                const u32 vr = DENSE ? (u32)__shfl((int)lr.vh, (int)rg, 64) : g * 64 + rg;
                if (hw == 0) f_sum += rs * cs_dest_hash(vr);
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");           // (cleared before the next half ORs into the stage)
            __builtin_amdgcn_wave_barrier();
        }
    }
    bp_block_add2(f_cnt, MODE == 2 ? f_sum : 0ull, fin.acc);
}

// LDS of the fold: MODE 2's checksum tables + a stage of 32 rows per wavefront; the piece fold stages in both modes and keeps a
// list of XP_HALF_PIECES entries (4 bytes + the row's byte) per wavefront
static size_t xp_fold_lds(u32 ws, int mode, size_t lds_tables, int pieces) {
    const size_t stage = (size_t)(XP_FOLD_THREADS / 64) * 32 * (ws + 1) * sizeof(u64);
    if (pieces) return (mode == 2 ? lds_tables : 0) + stage + (size_t)(XP_FOLD_THREADS / 64) * XP_HALF_PIECES * (sizeof(u32) + 1);
    return mode == 2 ? lds_tables + stage : 0;
}
// which fold a row width gets: the piece fold from expand_xp_fold_min_words words up (narrow rows: NOTES_r12 section 3.5)
static int xp_fold_by_pieces(const fgpu_ctx* ctx, u32 ws) {
    return ctx->opt.expand_xp_fold && ws >= (u32)ctx->opt.expand_xp_fold_min_words ? 1 : 0;
}
bool bp_xfold_fits(const fgpu_ctx* ctx, u32 ws, int mode, size_t lds_tables) {
    return xp_fold_lds(ws, mode, lds_tables, xp_fold_by_pieces(ctx, ws)) <= (size_t)ctx->opt.lds_limit;
}

// the partial rows that no chunk of the stream completes: the stream ORs into them, so they start from zero
static fgpu_info xp_zero_rows(fgpu_ctx* ctx, const BpXPlan* xp, u32 ql, uint4* partial) {
    if (!xp->nzrows) return FGPU_OK;
    u32 grid = cdiv(xp->nzrows, 256 / ql);
    if (grid > (u32)ctx->cus * 4) grid = ctx->cus * 4;
    return launch(xp_zero_rows_kernel, dim3(grid), dim3(256), 0, ctx->stream(), xp->zrows.p, xp->nzrows, ql, partial);
}

static fgpu_info xp_stream(fgpu_ctx* ctx, const BpXPlan* xp, const fgpu_mat* t, const u64* x, u32 ws, uint4* partial, u64 xrows) {
    // algorithmic bytes = what the HOP needs (SURVEY.md §8d's pull row): the entries of A' and its row pointers once, every
    // non-zero row of X once.  The partial rows are NOT in it — they exist only because of the partition, are written here and
    // read straight back by the fold (counting them made the kernel look 2.5 x closer to the roofline than the hop is)
    ProfScope ps(ctx, "xp_stream_kernel", 4 * xp->nentries + 4 * ((u64)xp->n + 1) + xrows * 8 * ws);
    const u32 ql = ws / 2;
    const size_t lds = (size_t)4 * XP_RUNS * ql * sizeof(uint4);
    u32 per_cu = (u32)((size_t)ctx->opt.lds_limit / lds);
    if (per_cu > 8) per_cu = 8;
    if (per_cu < 1) per_cu = 1;
    u32 most = 0;
    for (int k = 0; k < 8; ++k) most = std::max(most, xp->cbase[k + 1] - xp->cbase[k]);
    u32 grid = (u32)ctx->cus * per_cu;
    const u32 need = 8 * cdiv(most ? most : 1, 4);
    if (grid > need) grid = need;
    grid = (grid + 7) & ~7u;
    // expand_xp_stream_wgs: at most that many workgroups per partition (a small graph then has every wavefront walk many chunks)
    if (ctx->opt.expand_xp_stream_wgs > 0 && grid > 8u * (u32)ctx->opt.expand_xp_stream_wgs) grid = 8u * (u32)ctx->opt.expand_xp_stream_wgs;
    const bool wide = (u64)xp->n * ws * 8 > (1ull << 32) || (u64)t->ncols * ws * 8 > (1ull << 32);
    return pick<1, 2, 4, 8>((int)ql, [&](auto q) { return pick(wide, [&](auto w) { return pick<1, 2, 3, 0>(ctx->opt.expand_nt & 3, [&](auto nt) {
        return pick(ctx->opt.expand_xp_lookahead != 0, [&](auto la) {
            return launch(xp_stream_kernel<decltype(q)::value, decltype(w)::value, decltype(nt)::value, decltype(la)::value>, dim3(grid), dim3(256),
                          lds, ctx->stream(), xp->pcol.p, xp->pstart_dev.p, xp->cstart.p, xp->crun0.p, xp->cshared.p, (const uint4*)x, partial);
        });
    }); }); });
}

static fgpu_info xp_fold(fgpu_ctx* ctx, const BpXPlan* xp, const fgpu_mat* t, const u64* x, u32 ws, int mode, const BpFinal& fin,
                         u64* side, size_t lds_tables, const uint4* partial) {
    // (no algorithmic bytes of its own: everything it reads is the stream kernel's intermediate — bench.py quotes the hop,
    // stream + fold, against the stream kernel's bytes)
    // (the scope names the STEP, whichever of the two fold kernels runs it: bench.py quotes stream + fold under this name)
    ProfScope ps(ctx, "xp_fold_kernel", 0);
    // (4 or 8 wavefronts sharing one copy of the checksum tables, 16 or 32 resident per CU: the same 214 / 148 us with and
    // without the checksum at RMAT-22 — the kernel is not short of wavefronts)
    const u32 fthreads = XP_FOLD_THREADS;
    u32 grid = cdiv(xp->ng, fthreads / 64);
    if (grid > (u32)ctx->cus * (2048u / fthreads)) grid = ctx->cus * (2048u / fthreads);
    // (the count-hop planner takes the plain pull when this does not fit: bp_xfold_fits)
    const int pieces = xp_fold_by_pieces(ctx, ws);
    // (a list entry tags a slot of X with bit 31: the plan's own limits — nnz and columns below 2^31 — keep both kinds below it)
    FGPU_REQUIRE(!pieces || ((u64)xp->nprows < XP_PIECE_X && t->ncols < XP_PIECE_X), FGPU_INVALID,
                 "partitioned pull: the piece fold needs partial rows and columns below 2^31");
    (pieces ? ctx->xp_piece_folds : ctx->xp_slot_folds).fetch_add(1, std::memory_order_relaxed);
    const size_t lds = xp_fold_lds(ws, mode, lds_tables, pieces);
    FGPU_REQUIRE(lds <= (size_t)ctx->opt.lds_limit, FGPU_INVALID, "partitioned pull: the fold needs %zu B of LDS", lds);
    return pick<1, 2, 4, 8>((int)(ws / 2), [&](auto q) { return pick<2, 1>(mode, [&](auto md) { return pick((ctx->opt.expand_nt & 4) != 0, [&](auto nt) {
        return pick(xp->dense != 0, [&](auto dense) { return pick(xp->direct != 0, [&](auto direct) {
            constexpr int Q = decltype(q)::value, M = decltype(md)::value;
            constexpr bool N = decltype(nt)::value, D = decltype(direct)::value, G = decltype(dense)::value;
            if (pieces)
                return launch(xp_fold_pieces_kernel<Q, M, N, D, G>, dim3(grid), dim3(fthreads), lds, ctx->stream(), xp->ne.p, xp->pbase.p, xp->ng,
                              partial, fin, (uint4*)side, xp->de.p, xp->dbase.p, xp->dcol.p, (const uint4*)x, xp->gvtx.p);
            return launch(xp_fold_kernel<Q, M, N, D, G>, dim3(grid), dim3(fthreads), lds, ctx->stream(), xp->ne.p, xp->pbase.p, xp->ng,
                          partial, fin, (uint4*)side, xp->nprows, xp->de.p, xp->dbase.p, xp->dcol.p, (const uint4*)x, xp->gvtx.p);
        }); });
    }); }); });
}

fgpu_info bp_xpull_count(fgpu_ctx* ctx, const BpXPlan* xp, const fgpu_mat* t, const u64* x, u32 ws, int mode, const BpFinal& fin,
                         u64* side, size_t lds_tables, u64 xrows) {
    FGPU_REQUIRE(xp && xp->usable && ws >= 2 && ws <= 16 && (ws & (ws - 1)) == 0, FGPU_INVALID, "partitioned pull: bad plan / row width");
    FGPU_REQUIRE(mode == 1 || mode == 2, FGPU_INVALID, "partitioned pull: counting hops only");
    FGPU_REQUIRE(!xp->dense == !xp->gvtx.p, FGPU_INVALID, "partitioned pull: the plan's form and its slots disagree");
    // the read-only counters describe the hop's plan over ALL of A', also when the hop runs under the reduced plan beside it: which
    // pass of a whole-frontier call ends last is up to its lanes, and the counters of a snapshot must not depend on it (the
    // profiler scope xp_hub_rows says which hops took the short cut)
    const BpXPlan* rep = xp->full ? xp->full : xp;
    ctx->xp_last_direct.store(rep->ndirect, std::memory_order_relaxed);
    ctx->xp_last_groups.store(rep->ng, std::memory_order_relaxed);
    ctx->xp_last_chunks.store(rep->nchunks, std::memory_order_relaxed);
    ctx->xp_last_shared_rows.store(rep->nzrows - 1, std::memory_order_relaxed);   // (without the spare zero row)
    DevBuf<uint4> partial;
    FGPU_TRY(partial.alloc(ctx, ((size_t)xp->nprows + 1) * (ws / 2)));
    FGPU_TRY(xp_zero_rows(ctx, xp, ws / 2, partial.p));
    FGPU_TRY(xp_stream(ctx, xp, t, x, ws, partial.p, xrows));
    return xp_fold(ctx, xp, t, x, ws, mode, fin, side, lds_tables, partial.p);
}

}  // namespace fgpu
