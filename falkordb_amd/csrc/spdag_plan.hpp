// spdag_plan.hpp — the host side of fgpu_shortest_dag_batch (spdag_batch.hip): which queries form a group, which side every live
// query expands in a round, which segment of the shared pools every launch item may append to, and what the counters read back
// after a launch mean.  Plain C++17: no HIP, nothing of common.hpp, so a host program drives it over scripted read-backs
// (tests/host/spdag_plan_check.cpp).  The device code shares SdbDesc and SdbCtl with it and nothing else.
//
// A group is up to `slots` queries that advance in lock-step rounds; a query is a slot of the group.  Every round the planner
// emits one descriptor per live query (search) or per live sweep (phase 2, two per query: towards src and towards dst), the
// device runs one launch over the sum of their entry totals, and the planner folds the counters of every (slot, side) back
// into its copy of the query.  The rules of one query are those of the single call (spdag.hip), line by line: next_step() is
// its loop body, plan_sweeps() its Spdag::sweep.
//
// Pools.  All worklists of a group live in ONE array of vertex ids, handed out front to back: the two seeds of every slot, then
// per descriptor the segment its claimed vertices are appended to and (search) the segment of its meeting vertices.  A segment
// is reserved BEFORE the launch that fills it and is at least as long as anything that launch can append: a lane appends at
// most once per entry, and a side can claim at most nrows + 1 - (its queue length) more vertices.  So nothing truncates and the
// pools grow with the entries scanned, never with slots x nrows.  The pairs have a pool of their own, a pair per entry scanned.
// Segments are never reused inside a group: a later launch reads what an earlier one wrote (the frontier, the meeting set, the
// sweep queue), and the reset between groups walks them.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

namespace fgpu {
namespace sdb {

constexpr uint32_t SLOTS_MAX = 64;                    // FGPU_SPDAG_SLOTS_MAX
constexpr uint32_t NONE = 0xFFFFFFFFu;
constexpr uint64_t LAUNCH_ENTRIES_MAX = 0xFFFFFFFEull;   // a launch indexes its entries with 32 bits
constexpr uint64_t LEVEL_BYTES_MAX = 2ull << 30;         // the level words of a group: slots x 2 x nrows x 4 bytes

// one item of a launch: a frontier slice of one query and where its lanes may append.  Expansion: side 0 = forward over A,
// 1 = backward over At.  Sweep: side 0 = towards src (rows of At, levels of the forward ball), 1 = towards dst.  The reset and
// the pair compaction reuse the first five fields (side 2 / 3 there: the mark bits of sweep 0 / 1).
struct SdbDesc {
    uint32_t slot, side;
    uint32_t qbase, cnt;    // the input: pool[qbase .. qbase + cnt)
    uint32_t cbase;         // items before this one's in the launch's concatenated row list (exclusive prefix of cnt)
    uint32_t ebase, total;  // entries before this item's in the launch, and its own (the row lengths of its input, summed)
    uint32_t level;         // expansion: the level a claimed vertex gets; sweep: the level a predecessor must have
    uint32_t obase, ocap;   // claimed (sweep: newly marked) vertices go to pool[obase + (tail - tail0)], fewer than ocap
    uint32_t tail0;         // ctl.tail of (slot, side) before the launch
    uint32_t abase, acap;   // expansion: the meeting vertices, in the vertex pool; sweep: the pairs, in the pair pool
    uint32_t aux0;          // ctl.aux before the launch
    uint32_t direct;        // sweep towards dst at level 1: every input vertex emits (vertex, direct); NONE otherwise
    uint32_t pad;
};
static_assert(sizeof(SdbDesc) == 64, "SdbDesc is uploaded as 16 words");

// the device counters of one (slot, side), cumulative over the group's phase; read back whole after every launch
struct SdbCtl {
    uint32_t tail;       // vertices appended (search: the queue length, seeds included; sweep: vertices marked)
    uint32_t aux;        // search: meeting vertices listed; sweep: pairs emitted
    uint64_t ent;        // row lengths of every appended vertex, summed (sweep: and of the seeds)
    uint32_t overflow;   // an append found its segment full (never in a correct run)
    uint32_t pad;
};
static_assert(sizeof(SdbCtl) == 24, "SdbCtl is read back as 6 words");

// ---- groups -------------------------------------------------------------------------------------------------------------------
// slots == 0: as many queries together as the level words allow within LEVEL_BYTES_MAX, at most SLOTS_MAX and at most count
inline uint32_t derive_slots(uint64_t count, uint64_t nrows, uint32_t slots) {
    if (slots == 0) {
        const uint64_t fit = std::max<uint64_t>(1, LEVEL_BYTES_MAX / (8 * std::max<uint64_t>(nrows, 1)));
        slots = (uint32_t)std::min<uint64_t>(SLOTS_MAX, fit);
    }
    return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(slots, count));
}
inline uint64_t group_count(uint64_t count, uint32_t slots) { return (count + slots - 1) / slots; }
// group g holds the queries [first, first + n): whole groups of `slots` and a ragged last one
inline void group_range(uint64_t count, uint32_t slots, uint64_t g, uint64_t* first, uint32_t* n) {
    *first = g * slots;
    *n = (uint32_t)std::min<uint64_t>(slots, count - *first);
}

// ---- the side rule of the single call -----------------------------------------------------------------------------------------
inline int choose_side(int sides, uint32_t turn, uint64_t fent_fwd, uint64_t fent_bwd) {
    return sides == 1 ? 0 : sides == 2 ? 1 : sides == 3 ? (int)(turn & 1u) : (fent_fwd <= fent_bwd ? 0 : 1);
}

// ---- the pools ------------------------------------------------------------------------------------------------------------------
struct Pool {
    uint64_t used = 0;
    uint64_t reserve(uint64_t n) { const uint64_t at = used; used += n; return at; }
};

struct Seg { uint32_t slot, kind, base, cnt; };   // kind 0 / 1: level words of that side; 2 / 3: mark bits of that sweep

enum State { LIVE = 0, FOUND = 1, NOPATH = 2 };

struct Sweep {
    bool on = false;
    uint32_t qbase = 0, cnt = 0, d = 0;   // the input and the level of its vertices
    uint32_t tail = 0, pairs = 0;         // as last read
    uint64_t sent = 0, before = 0;        // ctl.ent as last read, and as it was before the launch that made the input
};

// the host's copy of one query of the group
struct Query {
    uint32_t slot = 0, src = 0, dst = 0;
    bool cycle = false, first_backward = false;   // the cycle shape still owes its unconditional backward expansion
    State state = LIVE;
    uint32_t r[2] = {0, 0}, head[2] = {0, 0}, cnt[2] = {1, 1}, tail[2] = {1, 1};
    uint64_t fent[2] = {0, 0}, ent[2] = {0, 0};   // entries of the current frontiers; ctl.ent as last read
    uint64_t levels[2] = {0, 0}, scanned = 0, swept = 0;
    uint32_t turn = 0, meet = 0, meet_base = 0;
    Sweep sw[2];
    std::vector<Seg> pairs;   // where the pair pool holds this query's pairs (kind unused)

    uint32_t length() const { return r[0] + r[1]; }
    uint64_t n_pairs() const { return (uint64_t)sw[0].pairs + sw[1].pairs; }
};

// slot `slot` of a group: its seeds are pool[2 * slot] = src and pool[2 * slot + 1] = dst (sdb_seed_kernel), out_deg / in_deg
// the lengths of src's row of A and dst's row of At as read back after the seeding
inline void seed_query(Query& q, uint32_t slot, uint32_t src, uint32_t dst) {
    q = Query();
    q.slot = slot;
    q.src = src;
    q.dst = dst;
    q.cycle = q.first_backward = src == dst;
    q.head[0] = 2 * slot;
    q.head[1] = 2 * slot + 1;
}
inline void seed_degrees(Query& q, uint64_t out_deg, uint64_t in_deg) {
    q.fent[0] = q.ent[0] = out_deg;
    q.fent[1] = q.ent[1] = in_deg;
}

// the single call's loop body: the side the query expands next, or -1 once it has left the search (state says how)
inline int next_step(Query& q, int sides, int64_t max_hops) {
    if (q.first_backward) {   // the backward side starts from the in-neighbours of src at level 1
        if (!q.fent[1]) { q.state = NOPATH; q.first_backward = false; return -1; }
        return 1;
    }
    if (q.meet) { q.state = FOUND; return -1; }
    if (max_hops >= 0 && (int64_t)q.r[0] + (int64_t)q.r[1] >= max_hops) { q.state = NOPATH; return -1; }
    const int side = choose_side(sides, q.turn, q.fent[0], q.fent[1]);
    if (!q.cnt[side] || !q.fent[side]) { q.state = NOPATH; return -1; }   // the frontier died
    return side;
}

struct Round {
    std::vector<SdbDesc> desc;
    uint64_t rows = 0, entries = 0;
    void clear() { desc.clear(); rows = entries = 0; }
    bool empty() const { return desc.empty(); }
};

inline void push_desc(Round& rd, SdbDesc d) {
    d.cbase = (uint32_t)rd.rows;
    d.ebase = (uint32_t)rd.entries;
    rd.rows += d.cnt;
    rd.entries += d.total;
    rd.desc.push_back(d);
}

// One search round over the group: a descriptor per query that is still searching.  A query whose entries would take the launch
// past LAUNCH_ENTRIES_MAX waits for the next round (its state is untouched).  false: the vertex pool would outgrow 32 bits.
inline bool plan_search(std::vector<Query>& qs, int sides, int64_t max_hops, uint64_t nrows, Pool& pool, Round& rd) {
    rd.clear();
    for (Query& q : qs) {
        if (q.state != LIVE) continue;
        const int s = next_step(q, sides, max_hops);
        if (s < 0) continue;
        const uint64_t total = q.fent[s];
        if (!rd.empty() && rd.entries + total > LAUNCH_ENTRIES_MAX) continue;
        if (q.first_backward) q.first_backward = false; else ++q.turn;
        const uint64_t cap = std::min<uint64_t>(total, nrows + 1 - q.tail[s]);
        SdbDesc d = {};
        d.slot = q.slot;
        d.side = (uint32_t)s;
        d.qbase = q.head[s];
        d.cnt = q.cnt[s];
        d.total = (uint32_t)total;
        d.level = q.r[s] + 1;
        d.obase = (uint32_t)pool.reserve(cap);
        d.abase = (uint32_t)pool.reserve(cap);
        d.ocap = d.acap = (uint32_t)cap;
        d.tail0 = q.tail[s];
        d.aux0 = 0;   // (the first level that lists a meeting vertex is the query's last)
        d.direct = NONE;
        if (pool.used > LAUNCH_ENTRIES_MAX) return false;
        push_desc(rd, d);
    }
    return true;
}

// ... and what its launch left in ctl[2 * slot + side]; segs receives the queue segments for the reset.  false: an overflow flag
inline bool apply_search(std::vector<Query>& qs, const Round& rd, const SdbCtl* ctl, std::vector<Seg>& segs) {
    for (const SdbDesc& d : rd.desc) {
        Query& q = qs[d.slot];
        const int s = (int)d.side;
        const SdbCtl& c = ctl[2 * d.slot + s];
        if (c.overflow) return false;
        ++q.r[s];
        ++q.levels[s];
        q.scanned += d.total;
        q.head[s] = d.obase;
        q.cnt[s] = c.tail - q.tail[s];
        q.tail[s] = c.tail;
        q.fent[s] = c.ent - q.ent[s];
        q.ent[s] = c.ent;
        if (q.cnt[s]) segs.push_back(Seg{d.slot, d.side, d.obase, q.cnt[s]});
        if (c.aux) {
            q.meet = c.aux;
            q.meet_base = d.abase;
        }
    }
    return true;
}

// Phase 2 of the found queries.  First the seeds: a descriptor per sweep over the meeting set, whose row lengths one launch sums
// into ctl.ent (apply_seeds reads them); then rounds of plan_sweeps / apply_sweeps until no sweep is on.
inline void plan_seeds(std::vector<Query>& qs, Round& rd) {
    rd.clear();
    for (Query& q : qs) {
        if (q.state != FOUND) continue;
        for (int s = 0; s < 2; ++s) {
            if (!q.r[s]) continue;   // (the ball of this side is its seed: the meeting set is the end of the DAG)
            Sweep& w = q.sw[s];
            w = Sweep();
            w.on = true;
            w.qbase = q.meet_base;
            w.cnt = q.meet;
            w.d = q.r[s];
            SdbDesc d = {};
            d.slot = q.slot;
            d.side = (uint32_t)s;
            d.qbase = w.qbase;
            d.cnt = w.cnt;
            d.direct = NONE;
            push_desc(rd, d);
        }
    }
}
inline void apply_seeds(std::vector<Query>& qs, const Round& rd, const SdbCtl* ctl) {
    for (const SdbDesc& d : rd.desc) qs[d.slot].sw[d.side].sent = ctl[2 * d.slot + d.side].ent;
}

inline bool plan_sweeps(std::vector<Query>& qs, uint64_t nrows, Pool& pool, Pool& pairs, Round& rd) {
    rd.clear();
    for (Query& q : qs) {
        if (q.state != FOUND) continue;
        for (int s = 0; s < 2; ++s) {
            Sweep& w = q.sw[s];
            if (!w.on) continue;
            const bool direct = s == 1 && w.d == 1;
            const uint64_t total = direct ? (uint64_t)w.cnt : w.sent - w.before;
            if (!w.cnt || !total) { w.on = false; continue; }
            if (!rd.empty() && rd.entries + total > LAUNCH_ENTRIES_MAX) continue;
            const uint64_t cap = direct ? 0 : std::min<uint64_t>(total, nrows);
            SdbDesc d = {};
            d.slot = q.slot;
            d.side = (uint32_t)s;
            d.qbase = w.qbase;
            d.cnt = w.cnt;
            d.total = (uint32_t)total;
            d.level = w.d - 1;
            d.obase = (uint32_t)pool.reserve(cap);
            d.ocap = (uint32_t)cap;
            d.tail0 = w.tail;
            d.abase = (uint32_t)pairs.reserve(total);
            d.acap = (uint32_t)total;
            d.aux0 = w.pairs;
            d.direct = direct ? q.dst : NONE;
            if (pool.used > LAUNCH_ENTRIES_MAX || pairs.used > LAUNCH_ENTRIES_MAX) return false;
            push_desc(rd, d);
        }
    }
    return true;
}

inline bool apply_sweeps(std::vector<Query>& qs, const Round& rd, const SdbCtl* ctl, std::vector<Seg>& segs) {
    for (const SdbDesc& d : rd.desc) {
        Query& q = qs[d.slot];
        Sweep& w = q.sw[d.side];
        const SdbCtl& c = ctl[2 * d.slot + d.side];
        if (c.overflow) return false;
        if (d.direct == NONE) q.swept += d.total;
        if (c.aux != w.pairs) q.pairs.push_back(Seg{d.slot, 0, d.abase, c.aux - w.pairs});
        w.pairs = c.aux;
        w.qbase = d.obase;
        w.cnt = c.tail - w.tail;
        w.tail = c.tail;
        w.before = w.sent;
        w.sent = c.ent;
        if (w.cnt) segs.push_back(Seg{d.slot, 2 + d.side, d.obase, w.cnt});
        if (--w.d == 0) w.on = false;
    }
    return true;
}

// the eight stats of the single call, from the query's counters
inline void fill_stats(const Query& q, uint64_t st[8]) {
    st[0] = q.levels[0];
    st[1] = q.levels[1];
    st[2] = q.tail[0] - 1;   // (without the seeds)
    st[3] = q.tail[1] - 1;
    st[4] = q.scanned;
    st[5] = st[7] = 0;
    st[6] = q.meet;
    if (q.state == FOUND) {
        st[5] = q.swept;
        st[7] = (uint64_t)q.meet + q.sw[0].tail + q.sw[1].tail + (q.r[1] ? 1 : 0);
    }
}

}  // namespace sdb
}  // namespace fgpu
