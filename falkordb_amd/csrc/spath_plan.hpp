// spath_plan.hpp — the host side of fgpu_shortest_path_batch (spath_batch.hip): which queries form a group, which side every live
// query expands in a round, which segment of the vertex pool receives a round's claimed vertices, and what the counters read
// back after a round mean.  Plain C++17: no HIP, nothing of common.hpp, so a host program drives it over scripted read-backs
// (tests/host/spath_plan_check.cpp).  The device code shares SpDesc, SpCtl and SpWalk with it and nothing else.
//
// The rules of one query are the reference's bfs_shortest_path (runtime/eval.rs:1386-1471), restated in include/fgpu.h:
// next_step() is its loop head — a dead frontier or df + db >= max_hops ends the search, the forward side expands iff it has
// at most as many frontier VERTICES as the backward side — and apply_search() its loop tail.  A frontier whose rows hold no
// entry is a level all the same (the reference walks it and finds nothing): plan_search() books it on the host, no launch.
//
// Pool.  All frontiers of a group live in ONE array of vertex ids, handed out front to back: the two seeds of every slot, then
// per descriptor the segment its claimed vertices are placed in, in key order.  A segment is reserved BEFORE the round that
// fills it and holds min(entries, nrows) ids: an entry claims at most one vertex.  Segments are never reused inside a group:
// the next round reads them as its frontier and the reset between groups walks them.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

namespace fgpu {
namespace spb {

constexpr uint32_t SLOTS_MAX = 64;                       // FGPU_SPATH_SLOTS_MAX
constexpr uint32_t NONE = 0xFFFFFFFFu;
constexpr uint64_t NO_MEET = ~0ull;
constexpr uint64_t LAUNCH_ENTRIES_MAX = 0xFFFFFFFEull;   // a launch indexes its entries with 32 bits
constexpr uint64_t STATE_BYTES_MAX = 2ull << 30;         // claim words and parents of a group: slots x nrows x 24 bytes

// one item of a round: the frontier of one query's expanding side and where the claimed vertices go.  side 0 = forward over
// F, 1 = backward over B.  The reset reuses slot, side, qbase, cnt and cbase.
struct SpDesc {
    uint32_t slot, side;
    uint32_t qbase, cnt;    // the frontier: pool[qbase .. qbase + cnt), in frontier order
    uint32_t cbase;         // rows before this item's in the round's concatenated row list (exclusive prefix of cnt)
    uint32_t ebase, total;  // entries before this item's in the round, and its own: the key of entry e is e - ebase
    uint32_t level;         // the depth a claimed vertex gets
    uint32_t obase, ocap;   // the claimed vertices go to pool[obase ..), in key order, at most ocap
    uint32_t pad[6];
};
static_assert(sizeof(SpDesc) == 64, "SpDesc is uploaded as 16 words");

// the device counters of one slot; read back whole after every round
struct SpCtl {
    uint64_t meet;      // (other side's depth << 32) | key, the least over the meeting candidates; NO_MEET without one
    uint64_t ent[2];    // row lengths of every claimed vertex of the side, summed over the group's rounds (seeds included)
    uint32_t cnt[2];    // vertices the side's last round claimed
    uint32_t cand;      // meeting candidates
    uint32_t meetv;     // the vertex behind meet's key
};
static_assert(sizeof(SpCtl) == 40, "SpCtl is read back as 10 words");

// one found query for the path walk: nodes[off .. off + length] receives src .. meet .. dst
struct SpWalk {
    uint32_t slot, meet, length, pad;
    uint64_t off;
};
static_assert(sizeof(SpWalk) == 24, "SpWalk is uploaded as 6 words");

// ---- groups -------------------------------------------------------------------------------------------------------------------
// slots == 0: as many queries together as the dense state allows within STATE_BYTES_MAX, at most SLOTS_MAX and at most count
inline uint32_t derive_slots(uint64_t count, uint64_t nrows, uint32_t slots) {
    if (slots == 0) {
        const uint64_t fit = std::max<uint64_t>(1, STATE_BYTES_MAX / (24 * std::max<uint64_t>(nrows, 1)));
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

struct Pool {
    uint64_t used = 0;
    uint64_t reserve(uint64_t n) { const uint64_t at = used; used += n; return at; }
};

struct Seg { uint32_t slot, side, base, cnt; };   // vertices whose claim word of (slot, side) is set

enum State { LIVE = 0, FOUND = 1, NOPATH = 2 };

// the host's copy of one query of the group
struct Query {
    uint32_t slot = 0, src = 0, dst = 0;
    State state = LIVE;
    uint32_t r[2] = {0, 0}, head[2] = {0, 0}, cnt[2] = {1, 1};   // completed depth, the frontier's place and vertex count
    uint64_t fent[2] = {0, 0}, ent[2] = {0, 0};                   // entries of the current frontiers; ctl.ent as last read
    uint64_t levels[2] = {0, 0}, claimed[2] = {0, 0}, walked = 0;
    uint32_t cand = 0, meetv = NONE, length = 0;
};

// slot `slot` of a group: its seeds are pool[2 * slot] = src and pool[2 * slot + 1] = dst; src == dst has no path
inline void seed_query(Query& q, uint32_t slot, uint32_t src, uint32_t dst) {
    q = Query();
    q.slot = slot;
    q.src = src;
    q.dst = dst;
    q.head[0] = 2 * slot;
    q.head[1] = 2 * slot + 1;
    if (src == dst) q.state = NOPATH;
}
// the lengths of src's row of F and dst's row of B as read back after the seeding
inline void seed_degrees(Query& q, uint64_t out_deg, uint64_t in_deg) {
    q.fent[0] = q.ent[0] = out_deg;
    q.fent[1] = q.ent[1] = in_deg;
}

// the loop head: the side the query expands next, or -1 once it has left the search without a path
inline int next_step(Query& q, int64_t max_hops) {
    if (!q.cnt[0] || !q.cnt[1] || (max_hops >= 0 && (int64_t)q.r[0] + (int64_t)q.r[1] >= max_hops)) {
        q.state = NOPATH;
        return -1;
    }
    return q.cnt[0] <= q.cnt[1] ? 0 : 1;   // vertex counts, not entry counts
}

struct Round {
    std::vector<SpDesc> desc;
    uint64_t rows = 0, entries = 0;
    void clear() { desc.clear(); rows = entries = 0; }
    bool empty() const { return desc.empty(); }
};

inline void push_desc(Round& rd, SpDesc d) {
    d.cbase = (uint32_t)rd.rows;
    d.ebase = (uint32_t)rd.entries;
    rd.rows += d.cnt;
    rd.entries += d.total;
    rd.desc.push_back(d);
}

// One round over the group: a descriptor per query that is still searching and has entries to walk.  A query whose entries
// would take the round past LAUNCH_ENTRIES_MAX waits for the next one (its state is untouched).  false: the vertex pool would
// outgrow 32 bits.
inline bool plan_search(std::vector<Query>& qs, int64_t max_hops, uint64_t nrows, Pool& pool, Round& rd) {
    rd.clear();
    for (Query& q : qs) {
        while (q.state == LIVE) {
            const int s = next_step(q, max_hops);
            if (s < 0) break;
            const uint64_t total = q.fent[s];
            if (total == 0) {   // a level without an entry: nothing claimed, the frontier dies
                ++q.r[s];
                ++q.levels[s];
                q.cnt[s] = 0;
                continue;
            }
            if (!rd.empty() && rd.entries + total > LAUNCH_ENTRIES_MAX) break;
            const uint64_t cap = std::min<uint64_t>(total, nrows);
            SpDesc d = {};
            d.slot = q.slot;
            d.side = (uint32_t)s;
            d.qbase = q.head[s];
            d.cnt = q.cnt[s];
            d.total = (uint32_t)total;
            d.level = q.r[s] + 1;
            d.obase = (uint32_t)pool.reserve(cap);
            d.ocap = (uint32_t)cap;
            if (pool.used > LAUNCH_ENTRIES_MAX) return false;
            push_desc(rd, d);
            break;
        }
    }
    return true;
}

// ... and what its launches left in ctl[slot]; segs receives the claimed segments for the reset.  false: a segment overran
inline bool apply_search(std::vector<Query>& qs, const Round& rd, const SpCtl* ctl, std::vector<Seg>& segs) {
    for (const SpDesc& d : rd.desc) {
        Query& q = qs[d.slot];
        const int s = (int)d.side;
        const SpCtl& c = ctl[d.slot];
        if (c.cnt[s] > d.ocap) return false;
        ++q.r[s];
        ++q.levels[s];
        q.walked += d.total;
        q.head[s] = d.obase;
        q.cnt[s] = c.cnt[s];
        q.claimed[s] += c.cnt[s];
        q.fent[s] = c.ent[s] - q.ent[s];
        q.ent[s] = c.ent[s];
        if (c.cnt[s]) segs.push_back(Seg{d.slot, d.side, d.obase, c.cnt[s]});
        if (c.meet != NO_MEET) {   // the level ran to its end; the least (other depth, key) is the meeting vertex
            q.state = FOUND;
            q.cand = c.cand;
            q.meetv = c.meetv;
            q.length = d.level + (uint32_t)(c.meet >> 32);
        }
    }
    return true;
}

// the eight stats of a query, from its counters
inline void fill_stats(const Query& q, uint64_t st[8]) {
    st[0] = q.levels[0];
    st[1] = q.levels[1];
    st[2] = q.claimed[0];
    st[3] = q.claimed[1];
    st[4] = q.walked;
    st[5] = q.state == FOUND ? (uint64_t)q.meetv : ~0ull;
    st[6] = q.cand;
    st[7] = 0;
}

}  // namespace spb
}  // namespace fgpu
