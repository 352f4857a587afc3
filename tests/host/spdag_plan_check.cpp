// spdag_plan_check.cpp — drives the round planner of fgpu_shortest_dag_batch (falkordb_amd/csrc/spdag_plan.hpp) on the host.
// The device is played by plain loops: every descriptor of a planned round is executed the way the kernels execute it (claim by
// level word, append behind the counter, count the row lengths), which scripts the counter read-backs the planner folds in.
// Checked while it runs, for spdag_sides 0 .. 3, several max_hops, groups of 1, 3, 7 and 64 slots:
//   - every reserved segment holds what its launch appends, and is at least min(entries to scan, nrows - claimed) long;
//   - no two segments handed out inside a group overlap, in the vertex pool and in the pair pool;
//   - the sides a query expands, in order, are those of the single call's loop (written out again below, from spdag.hip), the
//     cycle shape's first backward turn included, and so are its eight stats;
//   - length and pairs are those of two plain BFS distance arrays;
//   - groups of `slots` cover `count` in order with a ragged last group.
// Prints "ok <queries checked>" and exits 0, or says what failed and exits 1.  Built with -fsanitize=address,undefined by
// tests/test_spdag_plan_cpu.py and run as a child process.
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <deque>
#include <set>
#include <utility>
#include <vector>

#include "../../falkordb_amd/csrc/spdag_plan.hpp"

using namespace fgpu::sdb;
typedef uint32_t u32;
typedef uint64_t u64;

#define CHECK(cond, ...)                          \
    do {                                          \
        if (!(cond)) {                            \
            printf("FAILED %s:%d: ", __FILE__, __LINE__); \
            printf(__VA_ARGS__);                  \
            printf("\n");                         \
            exit(1);                              \
        }                                         \
    } while (0)

struct Csr {
    u32 n = 0;
    std::vector<u32> rp, ci;
    u32 len(u32 v) const { return rp[v + 1] - rp[v]; }
};
static Csr csr_of(u32 n, std::vector<std::pair<u32, u32>> e) {
    std::sort(e.begin(), e.end());
    e.erase(std::unique(e.begin(), e.end()), e.end());
    Csr m;
    m.n = n;
    m.rp.assign(n + 1, 0);
    for (auto& p : e) ++m.rp[p.first + 1];
    for (u32 v = 0; v < n; ++v) m.rp[v + 1] += m.rp[v];
    for (auto& p : e) m.ci.push_back(p.second);
    return m;
}
struct Graph {
    Csr m[2];   // A, At
};
static Graph graph_of(u32 n, const std::vector<std::pair<u32, u32>>& e) {
    std::vector<std::pair<u32, u32>> t;
    for (auto& p : e) t.push_back({p.second, p.first});
    Graph g;
    g.m[0] = csr_of(n, e);
    g.m[1] = csr_of(n, t);
    return g;
}

struct Answer {
    int64_t L = -1;
    std::vector<int> sides;   // the side of every expansion, in order
    u64 st[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    std::set<std::pair<u32, u32>> pairs;
};

// the single call: the host loop of fgpu_shortest_dag, on sets
static Answer single_call(const Graph& g, u32 src, u32 dst, int sides, int64_t max_hops) {
    const u32 n = g.m[0].n;
    Answer a;
    std::vector<u32> lvl[2] = {std::vector<u32>(n, NONE), std::vector<u32>(n, NONE)};
    std::vector<u32> fr[2] = {{src}, {dst}};
    u32 r[2] = {0, 0}, claimed[2] = {0, 0}, meet = 0;
    const bool cycle = src == dst;
    lvl[0][src] = 0;
    if (!cycle) lvl[1][dst] = 0;
    auto fent = [&](int s) { u64 t = 0; for (u32 v : fr[s]) t += g.m[s].len(v); return t; };
    auto expand = [&](int s) {
        std::vector<u32> next;
        a.st[4] += fent(s);
        for (u32 u : fr[s])
            for (u32 k = g.m[s].rp[u]; k < g.m[s].rp[u + 1]; ++k) {
                const u32 v = g.m[s].ci[k];
                if (lvl[s][v] != NONE) continue;
                lvl[s][v] = r[s] + 1;
                next.push_back(v);
                if (lvl[s ^ 1][v] != NONE) ++meet;
            }
        ++r[s];
        ++a.st[s];
        claimed[s] += (u32)next.size();
        fr[s] = next;
        a.sides.push_back(s);
    };
    bool found = false, dead = false;
    if (max_hops != 0 && !g.m[0].ci.empty()) {
        if (cycle) {
            if (!fent(1)) dead = true;
            else expand(1);
        }
        for (u32 turn = 0; !dead; ++turn) {
            if (meet) { found = true; break; }
            if (max_hops >= 0 && (int64_t)r[0] + r[1] >= max_hops) break;
            const int s = sides == 1 ? 0 : sides == 2 ? 1 : sides == 3 ? (int)(turn & 1u) : (fent(0) <= fent(1) ? 0 : 1);
            if (fr[s].empty() || !fent(s)) break;
            expand(s);
        }
        a.st[2] = claimed[0];
        a.st[3] = claimed[1];
        a.st[6] = meet;
    }
    if (found) a.L = r[0] + r[1];
    return a;
}

// length and pairs from two plain BFS distance arrays
static void plain_answer(const Graph& g, u32 src, u32 dst, int64_t max_hops, int64_t* L, std::set<std::pair<u32, u32>>* pairs) {
    const u32 n = g.m[0].n;
    auto bfs = [&](const Csr& m, u32 root) {
        std::vector<int64_t> d(n, -1);
        std::deque<u32> q{root};
        d[root] = 0;
        while (!q.empty()) {
            const u32 u = q.front();
            q.pop_front();
            for (u32 k = m.rp[u]; k < m.rp[u + 1]; ++k)
                if (d[m.ci[k]] < 0) { d[m.ci[k]] = d[u] + 1; q.push_back(m.ci[k]); }
        }
        return d;
    };
    const std::vector<int64_t> ds = bfs(g.m[0], src), dt = bfs(g.m[1], dst);
    *L = -1;
    pairs->clear();
    if (src != dst) {
        *L = ds[dst];
    } else {
        for (u32 k = g.m[1].rp[src]; k < g.m[1].rp[src + 1]; ++k) {
            const int64_t d = ds[g.m[1].ci[k]];
            if (d >= 0 && (*L < 0 || d + 1 < *L)) *L = d + 1;
        }
    }
    if (*L <= 0 || (max_hops >= 0 && *L > max_hops)) { *L = -1; return; }
    for (u32 u = 0; u < n; ++u)
        for (u32 k = g.m[0].rp[u]; k < g.m[0].rp[u + 1]; ++k) {
            const u32 v = g.m[0].ci[k];
            const int64_t tail = (src == dst && v == src) ? 0 : dt[v];
            if (ds[u] >= 0 && tail >= 0 && ds[u] + 1 + tail == *L) pairs->insert({u, v});
        }
}

// the device of one group
struct Device {
    const Graph* g;
    u32 n;
    std::vector<u32> pool, prow, pcol;
    std::vector<std::vector<u32>> lvl, bits;   // [2 * slot + side][v]
    std::vector<SdbCtl> ctl[2];                // search, sweeps
    std::vector<std::pair<u64, u64>> taken, ptaken;   // the segments handed out

    void expand(const SdbDesc& d) {
        SdbCtl& c = ctl[0][2 * d.slot + d.side];
        const Csr& m = g->m[d.side];
        std::vector<u32>& mine = lvl[2 * d.slot + d.side];
        const std::vector<u32>& other = lvl[2 * d.slot + (d.side ^ 1u)];
        u64 seen = 0;
        for (u32 i = 0; i < d.cnt; ++i) {
            const u32 u = pool[d.qbase + i];
            for (u32 k = m.rp[u]; k < m.rp[u + 1]; ++k, ++seen) {
                const u32 v = m.ci[k];
                if (mine[v] != NONE) continue;
                mine[v] = d.level;
                const u32 at = c.tail++ - d.tail0;
                CHECK(at < d.ocap, "slot %u side %u: claim %u outside a segment of %u", d.slot, d.side, at, d.ocap);
                pool[d.obase + at] = v;
                c.ent += m.len(v);
                if (other[v] != NONE) {
                    const u32 ma = c.aux++ - d.aux0;
                    CHECK(ma < d.acap, "slot %u side %u: meeting vertex %u outside a segment of %u", d.slot, d.side, ma, d.acap);
                    pool[d.abase + ma] = v;
                }
            }
        }
        CHECK(seen == d.total, "slot %u side %u: %llu entries, the descriptor says %u", d.slot, d.side, (unsigned long long)seen, d.total);
    }

    void sweep(const SdbDesc& d) {
        SdbCtl& c = ctl[1][2 * d.slot + d.side];
        const Csr& m = g->m[d.side ^ 1u];
        const std::vector<u32>& lv = lvl[2 * d.slot + d.side];
        std::vector<u32>& mark = bits[2 * d.slot + d.side];
        u64 seen = 0;
        auto emit = [&](u32 from, u32 to) {
            const u32 at = c.aux++ - d.aux0;
            CHECK(at < d.acap, "slot %u sweep %u: pair %u outside a segment of %u", d.slot, d.side, at, d.acap);
            prow[d.abase + at] = from;
            pcol[d.abase + at] = to;
        };
        for (u32 i = 0; i < d.cnt; ++i) {
            const u32 v = pool[d.qbase + i];
            if (d.direct != NONE) { emit(v, d.direct); ++seen; continue; }
            for (u32 k = m.rp[v]; k < m.rp[v + 1]; ++k, ++seen) {
                const u32 u = m.ci[k];
                if (lv[u] != d.level) continue;
                if (d.side == 0) emit(u, v); else emit(v, u);
                if (mark[u]) continue;
                mark[u] = 1;
                const u32 at = c.tail++ - d.tail0;
                CHECK(at < d.ocap, "slot %u sweep %u: vertex %u outside a segment of %u", d.slot, d.side, at, d.ocap);
                pool[d.obase + at] = u;
                c.ent += m.len(u);
            }
        }
        CHECK(seen == d.total, "slot %u sweep %u: %llu entries, the descriptor says %u", d.slot, d.side, (unsigned long long)seen, d.total);
    }
};

static void disjoint(std::vector<std::pair<u64, u64>> segs, const char* what) {
    segs.erase(std::remove_if(segs.begin(), segs.end(), [](const std::pair<u64, u64>& s) { return s.first == s.second; }), segs.end());
    std::sort(segs.begin(), segs.end());
    for (size_t i = 1; i < segs.size(); ++i)
        CHECK(segs[i - 1].second <= segs[i].first, "%s: segments [%llu, %llu) and [%llu, %llu) overlap", what,
              (unsigned long long)segs[i - 1].first, (unsigned long long)segs[i - 1].second, (unsigned long long)segs[i].first,
              (unsigned long long)segs[i].second);
}

static u64 checked = 0;

static void run_batch(const Graph& g, const std::vector<std::pair<u32, u32>>& queries, int sides, int64_t max_hops, u32 slots_arg) {
    const u32 n = g.m[0].n;
    const u64 count = queries.size();
    const u32 slots = derive_slots(count, n, slots_arg);
    CHECK(slots >= 1 && slots <= SLOTS_MAX && slots <= std::max<u64>(count, 1), "derive_slots(%llu, %u, %u) = %u", (unsigned long long)count, n, slots_arg, slots);
    if (slots_arg) CHECK(slots == std::min<u64>(slots_arg, count), "a given slots is kept");
    u64 covered = 0;
    Device dev;
    dev.g = &g;
    dev.n = n;
    dev.lvl.assign(2 * (size_t)slots, std::vector<u32>(n, NONE));
    dev.bits.assign(2 * (size_t)slots, std::vector<u32>(n, 0));
    for (u64 gi = 0; gi < group_count(count, slots); ++gi) {
        u64 first;
        u32 gn;
        group_range(count, slots, gi, &first, &gn);
        CHECK(first == covered && gn >= 1 && gn <= slots, "group %llu starts at %llu with %u queries", (unsigned long long)gi, (unsigned long long)first, gn);
        CHECK(gn == slots || first + gn == count, "only the last group is ragged");
        covered += gn;
        Pool pool, pairs;
        std::vector<Query> qs(gn);
        std::vector<Seg> segs;
        std::vector<std::vector<int>> turns(gn);
        dev.ctl[0].assign(2 * (size_t)gn, SdbCtl{});
        dev.ctl[1].assign(2 * (size_t)gn, SdbCtl{});
        dev.taken.clear();
        dev.ptaken.clear();
        dev.pool.assign(2 * (size_t)gn, 0);
        pool.reserve(2 * (u64)gn);
        dev.taken.push_back({0, 2 * (u64)gn});
        for (u32 j = 0; j < gn; ++j) {
            const u32 s = queries[first + j].first, d = queries[first + j].second;
            seed_query(qs[j], j, s, d);
            dev.pool[2 * j] = s;
            dev.pool[2 * j + 1] = d;
            dev.lvl[2 * j][s] = 0;
            if (s != d) dev.lvl[2 * j + 1][d] = 0;
            dev.ctl[0][2 * j].tail = dev.ctl[0][2 * j + 1].tail = 1;
            dev.ctl[0][2 * j].ent = g.m[0].len(s);
            dev.ctl[0][2 * j + 1].ent = g.m[1].len(d);
            seed_degrees(qs[j], dev.ctl[0][2 * j].ent, dev.ctl[0][2 * j + 1].ent);
            segs.push_back(Seg{j, 0, 2 * j, 1});
            segs.push_back(Seg{j, 1, 2 * j + 1, 1});
        }
        Round rd;
        const bool search = max_hops != 0 && !g.m[0].ci.empty();   // (the call returns before any group otherwise)
        for (u32 round = 0; search; ++round) {
            CHECK(round <= 2 * n + 4, "the search does not end");
            CHECK(plan_search(qs, sides, max_hops, n, pool, rd), "plan_search refused");
            if (rd.empty()) break;
            dev.pool.resize(pool.used);
            u64 rows = 0, entries = 0;
            std::set<u32> once;
            for (const SdbDesc& d : rd.desc) {
                CHECK(once.insert(d.slot).second, "slot %u twice in a search round", d.slot);
                CHECK(d.cbase == rows && d.ebase == entries && d.cnt > 0 && d.total > 0, "descriptor prefixes");
                rows += d.cnt;
                entries += d.total;
                u64 claimed = 0;
                for (u32 x : dev.lvl[2 * d.slot + d.side]) claimed += x != NONE;
                CHECK(d.ocap >= std::min<u64>(d.total, n - claimed), "slot %u side %u: %u slots for %u entries, %llu unclaimed", d.slot, d.side,
                      d.ocap, d.total, (unsigned long long)(n - claimed));
                CHECK(d.acap >= std::min<u64>(d.total, n - claimed), "slot %u side %u: meeting segment too short", d.slot, d.side);
                CHECK((u64)d.obase + d.ocap <= pool.used && (u64)d.abase + d.acap <= pool.used, "a segment outside the pool");
                dev.taken.push_back({d.obase, (u64)d.obase + d.ocap});
                dev.taken.push_back({d.abase, (u64)d.abase + d.acap});
                turns[d.slot].push_back((int)d.side);
            }
            CHECK(rows == rd.rows && entries == rd.entries && entries <= LAUNCH_ENTRIES_MAX, "round totals");
            for (const SdbDesc& d : rd.desc) dev.expand(d);
            CHECK(apply_search(qs, rd, dev.ctl[0].data(), segs), "apply_search saw an overflow");
        }
        plan_seeds(qs, rd);
        for (const SdbDesc& d : rd.desc) {
            u64 sum = 0;
            for (u32 i = 0; i < d.cnt; ++i) sum += g.m[d.side ^ 1u].len(dev.pool[d.qbase + i]);
            dev.ctl[1][2 * d.slot + d.side].ent += sum;
        }
        apply_seeds(qs, rd, dev.ctl[1].data());
        for (u32 round = 0; search; ++round) {
            CHECK(round <= 2 * n + 4, "the sweeps do not end");
            CHECK(plan_sweeps(qs, n, pool, pairs, rd), "plan_sweeps refused");
            if (rd.empty()) break;
            dev.pool.resize(pool.used);
            dev.prow.resize(pairs.used);
            dev.pcol.resize(pairs.used);
            for (const SdbDesc& d : rd.desc) {
                u64 marked = 0;
                for (u32 x : dev.bits[2 * d.slot + d.side]) marked += x;
                if (d.direct == NONE) CHECK(d.ocap >= std::min<u64>(d.total, n - marked), "slot %u sweep %u: queue segment too short", d.slot, d.side);
                CHECK(d.acap >= d.total, "slot %u sweep %u: %u pair slots for %u entries", d.slot, d.side, d.acap, d.total);
                CHECK((u64)d.obase + d.ocap <= pool.used && (u64)d.abase + d.acap <= pairs.used, "a segment outside its pool");
                dev.taken.push_back({d.obase, (u64)d.obase + d.ocap});
                dev.ptaken.push_back({d.abase, (u64)d.abase + d.acap});
            }
            for (const SdbDesc& d : rd.desc) dev.sweep(d);
            CHECK(apply_sweeps(qs, rd, dev.ctl[1].data(), segs), "apply_sweeps saw an overflow");
        }
        disjoint(dev.taken, "vertex pool");
        disjoint(dev.ptaken, "pair pool");
        for (u32 j = 0; j < gn; ++j) {
            const Query& q = qs[j];
            const Answer want = single_call(g, q.src, q.dst, sides, max_hops);
            CHECK(!search || q.state != LIVE, "query %u never left the search", j);
            const int64_t L = search && q.state == FOUND ? (int64_t)q.length() : -1;
            CHECK(L == want.L, "query (%u, %u) sides %d: length %lld, the single call finds %lld", q.src, q.dst, sides, (long long)L, (long long)want.L);
            CHECK(turns[j] == want.sides, "query (%u, %u) sides %d: the sides expanded differ from the single call's", q.src, q.dst, sides);
            u64 st[8] = {0, 0, 0, 0, 0, 0, 0, 0};
            if (search) fill_stats(q, st);
            for (int k : {0, 1, 2, 3, 4, 6}) CHECK(st[k] == want.st[k], "query (%u, %u) sides %d: stats[%d] %llu, single %llu", q.src, q.dst, sides, k,
                                                   (unsigned long long)st[k], (unsigned long long)want.st[k]);
            int64_t pl;
            std::set<std::pair<u32, u32>> pp, got;
            plain_answer(g, q.src, q.dst, max_hops, &pl, &pp);
            CHECK(L == pl, "query (%u, %u): length %lld, plain BFS says %lld", q.src, q.dst, (long long)L, (long long)pl);
            u64 k = 0;
            for (const Seg& s : q.pairs)
                for (u32 i = 0; i < s.cnt; ++i, ++k) got.insert({dev.prow[s.base + i], dev.pcol[s.base + i]});
            CHECK(k == got.size() && k == q.n_pairs(), "query (%u, %u): a pair twice", q.src, q.dst);
            CHECK(got == pp, "query (%u, %u) sides %d: %zu pairs, plain BFS says %zu", q.src, q.dst, sides, got.size(), pp.size());
            std::set<u32> dag;
            for (auto& p : pp) { dag.insert(p.first); dag.insert(p.second); }
            if (L > 0) CHECK(st[7] == dag.size() + (q.src == q.dst ? 1 : 0), "query (%u, %u): stats[7] %llu, the DAG has %zu vertices", q.src, q.dst,
                             (unsigned long long)st[7], dag.size());
            ++checked;
        }
        // the reset: what the segments name is all that was set
        for (const Seg& s : segs)
            for (u32 i = 0; i < s.cnt; ++i) {
                const u32 v = dev.pool[s.base + i];
                if (s.kind < 2) dev.lvl[2 * s.slot + s.kind][v] = NONE;
                else dev.bits[2 * s.slot + (s.kind - 2)][v] = 0;
            }
        for (auto& l : dev.lvl) for (u32 x : l) CHECK(x == NONE, "a level word survived the reset");
        for (auto& b : dev.bits) for (u32 x : b) CHECK(x == 0, "a mark survived the reset");
    }
    CHECK(covered == count, "the groups cover %llu of %llu queries", (unsigned long long)covered, (unsigned long long)count);
}

int main() {
    // derive_slots: the level words of a group stay within 2 GiB
    CHECK(derive_slots(1000, 1u << 22, 0) == 64 && derive_slots(1000, 1u << 23, 0) == 32 && derive_slots(1000, 0xFFFFFFFEu, 0) == 1,
          "derive_slots by vertex count");
    CHECK(derive_slots(5, 100, 0) == 5 && derive_slots(0, 100, 0) == 1 && derive_slots(200, 100, 7) == 7, "derive_slots by query count");
    for (int sides = 0; sides < 4; ++sides)
        for (u32 turn = 0; turn < 3; ++turn)
            for (u64 f : {0, 3, 9})
                for (u64 b : {0, 3, 9})
                    CHECK(choose_side(sides, turn, f, b) == (sides == 1 ? 0 : sides == 2 ? 1 : sides == 3 ? (int)(turn & 1) : (f <= b ? 0 : 1)),
                          "choose_side");

    std::vector<Graph> graphs;
    u64 rng = 0x9E3779B97F4A7C15ull;
    auto next = [&]() { rng ^= rng << 13; rng ^= rng >> 7; rng ^= rng << 17; return rng; };
    for (u32 n : {9u, 23u, 40u}) {   // random multigraphs with self-loops, about two entries per vertex
        std::vector<std::pair<u32, u32>> e;
        for (u32 k = 0; k < 2 * n; ++k) e.push_back({(u32)(next() % n), (u32)(next() % n)});
        graphs.push_back(graph_of(n, e));
        std::vector<std::pair<u32, u32>> sym = e;
        for (auto& p : e) sym.push_back({p.second, p.first});
        graphs.push_back(graph_of(n, sym));
    }
    {   // a path with a tail and an isolated vertex; a hub between two vertices; an empty matrix
        std::vector<std::pair<u32, u32>> e;
        for (u32 v = 0; v + 1 < 12; ++v) e.push_back({v, v + 1});
        graphs.push_back(graph_of(13, e));
        e.clear();
        for (u32 v = 1; v <= 30; ++v) { e.push_back({0, v}); e.push_back({v, 31}); e.push_back({v, 0}); }
        graphs.push_back(graph_of(33, e));
        graphs.push_back(graph_of(5, {}));
    }
    for (const Graph& g : graphs) {
        const u32 n = g.m[0].n;
        std::vector<std::pair<u32, u32>> all;
        for (u32 s = 0; s < n; ++s)
            for (u32 d = 0; d < n; ++d)
                if (n <= 13 || (s * 7 + d * 3) % 5 == 0 || s == d) all.push_back({s, d});
        for (int sides = 0; sides < 4; ++sides)
            for (int64_t mh : {-1, 0, 1, 2, 3, 5})
                for (u32 slots : {0u, 1u, 3u, 7u, 64u}) {
                    if (slots == 1 && (sides == 3 || mh == 1)) continue;   // (keeps the run short: one slot is the slowest shape)
                    run_batch(g, all, sides, mh, slots);
                }
    }
    run_batch(graphs[0], {}, 0, -1, 0);
    printf("ok %llu\n", (unsigned long long)checked);
    return 0;
}
