// spath_plan_check.cpp — drives the round planner of fgpu_shortest_path_batch (falkordb_amd/csrc/spath_plan.hpp) on the host.
// The device is played by plain loops that do what the kernels do, in the kernels' terms: every entry of a descriptor gets its
// key, the claim words take the minimum of (level << 32 | key), the entries whose value the word holds are the winners, they
// store the parent, lower the meeting word where the other ball holds the vertex, and are placed in key order; the counters
// the planner folds in are scripted that way.  The entries are claimed in REVERSE key order, so a device that depended on
// arrival order would show.
// Checked while it runs, for several max_hops and groups of 1, 3, 7 and 64 slots:
//   - every reserved segment holds what its round places and lies inside the pool; no two segments of a group overlap;
//   - a descriptor has rows and entries, and its prefixes are the running sums;
//   - path, length and the eight stats of every query are those of the contract's loop, written out again below on hash maps
//     (the side by vertex count, the first discoverer as parent, the first candidate of the least other depth);
//   - the reset that walks the segments leaves no claim word set;
//   - groups of `slots` cover `count` in order with a ragged last group.
// Prints "ok <queries checked>" and exits 0, or says what failed and exits 1.  Built with -fsanitize=address,undefined by
// tests/test_spath_plan_cpu.py and run as a child process.
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <map>
#include <set>
#include <utility>
#include <vector>

#include "../../falkordb_amd/csrc/spath_plan.hpp"

using namespace fgpu::spb;
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
    Csr m[2];   // F, B
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
    std::vector<u32> path;   // empty: none
    u64 st[8] = {0, 0, 0, 0, 0, ~0ull, 0, 0};
};

// the contract's loop, on maps
static Answer contract(const Graph& g, u32 src, u32 dst, int64_t max_hops) {
    Answer a;
    if (src == dst) return a;
    std::map<u32, std::pair<u32, u32>> ball[2];   // vertex -> (parent, depth)
    ball[0][src] = {src, 0};
    ball[1][dst] = {dst, 0};
    std::vector<u32> fr[2] = {{src}, {dst}};
    u32 depth[2] = {0, 0};
    bool met = false;
    u32 best_od = 0, meet = 0;
    while (!met) {
        if (fr[0].empty() || fr[1].empty() || (max_hops >= 0 && (int64_t)depth[0] + depth[1] >= max_hops)) return a;
        const int s = fr[0].size() <= fr[1].size() ? 0 : 1;
        const Csr& m = g.m[s];
        std::vector<u32> next;
        u64 cands = 0;
        for (u32 cur : fr[s])
            for (u32 k = m.rp[cur]; k < m.rp[cur + 1]; ++k) {
                ++a.st[4];
                const u32 nb = m.ci[k];
                if (ball[s].count(nb)) continue;
                ball[s][nb] = {cur, depth[s] + 1};
                ++a.st[2 + s];
                auto o = ball[s ^ 1].find(nb);
                if (o != ball[s ^ 1].end()) {
                    ++cands;
                    if (!met || o->second.second < best_od) { met = true; best_od = o->second.second; meet = nb; }
                } else {
                    next.push_back(nb);
                }
            }
        fr[s] = next;
        ++depth[s];
        ++a.st[s];
        a.st[6] = cands;
    }
    a.st[5] = meet;
    a.path.push_back(meet);
    while (a.path.back() != src) a.path.push_back(ball[0][a.path.back()].first);
    std::reverse(a.path.begin(), a.path.end());
    while (a.path.back() != dst) a.path.push_back(ball[1][a.path.back()].first);
    return a;
}

// the device of one group
struct Device {
    const Graph* g;
    u32 n;
    std::vector<u32> pool;
    std::vector<std::vector<u64>> word;   // [2 * slot + side][v]
    std::vector<std::vector<u32>> par;
    std::vector<SpCtl> ctl;

    void round(const SpDesc& d) {
        const Csr& m = g->m[d.side];
        std::vector<u64>& mine = word[2 * d.slot + d.side];
        const std::vector<u64>& other = word[2 * d.slot + (d.side ^ 1u)];
        std::vector<std::pair<u32, u32>> ent;   // (frontier vertex, column) by key
        for (u32 i = 0; i < d.cnt; ++i) {
            const u32 u = pool[d.qbase + i];
            for (u32 k = m.rp[u]; k < m.rp[u + 1]; ++k) ent.push_back({u, m.ci[k]});
        }
        CHECK(ent.size() == d.total, "slot %u side %u: %zu entries, the descriptor says %u", d.slot, d.side, ent.size(), d.total);
        for (size_t key = ent.size(); key-- > 0;) {   // claim, last key first
            const u64 val = ((u64)d.level << 32) | key;
            if (val < mine[ent[key].second]) mine[ent[key].second] = val;
        }
        SpCtl& c = ctl[d.slot];
        u32 rank = 0;
        for (size_t key = 0; key < ent.size(); ++key) {   // resolve and place
            const u32 v = ent[key].second;
            if (mine[v] != (((u64)d.level << 32) | key)) continue;
            par[2 * d.slot + d.side][v] = ent[key].first;
            if (other[v] != ~0ull) {
                c.meet = std::min<u64>(c.meet, (other[v] & 0xFFFFFFFF00000000ull) | key);
                ++c.cand;
            }
            CHECK(rank < d.ocap, "slot %u side %u: winner %u outside a segment of %u", d.slot, d.side, rank, d.ocap);
            pool[d.obase + rank++] = v;
            c.ent[d.side] += m.len(v);
        }
        c.cnt[d.side] = rank;
        if (c.meet != NO_MEET) c.meetv = ent[(u32)c.meet].second;
    }

    std::vector<u32> walk(u32 slot, u32 meet, u32 length, u32 src, u32 dst) const {
        std::vector<u32> p{meet};
        while (p.back() != src) { CHECK(p.size() <= length, "forward parents do not reach src"); p.push_back(par[2 * slot][p.back()]); }
        std::reverse(p.begin(), p.end());
        while (p.back() != dst) { CHECK(p.size() <= length, "backward parents do not reach dst"); p.push_back(par[2 * slot + 1][p.back()]); }
        return p;
    }
};

static void disjoint(std::vector<std::pair<u64, u64>> segs) {
    segs.erase(std::remove_if(segs.begin(), segs.end(), [](const std::pair<u64, u64>& s) { return s.first == s.second; }), segs.end());
    std::sort(segs.begin(), segs.end());
    for (size_t i = 1; i < segs.size(); ++i)
        CHECK(segs[i - 1].second <= segs[i].first, "segments [%llu, %llu) and [%llu, %llu) overlap", (unsigned long long)segs[i - 1].first,
              (unsigned long long)segs[i - 1].second, (unsigned long long)segs[i].first, (unsigned long long)segs[i].second);
}

static u64 checked = 0;

static void run_batch(const Graph& g, const std::vector<std::pair<u32, u32>>& queries, int64_t max_hops, u32 slots_arg) {
    const u32 n = g.m[0].n;
    const u64 count = queries.size();
    const u32 slots = derive_slots(count, n, slots_arg);
    CHECK(slots >= 1 && slots <= SLOTS_MAX && slots <= std::max<u64>(count, 1), "derive_slots(%llu, %u, %u) = %u", (unsigned long long)count, n,
          slots_arg, slots);
    if (slots_arg) CHECK(slots == std::min<u64>(slots_arg, std::max<u64>(count, 1)), "a given slots is kept");
    u64 covered = 0;
    Device dev;
    dev.g = &g;
    dev.n = n;
    dev.word.assign(2 * (size_t)slots, std::vector<u64>(n, ~0ull));
    dev.par.assign(2 * (size_t)slots, std::vector<u32>(n, NONE));
    for (u64 gi = 0; gi < group_count(count, slots); ++gi) {
        u64 first;
        u32 gn;
        group_range(count, slots, gi, &first, &gn);
        CHECK(first == covered && gn >= 1 && gn <= slots, "group %llu starts at %llu with %u queries", (unsigned long long)gi,
              (unsigned long long)first, gn);
        CHECK(gn == slots || first + gn == count, "only the last group is ragged");
        covered += gn;
        Pool pool;
        std::vector<Query> qs(gn);
        std::vector<Seg> segs;
        std::vector<std::pair<u64, u64>> taken;
        dev.ctl.assign(gn, SpCtl{NO_MEET, {0, 0}, {0, 0}, 0, NONE});
        dev.pool.assign(2 * (size_t)gn, 0);
        pool.reserve(2 * (u64)gn);
        taken.push_back({0, 2 * (u64)gn});
        for (u32 j = 0; j < gn; ++j) {
            const u32 s = queries[first + j].first, d = queries[first + j].second;
            seed_query(qs[j], j, s, d);
            dev.pool[2 * j] = s;
            dev.pool[2 * j + 1] = d;
            dev.ctl[j].ent[0] = g.m[0].len(s);
            dev.ctl[j].ent[1] = g.m[1].len(d);
            seed_degrees(qs[j], dev.ctl[j].ent[0], dev.ctl[j].ent[1]);
            if (s == d) continue;
            dev.word[2 * j][s] = 0;
            dev.word[2 * j + 1][d] = 0;
            segs.push_back(Seg{j, 0, 2 * j, 1});
            segs.push_back(Seg{j, 1, 2 * j + 1, 1});
        }
        Round rd;
        for (u32 round = 0;; ++round) {
            CHECK(round <= 2 * n + 4, "the search does not end");
            CHECK(plan_search(qs, max_hops, n, pool, rd), "plan_search refused");
            if (rd.empty()) break;
            dev.pool.resize(pool.used);
            u64 rows = 0, entries = 0;
            std::set<u32> once;
            for (const SpDesc& d : rd.desc) {
                CHECK(once.insert(d.slot).second, "slot %u twice in a round", d.slot);
                CHECK(d.cbase == rows && d.ebase == entries && d.cnt > 0 && d.total > 0, "descriptor prefixes");
                rows += d.cnt;
                entries += d.total;
                CHECK(d.ocap >= std::min<u64>(d.total, n), "slot %u side %u: %u places for %u entries", d.slot, d.side, d.ocap, d.total);
                CHECK((u64)d.obase + d.ocap <= pool.used, "a segment outside the pool");
                taken.push_back({d.obase, (u64)d.obase + d.ocap});
            }
            CHECK(rows == rd.rows && entries == rd.entries && entries <= LAUNCH_ENTRIES_MAX, "round totals");
            for (const SpDesc& d : rd.desc) dev.round(d);
            CHECK(apply_search(qs, rd, dev.ctl.data(), segs), "apply_search saw an overrun");
        }
        disjoint(taken);
        for (u32 j = 0; j < gn; ++j) {
            const Query& q = qs[j];
            CHECK(max_hops == 0 || q.state != LIVE, "query %u never left the search", j);
            const Answer want = contract(g, q.src, q.dst, max_hops);
            std::vector<u32> path;
            if (q.state == FOUND) path = dev.walk(q.slot, q.meetv, q.length, q.src, q.dst);
            CHECK(path == want.path, "query (%u, %u) max_hops %lld: a path of %zu nodes, the contract gives %zu", q.src, q.dst,
                  (long long)max_hops, path.size(), want.path.size());
            if (q.state == FOUND) CHECK(path.size() == (size_t)q.length + 1, "query (%u, %u): length %u, %zu nodes", q.src, q.dst, q.length, path.size());
            u64 st[8];
            fill_stats(q, st);
            if (max_hops == 0) continue;   // (the call returns before any group: the stats are the zeros it wrote)
            for (int k = 0; k < 8; ++k)
                CHECK(st[k] == want.st[k], "query (%u, %u) max_hops %lld: stats[%d] %llu, the contract gives %llu", q.src, q.dst,
                      (long long)max_hops, k, (unsigned long long)st[k], (unsigned long long)want.st[k]);
            ++checked;
        }
        for (const Seg& s : segs)   // the reset: what the segments name is all that was set
            for (u32 i = 0; i < s.cnt; ++i) dev.word[2 * s.slot + s.side][dev.pool[s.base + i]] = ~0ull;
        for (auto& w : dev.word)
            for (u64 x : w) CHECK(x == ~0ull, "a claim word survived the reset");
    }
    CHECK(covered == count, "the groups cover %llu of %llu queries", (unsigned long long)covered, (unsigned long long)count);
}

int main() {
    // derive_slots: claim words and parents of a group stay within 2 GiB
    CHECK(derive_slots(1000, 1u << 20, 0) == 64 && derive_slots(1000, 1u << 22, 0) == 21 && derive_slots(1000, 0xFFFFFFFEu, 0) == 1,
          "derive_slots by vertex count");
    CHECK(derive_slots(5, 100, 0) == 5 && derive_slots(0, 100, 0) == 1 && derive_slots(200, 100, 7) == 7, "derive_slots by query count");

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
    {   // a path with an isolated vertex; a hub between two vertices; the two pinned graphs of the contract; an empty matrix
        std::vector<std::pair<u32, u32>> e;
        for (u32 v = 0; v + 1 < 12; ++v) e.push_back({v, v + 1});
        graphs.push_back(graph_of(13, e));
        e.clear();
        for (u32 v = 1; v <= 30; ++v) { e.push_back({0, v}); e.push_back({v, 31}); e.push_back({v, 0}); }
        graphs.push_back(graph_of(33, e));
        graphs.push_back(graph_of(13, {{0, 1}, {0, 2}, {1, 9}, {2, 3}, {9, 5}, {3, 5}, {5, 10}, {5, 11}, {5, 12}, {10, 8}, {11, 8}, {12, 8}}));
        graphs.push_back(graph_of(6, {{0, 0}, {0, 2}, {0, 3}, {1, 5}, {2, 0}, {2, 4}, {3, 1}, {4, 5}}));
        graphs.push_back(graph_of(5, {}));
    }
    {   // the pinned answers
        const Answer a = contract(graphs[graphs.size() - 3], 0, 8, -1), b = contract(graphs[graphs.size() - 2], 0, 5, -1);
        CHECK((a.path == std::vector<u32>{0, 1, 9, 5, 10, 8}), "parent by frontier position");
        CHECK((b.path == std::vector<u32>{0, 2, 4, 5}), "side by vertex count");
    }
    for (const Graph& g : graphs) {
        const u32 n = g.m[0].n;
        std::vector<std::pair<u32, u32>> all;
        for (u32 s = 0; s < n; ++s)
            for (u32 d = 0; d < n; ++d)
                if (n <= 13 || (s * 7 + d * 3) % 5 == 0 || s == d) all.push_back({s, d});
        for (int64_t mh : {-1, 0, 1, 2, 3, 5})
            for (u32 slots : {0u, 1u, 3u, 7u, 64u}) run_batch(g, all, mh, slots);
    }
    run_batch(graphs[0], {}, -1, 0);
    printf("ok %llu\n", (unsigned long long)checked);
    return 0;
}
