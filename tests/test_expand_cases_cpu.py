"""CPU: tests/expand_cases.py holds what it names.  Every builder's claim (run lengths, segments per frame, where the childless
frames sit, the stretches of empty segments and count-0 items, the k P n values, n_ent, the closed forms of D and E) is proved from
the model alone; the plain reference (trail_rows / edge_rows) equals oracle.model.var_len_expand / expand_row on a shrunken instance
of every family, and tests/trails_check.py's level_expand on A, C and D; the constants in the header are what the sources say; and
for A, C and F a deliberately wrong variant of the PYTHON rule gives another answer on that family's inputs, so the inputs can see
the error (no kernel is altered)."""
import os
import re
import sys
from bisect import bisect_left

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import expand_cases as ec  # noqa: E402
from trails_check import level_expand  # noqa: E402

from oracle import model  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "falkordb_amd", "csrc")
MODEL_DIR = {"out": {}, "in": {"reversed": True}, "both": {"bidirectional": True}}


# ---- the constants ---------------------------------------------------------------------------------------------------------
def test_the_constants_are_the_sources():
    src = {f: open(os.path.join(CSRC, f)).read() for f in ("bulk.hpp", "prims.hip", "sort_plan.hpp", "expand_edges.hip",
                                                           "expand_trails.hip", "edge_layers.hpp")}
    hdr = open(os.path.join(ROOT, "include", "fgpu.h")).read()
    const = lambda text, name: int(re.search(r"constexpr\s+[\w ]+?\b" + name + r"\s*=\s*(\d+)(?:ull|u)?\s*;", text).group(1))
    assert ec.WORD == 64 and "w << 6" in src["bulk.hpp"] and "p >> 6" in src["bulk.hpp"] and "(n + 63) >> 6" in src["bulk.hpp"]
    for f in ("expand_edges.hip", "expand_trails.hip", "bulk.hpp"):
        bounds = set(re.findall(r"__launch_bounds__\((\d+)\)", src[f]))
        assert bounds == {str(ec.BLOCK)}, (f, bounds)
        assert set(re.findall(r"blockIdx\.x \* (\d+) \+ threadIdx\.x", src[f])) == {str(ec.BLOCK)}, f
    assert const(src["prims.hip"], "SCAN_THREADS") * const(src["prims.hip"], "SCAN_SUBTILES") == ec.SCAN_TILE
    assert re.search(r"SCAN_TILE\s*=\s*SCAN_THREADS \* SCAN_SUBTILES;", src["prims.hip"])
    assert const(src["sort_plan.hpp"], "KP_EB") == ec.KP_EB   # (the sorts' shape decisions: transpose.hip takes them from this header)
    assert "(kb + %d) / %d" % (ec.KP_BITS - 1, ec.KP_BITS) in src["sort_plan.hpp"]
    assert "if (kb >= %d && L < 3) L = 3;" % ec.KP_THREE_LEVELS_KB in src["sort_plan.hpp"]
    m = re.search(r"if \(nrp \* n <= \(1ull << (\d+)\)\)", src["expand_edges.hip"])
    assert m and 1 << int(m.group(1)) == ec.ONE_KEY_LIMIT
    assert const(src["edge_layers.hpp"], "EE_MAX_TYPES") == ec.EE_MAX_TYPES
    for f in ("expand_edges.hip", "expand_trails.hip"):       # the packed type word: position in the low six bits, bit 31 = table row
        assert "tyw & %du" % (ec.EE_MAX_TYPES - 1) in src[f] and "tyw |= 0x80000000u" in src[f], f
    assert int(re.search(r"#define FGPU_TRAILS_MAX_DEPTH (\d+)", hdr).group(1)) == ec.TRAILS_MAX_DEPTH
    assert [ec.kp_levels(x) for x in (2, 512, 513, 1 << 16, (1 << 16) + 1, 1 << 17, 1 << 18, (1 << 18) + 1, 1 << 27, (1 << 27) + 1)] == \
        [1, 1, 2, 2, 3, 3, 3, 3, 3, 4]


# ---- what the device walks, from the model alone -------------------------------------------------------------------------
def stored_runs(T, node, half, mt_layers):
    """(m run, dp run) of a (frame, type, half) group: the other nodes of the stored entries, ascending, as the layers are passed
    (mt_layers False: mt_m is the clean transposed structure and there is no mt_dp)"""
    if half == "out":
        return sorted(d for (s, d) in T.m if s == node), sorted(d for (s, d) in T.dp if s == node)
    if mt_layers:
        return sorted(s for (s, d) in T.m if d == node), sorted(s for (s, d) in T.dp if d == node)
    return sorted(s for (s, d) in T.structure() if d == node), []


def trail_segments(g, nodes, types, direction, mt_layers=False):
    """the segment lengths of one level of expand_trails: frame x type x half x layer"""
    scan = ec.scan_of(g, types)
    L = 2 if any(g.tensors[t].dp for t in scan) else 1
    out = []
    for v in nodes:
        for t in scan:
            for half in (("out", "in") if direction == "both" else (direction,)):
                runs = stored_runs(g.tensors[t], v, half, mt_layers)
                out += [len(r) for r in runs[:L]]
    return out


def longest_zero_run(xs, between_populated=False):
    best = cur = 0
    seen = False
    for x in xs:
        if x == 0:
            cur += 1
        else:
            if seen or not between_populated:
                best = max(best, cur)
            cur, seen = 0, True
    return best if between_populated else max(best, cur)


def merged_slots(T, node, half, dp_searches=lambda x: x + 1, m_searches=lambda x: x):
    """et_gather_kernel's slot rule for one group, layers passed as layers: slot = own offset + the rank of the other node in the
    other run.  Returns (slot -> [(layer, other)] claims, [(other, ids)] of the live items in slot order)"""
    mrun, drun = stored_runs(T, node, half, True)
    claims = [[] for _ in range(len(mrun) + len(drun))]
    for at, x in enumerate(mrun):
        claims[at + bisect_left(drun, m_searches(x))].append(("m", x))
    for at, x in enumerate(drun):
        claims[at + bisect_left(mrun, dp_searches(x))].append(("dp", x))
    live = []
    for c in claims:
        for layer, x in c:
            p = (node, x) if half == "out" else (x, node)
            if half == "out":
                valid = layer == "dp" or (p not in T.dp and p not in T.dm)
            else:
                hidden = p in T.dm and p in T.m
                valid = (hidden or p not in T.m) if layer == "dp" else not hidden
            if valid and T.get(*p):
                live.append((x, T.get(*p)))
    return claims, live


# ---- A ---------------------------------------------------------------------------------------------------------------------
def test_a_runs_patterns_and_the_slot_rule():
    g, hubs = ec.layer_merge()
    T = g.tensors[0]
    ix = ec.index_of(T)
    assert g.n == ec.A_N and len(hubs) == len(ec.RUNS) * len(ec.PATTERNS) == 28
    assert sorted({(a, b) for (_, _, a, b, *_) in hubs}) == sorted(ec.RUNS)
    sizes = {a + b for (a, b) in ec.RUNS}
    assert {64, 128, 260} <= sizes and max(sizes) > ec.BLOCK and min(a for a, _ in ec.RUNS) == 0 == min(b for _, b in ec.RUNS)
    multi_m = multi_dp = readded = shadowed = 0
    for (h, mir, a, b, pattern, mn, dn) in hubs:
        for node, half in ((h, "out"), (mir, "in")):
            mrun, drun = stored_runs(T, node, half, True)
            assert (mrun, drun) == (mn, dn) and (len(mrun), len(drun)) == (a, b), (h, pattern)
            pair = (lambda x: (node, x)) if half == "out" else (lambda x: (x, node))
            assert [i for i, x in enumerate(mn) if pair(x) in T.dm] == list(range(3, a, 7))       # every 7th m entry
            multi_m += sum(1 for x in mn if T.eff_get(*pair(x)) == model.MULTI_EDGE and pair(x) not in T.dp)
            multi_dp += sum(1 for x in dn if T.dp[pair(x)] == model.MULTI_EDGE)
            readded += sum(1 for x in dn if pair(x) in T.dm)
            shadowed += sum(1 for x in dn if pair(x) in T.m and pair(x) not in T.dm)
            # the kernel's slot rule gives the reference's adjacency, and every slot is claimed once
            claims, live = merged_slots(T, node, half)
            assert all(len(c) == 1 for c in claims)
            assert live == (ix.out if half == "out" else ix.inn).get(node, [])
            others = [x for c in claims for (_, x) in c]
            assert others == sorted(others)
        both = set(mn) & set(dn)
        if pattern == "interleave":
            assert not both and all(x % 2 != y % 2 for x in mn for y in dn[:1])
        elif pattern == "dp_below":
            assert not both and (not mn or not dn or max(dn) < min(mn))
        elif pattern == "dp_above":
            assert not both and (not mn or not dn or max(mn) < min(dn))
        else:
            assert len(both) == min(a, b) and (a > b or set(mn) <= set(dn))          # a <= b: every m entry is shadowed
    assert multi_m > 0 and multi_dp > 0 and readded > 0 and shadowed > 0
    for j, root in enumerate(ec.A_OPENERS):
        assert len(ix.out.get(root, [])) == len(ix.inn.get(root, [])) == j
    assert all(not ix.inn.get(h[0]) and not ix.out.get(h[1]) for h in hubs)           # the other half of a hub is an empty run
    froms, tos = ec.merge_edge_rows(hubs)
    kinds = {"m": 0, "dp": 0, "shadow": 0, "dead": 0}
    for f, t in zip(froms, tos):
        if f is not None and t is not None:
            p = (f, t)
            kinds["dead" if p in T.dm and p not in T.dp else "shadow" if p in T.dp and p in T.m else "dp" if p in T.dp else "m"] += 1
    assert all(v >= 10 for v in kinds.values()), kinds


def test_a_discrimination_the_merge_order():
    """Three wrong slot rules on the hubs of A.  (1) No merge — the dp run after the m run, the order of the one-layer path: other
    rows.  (2) The dp side searching for `other` instead of `other + 1` while the m side is unchanged: on a shared pair both items
    claim one slot and the next is left unwritten.  (3) Ties placed dp-first consistently (m searching for `other + 1`): the SLOT
    sequence differs on every shared pair; the emitted rows cannot, because of the two items of one pair exactly one has a count —
    which is why the device comparison of family A also runs the hubs where the live item is the m one (the incoming half with
    the transposed layers) and the dp one (the outgoing half)."""
    g, hubs = ec.layer_merge()
    T = g.tensors[0]
    ix = ec.index_of(T)
    seen = {1: 0, 2: 0, 3: 0}
    for (h, mir, a, b, pattern, mn, dn) in hubs:
        right, live = merged_slots(T, h, "out")
        unmerged = [(x, T.get(h, x)) for x in mn if (h, x) not in T.dp and (h, x) not in T.dm] + [(x, T.get(h, x)) for x in dn]
        if [x for x, _ in unmerged] != sorted(x for x, _ in unmerged):
            assert pattern != "dp_above" and unmerged != ix.out[h]
            seen[1] += 1
        wrong, _ = merged_slots(T, h, "out", dp_searches=lambda x: x)
        if set(mn) & set(dn):
            assert any(len(c) == 2 for c in wrong) and any(len(c) == 0 for c in wrong)
            seen[2] += 1
            dp_first, live3 = merged_slots(T, h, "out", dp_searches=lambda x: x, m_searches=lambda x: x + 1)
            assert all(len(c) == 1 for c in dp_first) and dp_first != right and live3 == live
            seen[3] += 1
        else:
            assert wrong == right
    assert seen[1] >= 8 and seen[2] >= 5 and seen[3] >= 5
    # ... and on the rows: the unmerged order changes what expand_trails would emit for level 2
    h = next(x for x in hubs if x[2:5] == (64, 64, "interleave"))
    want = ec.trail_rows(g, h[0], None, ("T",), 1, 2)
    order = {x: i for i, (x, _) in enumerate([(x, None) for x in h[5]] + [(x, None) for x in h[6]])}
    level1 = [r for r in want if len(r[2]) == 3]
    assert [r[1] for r in level1] != sorted((r[1] for r in level1), key=order.get)


# ---- B ---------------------------------------------------------------------------------------------------------------------
def test_b_types_segments_and_empty_stretches():
    g = ec.many_types()
    assert len(g.tensors) == ec.EE_MAX_TYPES == 64 and len(ec.B_TYPES) == 64
    assert [t for t, T in enumerate(g.tensors) if T.structure()] == list(ec.B_HELD) == [0, 31, 63]
    assert [t for t, T in enumerate(g.tensors) if T.dp] == [31]
    last, first = g.tensors[63], g.tensors[0]
    assert any(v == model.MULTI_EDGE for v in last.m.values()) and set(last.m) & set(first.m)       # first-only scans 63 types
    rows = ec.many_types_rows()
    populated = {v for T in g.tensors for p in T.structure() for v in p}
    assert len(rows) == ec.B_ROWS == 300 and [i for i, v in enumerate(rows) if v in populated] == list(range(0, 300, ec.B_EVERY))
    for order in (ec.B_TYPES, ec.B_TYPES[::-1]):
        for mt_layers in (False, True):
            seg = trail_segments(g, rows, order, "both", mt_layers)
            per_frame = len(seg) // len(rows)
            assert per_frame == 64 * 2 * 2 == ec.BLOCK and len(seg) > ec.BLOCK
            assert longest_zero_run(seg[:per_frame], between_populated=True) >= ec.WORD         # inside one frame
            assert longest_zero_run(seg) >= 49 * per_frame
        for direction in ("out", "in"):
            seg = trail_segments(g, rows[:1], order, direction)
            assert len(seg) == 128 and longest_zero_run(seg, between_populated=True) >= 59
    # the type position survives the packed word at 63: the reference's type column reaches it on a multi-edge pair
    want = ec.edge_columns(g, rows, [None] * len(rows), types=ec.B_TYPES)
    sizes = np.bincount(want[want[:, 5] == 63][:, 2].astype(np.int64))
    assert want[:, 5].max() == 63 and sizes[43] == 3 * 6
    t = ec.tombstones()
    T = t.tensors[0]
    assert [(0, 100 + i) in T.dm for i in range(ec.TOMB_RUN + 1)] == [True] * ec.TOMB_RUN + [False] and ec.TOMB_RUN >= 2 * ec.WORD
    assert [(100 + i, 1) in T.dm for i in range(ec.TOMB_RUN + 1)] == [True] * ec.TOMB_RUN + [False]
    assert stored_runs(T, 0, "out", True)[0] == list(range(100, 101 + ec.TOMB_RUN)) == stored_runs(T, 1, "in", True)[0]
    assert ec.index_of(T).out[0] == [(100 + ec.TOMB_RUN, T.get(0, 100 + ec.TOMB_RUN))]


# ---- C ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tree():
    return ec.irregular_tree()


def test_c_childless_frames_sit_at_the_tile_edges(tree):
    g, sizes, (c1, c2) = tree
    assert sizes == (1, 9000, 18000, 18000) and g.n == 45001
    assert sorted(np.bincount(c1).tolist()) == [1800] * 5 and sorted(np.bincount(c2).tolist()) == [6000] * 3     # j % 5 and g % 3
    ix = ec.index_of(g.tensors[0])
    for first, counts in ((1, c1), (1 + sizes[1], c2)):
        assert [len(ix.out.get(first + p, [])) for p in range(len(counts))] == counts                           # position = id - first
        edge = (0, 255, 256, 4095, 4096, len(counts) - 1)
        assert [counts[p] for p in edge] == [0] * 6
        assert all(counts[p - 1] or counts[p + 1] for p in edge[1:5])                                          # with neighbours that have some
    assert 4095 == ec.SCAN_TILE - 1 and 255 == ec.BLOCK - 1
    want, c = ec.trail_columns(g, [0], types=("T",), lo=1, hi=3)
    assert len(want[0]) == 45000 <= 120000 and c["frames"] == 27001
    assert len(ec.trail_columns(g, [0], types=("T",), lo=0, hi=3)[0][0]) == 45001
    assert np.array_equal(np.bincount(want[3])[1:], sizes[1:])


def test_c_many_roots_interleave_zero_hop_rows():
    g = ec.many_roots_graph()
    K = ec.labelled(g, ("K",))
    assert ec.MANY_ROOTS == (4095, 4096, 4097)
    for k in ec.MANY_ROOTS:
        starts, dests = ec.many_roots(k)
        assert [i for i, s in enumerate(starts) if s not in K] == list(range(4, k, 5))
        assert [i for i, d in enumerate(dests) if d is not None] == list(range(0, k, 3)) and all(d in (None, s) for s, d in zip(starts, dests))
        want, _ = ec.trail_columns(g, starts, dests, types=("T",), lo=0, hi=2, bitmap_nodes=K)
        zero = want[0][want[3] == 0]
        assert np.array_equal(zero, [i for i in range(k) if i % 5 != 4])
        walked = np.unique(want[0][want[3] > 0])
        assert len(walked) > k // 2 and len(want[0]) > k


# ---- D and E ---------------------------------------------------------------------------------------------------------------
def test_d_closed_forms():
    assert ec.trails_between_two(4) == 4 + 12 + 24 + 24 == 64
    for s in (0, 1):
        assert len(ec.trail_rows(ec.parallel_pair(4), s, None, ("T",), 1, None, "both")) == 64
    ring = ec.parallel_ring(3, 3)
    assert ec.RING_TRAILS == 93
    for direction in ("out", "in"):
        assert [len(ec.trail_rows(ring, s, None, ("T",), 1, 4, direction)) for s in range(3)] == [93] * 3
    lists = ec.id_lists()
    assert [len(v) for v in lists.tensors[0].me.values()] == list(ec.LISTS) == [63, 64, 65, 129]
    c = {}
    rows = ec.trail_rows(lists, 0, None, ("T",), 1, 2, "both", counters=c)
    assert len(rows) == 321 + sum(L * (L - 1) for L in ec.LISTS) == 321 + 28610 and c["used"] == 321
    # a list boundary on a candidate-word edge: the candidates of level 0 are the lists back to back
    assert np.cumsum(ec.LISTS).tolist() == [63, 127, 192, 321] and 63 == ec.WORD - 1 and 192 == 3 * ec.WORD


def test_e_held_after_every_depth():
    g = ec.budget_tree()
    assert g.n == 1 + 3 + 9 + 27 + 81
    for k in (1, 2):
        assert [ec.held_after(d, k=k) for d in range(ec.E_DEPTH)] == [k * x for x in (1 + 6, 1 + 6 + 18, 1 + 6 + 18 + 54, 1 + 6 + 18 + 54 + 81)]
        for d in range(ec.E_DEPTH):
            c = {}
            rows = ec.trail_columns(g, [0] * k, types=("T",), lo=1, hi=min(d + 2, ec.E_DEPTH))[0]
            ec.trail_rows(g, 0, None, ("T",), 1, min(d + 2, ec.E_DEPTH), counters=c)
            assert ec.held_after(d, k=k) == k * c["frames"] + int((rows[3] <= d + 1).sum())


# ---- F ---------------------------------------------------------------------------------------------------------------------
def test_f_key_spaces_and_entry_counts():
    cases = ec.key_space_cases()
    keys = [k * (2 if bidir else 1) * n for (_, n, k, bidir, _, _) in cases]
    n_of = {c[0]: c[1] for c in cases}
    assert keys == [2**9, 2**9 + n_of["2^9+n"], 2**16, 2**16 + n_of["2^16+n"], 2**17 - n_of["2^17-n"], 2**17, 2**22, 2**22 + n_of["2^22+n"]]
    assert [c[4] for c in cases] == [1] * 7 + [2] and [c[5] for c in cases] == [1, 2, 2, 3, 3, 3, 3, 2]
    assert cases[6][1:3] == (cases[7][1], cases[7][2] - 1) and ec.key_space_rows(1024, 4097)[:4096] == ec.key_space_rows(1024, 4096)
    for n in (64, 1024):
        g = ec.sort_graph(n)
        held = {}
        for t, T in enumerate(g.tensors):
            for p in T.structure():
                held.setdefault(p, []).append(t)
        assert sum(len(v) >= 2 for v in held.values()) > len(held) // 2 and any(len(v) == 3 for v in held.values())
        assert g.tensors[1].dp and all(T.me for T in g.tensors)
        rows = ec.key_space_rows(n, 2 * n)
        assert set(rows) == set(range(n)) and all(a != b for a, b in zip(rows, rows[1:]))
    assert list(ec.F_TYPES) != sorted(ec.F_TYPES)
    for n_ent in ec.STABLE_ENT:
        g = ec.stable_graph(n_ent)
        assert g.n == 1 << 20 and len(ec.STABLE_ROWS) * g.n > ec.ONE_KEY_LIMIT
        per_type = [sum(1 for (s, _) in T.m if s == ec.STABLE_HUB) for T in g.tensors]
        assert sum(per_type) == n_ent and per_type[1] == per_type[2] == n_ent // 3 and per_type[0] == n_ent // 3 + n_ent % 3
        assert all(len(T.m) == c for T, c in zip(g.tensors, per_type))                                         # nothing but the hub row
    assert [x - ec.KP_EB for x in ec.STABLE_ENT[:3]] == [-1, 0, 1] and ec.STABLE_ENT[3] == 2 * ec.KP_EB + 1


def test_f_discrimination_an_unstable_second_sort():
    """ties of (row, pass, other node) in descending type position: what a second sort that does not keep the first one's order
    could give"""
    for n_ent in ec.STABLE_ENT[:4]:
        g = ec.stable_graph(n_ent)
        assert ec.edge_rows(g, ec.STABLE_HUB, None, ec.F_TYPES) != ec.edge_rows(g, ec.STABLE_HUB, None, ec.F_TYPES, _types="descending")
    for (_, n, k, bidir, _, _) in ec.key_space_cases()[:6]:
        g = ec.sort_graph(n)
        rows = ec.key_space_rows(n, k)
        right = ec.edge_columns(g, rows, [None] * k, types=ec.F_TYPES, bidirectional=bidir)
        wrong = ec.edge_columns(g, rows, [None] * k, types=ec.F_TYPES, bidirectional=bidir, _types="descending")
        assert right.shape == wrong.shape and (right != wrong).any()


def test_c_discrimination_the_sibling_order(tree):
    """siblings' subtrees in forward instead of reverse order"""
    g = tree[0]
    for lo, hi in ((1, 3), (2, 3), (3, 3), (1, 2), (0, 3)):
        right = ec.trail_rows(g, 0, None, ("T",), lo, hi)
        wrong = ec.trail_rows(g, 0, None, ("T",), lo, hi, _siblings="forward")
        assert sorted(map(str, right)) == sorted(map(str, wrong)) and right != wrong
    mr = ec.many_roots_graph()
    assert ec.trail_rows(mr, 0, None, ("T",), 0, 2) != ec.trail_rows(mr, 0, None, ("T",), 0, 2, _siblings="forward")


# ---- G ---------------------------------------------------------------------------------------------------------------------
def test_g_deciding_bits_and_dirty_words():
    assert ec.G_SIZES == (63, 64, 65, 127, 128, 129)
    for n in ec.G_SIZES:
        g, special = ec.word_edge_graph(n)
        assert special == sorted({v for v in (0, 1, 62, 63, 64, n - 2, n - 1) if v < n}) and (n - 1) // 64 == (n + 63) // 64 - 1
        F, Q = ec.labelled(g, ("F",)), ec.labelled(g, ("Q",))
        assert F == {v for v in (n - 1, 63) if v < n} and Q == {v for v in (n - 1, 64, 0) if v < n}
        assert set(special) - F and set(special) - Q                                                            # the bitmaps decide
        words = np.zeros((n + 63) // 64, dtype=np.uint64)
        for v in F:
            words[v >> 6] |= np.uint64(1) << np.uint64(v & 63)
        dirty = ec.dirty_bits(words, n)
        bits = lambda w: [int(w[v >> 6]) >> (v & 63) & 1 for v in range(64 * len(w))]
        assert bits(dirty)[:n] == bits(words)[:n] and all(bits(dirty)[n:]) and (n % 64 == 0) == np.array_equal(dirty, words)
        # the label decides rows in both calls
        assert ec.edge_columns(g, special, [None] * len(special), types=("T",), from_nodes=F).shape[0] < \
            ec.edge_columns(g, special, [None] * len(special), types=("T",)).shape[0]
        zero = [r for s in special for r in ec.trail_rows(g, s, None, ("T",), 0, 1, bitmap_nodes=F) if len(r[2]) == 1]
        assert [r[0] for r in zero] == sorted(F)


# ---- the reference against the model ----------------------------------------------------------------------------------------
def same_trails(g, starts, dests=(None,), types=(), hops=((1, 2),), labels=(), levelled=False):
    n = 0
    for direction in ec.DIRECTIONS:
        for s in starts:
            for d in dests:
                for lo, hi in hops:
                    got = ec.trail_rows(g, s, d, types, lo, hi, direction, ec.labelled(g, labels))
                    kw = dict(dest=d, min_hops=lo, max_hops=hi, dst_labels=labels, emit_path=True, **MODEL_DIR[direction])
                    assert got == model.var_len_expand(g, s, list(types), **kw), (direction, s, d, lo, hi)
                    if levelled:
                        assert got == level_expand(g, s, list(types), **kw), (direction, s, d, lo, hi)
                    n += len(got)
    return n


def same_edges(g, froms, tos, types=(), from_labels=(), to_labels=()):
    n = 0
    for transposed in (False, True):
        for bidir in (False, True):
            for first in (False, True):
                for f, t in zip(froms, tos):
                    got = ec.edge_rows(g, f, t, types, transposed, bidir, first, ec.labelled(g, from_labels), ec.labelled(g, to_labels))
                    want = model.expand_row(g, f, t, list(types), from_labels, to_labels, transposed, bidir, emit_relationship=not first)
                    assert got == want, (transposed, bidir, first, f, t)
                    n += len(got)
    return n


def test_reference_equals_the_model_a():
    g, hubs = ec.layer_merge_small()
    assert 100 < len(g.tensors[0].m) + len(g.tensors[0].dp) < 400
    nodes = [h[0] for h in hubs] + [h[1] for h in hubs]
    assert same_trails(g, nodes, types=("T",), hops=((1, 2), (0, 1)), levelled=True) > 1000
    froms, tos = ec.merge_edge_rows(hubs)
    assert same_edges(g, froms, tos, ("T",)) > 1000


def test_reference_equals_the_model_b():
    g = ec.many_types(ntypes=8, held=(0, 3, 7))
    names = tuple("T%02d" % t for t in range(8))
    rows = ec.many_types_rows(20, 5)
    for order in (names, names[::-1]):
        assert same_trails(g, rows, (None, 40), order) > 100
        assert same_edges(g, rows + [None] * 20, [None] * 20 + rows, order) > 100
    t = ec.tombstones(run=9, n=40)
    assert same_trails(t, [0, 1, 2, 3, 109], types=("T",), hops=((1, 3),), levelled=True) > 10
    assert same_edges(t, [0, None, 109, 0, 100], [None, 1, None, 109, 1], ("T",)) > 10


def test_reference_equals_the_model_c():
    g, sizes, _ = ec.irregular_tree(children=40)
    assert 150 < len(g.tensors[0].m) < 400
    leaf = g.n - 1
    for labels in ((), ("K",)):
        assert same_trails(g, [0, 5, leaf], (None, leaf, 1 + sizes[1]), ("T",), ((1, 3), (2, 3), (3, 3), (1, 2), (0, 3)), labels, True) > 200
    mr = ec.many_roots_graph()
    assert same_trails(mr, range(12), (None, 0, 3), ("T",), ((0, 2), (0, 0)), ("K",), True) > 100


def test_reference_equals_the_model_d_and_e():
    assert same_trails(ec.parallel_pair(4), [0, 1], (None, 0), ("T",), ((1, None), (0, 3)), levelled=True) > 128
    assert same_trails(ec.parallel_ring(3, 3), [0, 1, 2], (None, 1), ("T",), ((1, 4), (0, 2)), levelled=True) > 500
    assert same_trails(ec.id_lists((3, 4, 5)), range(4), (None,), ("T",), ((1, 2), (1, 3)), levelled=True) > 100
    assert same_trails(ec.budget_tree(2, 3), [0, 1, 14], (None,), ("T",), ((1, 3), (1, 1), (2, 2))) > 20


def test_reference_equals_the_model_f_and_g():
    g = ec.sort_graph(24)
    assert 100 < sum(len(T.m) + len(T.dp) for T in g.tensors) < 400
    nodes = list(range(24))
    for types in (ec.F_TYPES, ("B", "A"), ()):
        assert same_edges(g, nodes + [None] * 24 + nodes, [None] * 24 + nodes + nodes[::-1], types) > 300
    assert same_trails(g, nodes[:6], (None,), ec.F_TYPES, ((1, 2),)) > 50
    s = ec.stable_graph(11, n=2000)
    assert same_edges(s, list(ec.STABLE_ROWS) + [None], [None] * 5 + [1000], ec.F_TYPES) > 20
    for n in ec.G_SIZES:
        g, special = ec.word_edge_graph(n)
        none = [None] * len(special)
        assert same_edges(g, special + none, none + special, ("T",), ("F",), ("Q",)) > 0
        assert same_edges(g, special, none, ("T",), (), ("Q",)) > 0
        assert same_trails(g, special, (None, n - 1), ("T",), ((0, 2),), ("F",)) > 10
