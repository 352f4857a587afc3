"""The references of tests/bfs_cases.py agree with the C oracle, and its case builders hold what the GPU tests of
tests/test_gpu_bfs_edges.py rely on — every property recomputed here from the edge lists (no GPU needed).  The last test
reads the kernel sources: a retuned threshold fails here, with the case to rebuild, instead of a GPU case that silently
stops reaching its branch."""
import os
import re
import sys

import numpy as np
import pytest

import oracle

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bfs_cases as bc  # noqa: E402

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "falkordb_amd", "csrc")
U64 = np.uint64


def all_cases():
    out = [(f"ragged{n}", bc.ragged_random(n)) for n in bc.RAGGED_SIZES]
    out += [("heavy_push", bc.heavy_push()), ("pull_ladder", bc.pull_ladder()), ("push_ladder", bc.push_ladder())]
    out += [(f"fan{v}x{p}", bc.fan(v, p)) for v, p in bc.FANS]
    out += [(f"pull_gate{m}", bc.pull_gate(m)) for m in bc.PULL_GATES]
    out += list(bc.degenerate().items())
    return out


CASES = all_cases()
IDS = [name for name, _ in CASES]


def orc(n, rows, cols):
    return oracle.build_csr(n, n, np.asarray(rows, dtype=U64), np.asarray(cols, dtype=U64))


def three_sources(n, named):
    return (named["sources"] + [n // 2, 0, n - 1])[:3]


@pytest.mark.parametrize("case", [c for _, c in CASES], ids=IDS)
def test_bfs_levels_equal_the_oracle(case):
    n, rows, cols, named = case
    a = orc(n, rows, cols)
    assert a.nnz == len(rows)                                              # the builders hand out unique edges
    rp, ci = bc.csr(n, rows, cols)
    np.testing.assert_array_equal(rp, a.rowptr.astype(np.int64))
    np.testing.assert_array_equal(ci, a.colidx.astype(np.int64))
    for src in three_sources(n, named):
        for max_level in (-1, 0, 1, 2):
            want, want_parent, want_edges = oracle.bfs(a, src, max_level)
            level, edges = bc.bfs_levels(n, rows, cols, src, max_level)
            np.testing.assert_array_equal(level, want)
            assert edges == want_edges
            assert level.dtype == np.int32
            bc.check_parents(n, rows, cols, src, level, want_parent)       # the oracle's parents pass the parent check
            assert 0 <= bc.level_steps(level, max_level) <= (max_level if max_level >= 0 else n)
    # ... and the parent check refuses a parent two levels up, a parent without the edge and a parent of an unreached vertex
    src = named["sources"][0]
    level, parent, _ = oracle.bfs(a, src, -1)
    deep = np.nonzero(level >= 2)[0]
    if len(deep):
        bad = parent.copy()
        bad[deep[0]] = src
        with pytest.raises(AssertionError):
            bc.check_parents(n, rows, cols, src, level, bad)
    if (level < 0).any():
        bad = parent.copy()
        bad[np.nonzero(level < 0)[0][0]] = src
        with pytest.raises(AssertionError):
            bc.check_parents(n, rows, cols, src, level, bad)


def frontiers(n, named, rng):
    full = np.arange(n)
    return {"empty": [], "last": [n - 1], "all": full, "half": rng.choice(n, (n + 1) // 2, replace=False)}


@pytest.mark.parametrize("case", [c for _, c in CASES], ids=IDS)
def test_vxm_bits_equal_the_oracle(case):
    n, rows, cols, named = case
    a = orc(n, rows, cols)
    rng = np.random.default_rng(n)
    mask = bc.bits_of(n, rng.choice(n, n // 3, replace=False))
    for name, ids in frontiers(n, named, rng).items():
        f = bc.bits_of(n, ids)
        np.testing.assert_array_equal(f, oracle.bits_from_ids(n, ids))
        np.testing.assert_array_equal(bc.ids_of(f, n), np.sort(np.asarray(ids, dtype=np.int64)))
        for mk in (None, mask, bc.bits_of(n, np.arange(n))):
            got = bc.vxm_bits(n, rows, cols, f, mk)
            np.testing.assert_array_equal(got, oracle.vxm(a, f, mk), err_msg=name)
            assert got.dtype == U64 and len(got) == (n + 63) // 64
            assert not np.unpackbits(got.view(np.uint8), bitorder="little")[n:].any()


def test_references_equal_the_oracle_on_rmat10():
    a = oracle.rmat_csr(10)
    n = a.nrows
    r, c = a.pairs()
    rows, cols = r.astype(np.int64), c.astype(np.int64)
    deg = np.diff(a.rowptr.astype(np.int64))
    for src in (int(np.argmax(deg)), int(np.nonzero(deg > 0)[0][0]), n - 1):
        for max_level in (-1, 0, 1, 2):
            want, _, want_edges = oracle.bfs(a, src, max_level)
            level, edges = bc.bfs_levels(n, rows, cols, src, max_level)
            np.testing.assert_array_equal(level, want)
            assert edges == want_edges
    rng = np.random.default_rng(10)
    mask = bc.bits_of(n, rng.choice(n, n // 3, replace=False))
    for ids in ([], np.arange(n), rng.choice(n, 300, replace=False)):
        for mk in (None, mask):
            f = bc.bits_of(n, ids)
            np.testing.assert_array_equal(bc.vxm_bits(n, rows, cols, f, mk), oracle.vxm(a, f, mk))


# ---- what the GPU tests rely on ---------------------------------------------------------------------------------------

def degrees(n, rows, cols):
    return np.bincount(rows, minlength=n), np.bincount(cols, minlength=n)


def frontier_edges(n, rows, level, k):
    """(vertices, out-edges) of the level-k frontier: the m_frontier the control step sees before that level's push."""
    out, _ = degrees(n, rows, rows)
    f = level == k
    return int(f.sum()), int(out[f].sum())


def test_degenerate_graphs_are_the_four_small_ones():
    shapes = {name: (n, list(zip(rows.tolist(), cols.tolist()))) for name, (n, rows, cols, _) in bc.degenerate().items()}
    assert shapes == {"n1_empty": (1, []), "n1_self_loop": (1, [(0, 0)]), "n2_one_edge": (2, [(0, 1)]), "n65_empty": (65, [])}
    assert all(n > 3 for n in bc.RAGGED_FULL) and set(bc.RAGGED_SIZES) - set(bc.RAGGED_FULL) == {1, 2, 3}


@pytest.mark.parametrize("n", bc.RAGGED_FULL)
def test_ragged_random_has_the_edges_it_names(n):
    n_, rows, cols, named = bc.ragged_random(n)
    assert n_ == n and rows.max() < n and cols.max() < n
    assert 2.5 * n <= len(rows) <= 3 * n + 7
    out, ind = degrees(n, rows, cols)
    edges = set(zip(rows.tolist(), cols.tolist()))
    s = named["self_loop"]
    p, q = named["two_cycle"]
    assert (s, s) in edges and (p, q) in edges and (q, p) in edges
    assert ind[named["no_in"]] == 0 and out[named["no_in"]] > 0
    assert out[named["no_out"]] == 0
    assert ind[n - 1] >= 1 and any(c == n - 1 and r != n - 1 for r, c in edges)
    w = named["only_via_last"]
    assert ind[w] == 1 and (n - 1, w) in edges
    assert not bc.coo_is_hyper(n, rows)
    # the searches in the order the GPU tests run them: a wide one, one that ends at its source, a wide one again; the
    # first one reaches n - 1 and, through it, the vertex nothing else points at; a vertex stays unreached
    reached = [int((bc.bfs_levels(n, rows, cols, src)[0] >= 0).sum()) for src in named["sources"]]
    assert named["sources"] == [0, named["no_out"], n - 1]
    assert reached[0] > reached[1] == 1 and reached[2] > n // 2
    level0 = bc.bfs_levels(n, rows, cols, 0)[0]
    assert level0[n - 1] >= 1 and level0[w] == level0[n - 1] + 1 and level0[named["no_in"]] == -1
    if n > 64:
        assert level0.max() >= 3                                           # max_level = 2 cuts the search


def test_heavy_push_has_a_live_ragged_quad_behind_a_level_that_does_not_append():
    n, rows, cols, named = bc.heavy_push()
    assert n == 1203 and n % 4 == 3 and n % 64 != 0 and len(rows) == 161_258
    out, _ = degrees(n, rows, cols)
    level, _ = bc.bfs_levels(n, rows, cols, 0)
    for k, name in ((1, "L1"), (2, "L2")):
        np.testing.assert_array_equal(np.nonzero(level == k)[0], named[name])
    assert frontier_edges(n, rows, level, 0) == (1, 400) and 400 <= bc.QGATE                 # level 1 appends: queue mode
    assert frontier_edges(n, rows, level, 1) == (400, 160_000) and 160_000 > bc.QGATE        # level 2 does not
    assert frontier_edges(n, rows, level, 2) == (400, 800)                                   # ... so level 3 walks the bitmap
    assert (level == 3).sum() == 400 and bc.level_steps(level) == 4
    # the last quad, v0 = 1200, is ragged (n - v0 = 3 < 4) and every vertex of it is in the level-2 frontier with an edge
    # to a level-3 vertex
    v0 = n - n % 4
    assert v0 == 1200 and v0 + 4 > n
    edges = set(zip(rows.tolist(), cols.tolist()))
    for v in range(n - 3, n):
        assert level[v] == 2 and any(level[c] == 3 for r, c in edges if r == v)
    # the last 64-vertex window of a blocked push is ragged and receives discoveries at level 2 (fused launch 1)
    w0 = n - n % 64
    assert w0 == 1152 and (level[w0:] == 2).all()
    assert 400 <= bc.TINY_EDGES                                            # level 1 is the tiny kernel's under bfs_tiny = 1
    reached = [int((bc.bfs_levels(n, rows, cols, s)[0] >= 0).sum()) for s in named["sources"]]
    assert reached[0] > reached[1] > reached[2] == 1 and reached[0] < n
    assert not bc.coo_is_hyper(n, rows)


def pull_order(n, rows, cols, v):
    """Row v of A' as a pull level reads it with bfs_hub_first = 1 (ensure_pull_order: descending out-degree class
    floor(log2(outdeg + 1)), ids ascending inside a class; rows of HUB_DEG entries and more keep the ascending order)."""
    out, _ = degrees(n, rows, cols)
    nb = np.sort(rows[cols == v])
    if len(nb) >= bc.HUB_DEG:
        return nb
    cls = np.floor(np.log2(out[nb] + 1)).astype(np.int64)
    return nb[np.lexsort((nb, -cls))]


def test_pull_ladder_puts_the_only_frontier_in_neighbour_last_in_every_row():
    n, rows, cols, named = bc.pull_ladder()
    x, u, t = named["x"], named["u"], named["t"]
    assert n == 4133 and n % 64 == 37 and len(rows) == 12_608
    out, ind = degrees(n, rows, cols)
    level, _ = bc.bfs_levels(n, rows, cols, 0)
    assert (level[named["decoys"]] == -1).all() and (ind[named["decoys"]] == 0).all() and len(named["decoys"]) == 4096
    for d in bc.PULL_DEGS:
        nb = np.sort(rows[cols == t[d]])
        assert ind[t[d]] == d == len(nb)
        assert nb[-1] == x[d] and x[d] > named["decoys"].max()             # last in ascending order ...
        assert pull_order(n, rows, cols, t[d])[-1] == x[d]                 # ... and in the hub-first order
        assert [int(v) for v in nb if level[v] >= 0] == [x[d]]             # the only reached one: the parent is forced
        assert level[x[d]] == 1 and level[t[d]] == 2 and level[u[d]] == 3
        assert rows[cols == u[d]].tolist() == [t[d]] and rows[cols == x[d]].tolist() == [0]
    assert bc.level_steps(level) == 4
    # the row of t_3 is the last of A' and ends it: its 16-byte read of entries 2 .. 5 would overrun (the `tail` path)
    assert t[3] == n - 1
    at_rowptr = np.concatenate([[0], np.cumsum(ind)])
    assert ind[n - 1] == 3 and at_rowptr[n - 1] + bc.PULL_H + 4 > at_rowptr[n] == len(rows)
    assert np.nonzero(ind)[0][-1] == n - 1
    # the other rows read past their head: the 16-byte read stays inside the array
    assert all(at_rowptr[t[d]] + bc.PULL_H + 4 <= len(rows) for d in bc.PULL_DEGS if d not in (1, 3))
    # which phase finds x_d: the head (1), A2 = entries PULL_H + 1 .. PULL_H + 4 (2, 3, 5), phase B past them in 64-entry
    # trips (6, 7: one short trip; 69: exactly one; 70, 133: two), the hub section (>= HUB_DEG)
    assert bc.PULL_H == 1
    phase = {d: ("head" if d <= bc.PULL_H else "A2" if d <= bc.PULL_H + 4 else "hub" if d >= bc.HUB_DEG else
                 f"B{-(-(d - bc.PULL_H - 4) // 64)}") for d in bc.PULL_DEGS}
    assert phase == {1: "head", 2: "A2", 3: "A2", 5: "A2", 6: "B1", 7: "B1", 69: "B1", 70: "B2", 133: "B2", 4095: "B64",
                     4096: "hub", 4097: "hub"}
    # hub rows and ordinary rows share one 64-bit word of the bitmaps, and one trip of PULL_R words
    words = {d: t[d] // 64 for d in bc.PULL_DEGS}
    assert len(set(words.values())) == 1
    assert any(d >= bc.HUB_DEG for d in bc.PULL_DEGS) and any(d < bc.HUB_DEG for d in bc.PULL_DEGS)
    assert (ind > 0).sum() == 3 * len(bc.PULL_DEGS)
    assert not bc.coo_is_hyper(n, rows)
    assert bc.coo_is_hyper(n, cols)              # (the transpose is built on the device from the dense A, never from a COO list)
    reached = [int((bc.bfs_levels(n, rows, cols, s)[0] >= 0).sum()) for s in named["sources"]]
    assert reached == [1 + 3 * len(bc.PULL_DEGS), 3, 1]


def test_push_ladder_has_the_out_degrees_it_names():
    n, rows, cols, named = bc.push_ladder()
    assert n % 64 != 0 and n % 4 != 0
    out, ind = degrees(n, rows, cols)
    assert [int(out[named["h"][d]]) for d in bc.PUSH_DEGS] == list(bc.PUSH_DEGS)
    assert out[0] == len(bc.PUSH_DEGS)
    for d in bc.PUSH_DEGS:
        assert np.isin(cols[rows == named["h"][d]], named["pool"]).all()
    assert bc.PUSH_HUB_DEG - 1 in bc.PUSH_DEGS and bc.PUSH_HUB_DEG in bc.PUSH_DEGS and bc.PUSH_HUB_DEG + 1 in bc.PUSH_DEGS
    assert 2 * bc.PUSH_HUB_CHUNK + 1 in bc.PUSH_DEGS                       # a chunk of one edge
    assert bc.HUB_DEG - 1 in bc.PUSH_DEGS and bc.HUB_DEG in bc.PUSH_DEGS and bc.HUB_DEG + 1 in bc.PUSH_DEGS
    assert 4800 <= len(named["pool"]) <= 5200
    assert (ind[named["pool"]] >= 2).sum() > 1000                          # overlapping ranges: duplicate discoveries
    # a pool target that an ordinary row (1023 edges) and a hub row both point at
    small, big = cols[rows == named["h"][1023]], cols[rows == named["h"][1024]]
    assert len(np.intersect1d(small, big)) > 0
    pool_out = out[named["pool"]]
    np.testing.assert_array_equal(np.nonzero(pool_out)[0], np.arange(0, len(named["pool"]), 97))
    assert pool_out.max() == 1
    level, _ = bc.bfs_levels(n, rows, cols, 0)
    assert frontier_edges(n, rows, level, 1) == (7, sum(bc.PUSH_DEGS)) and sum(bc.PUSH_DEGS) <= bc.QGATE   # queue mode
    assert bc.level_steps(level) == 4
    # mat_from_coo would store this adjacency hypersparse, which a plan refuses: the GPU tests upload its CSR
    assert bc.coo_is_hyper(n, rows)
    reached = [int((bc.bfs_levels(n, rows, cols, s)[0] >= 0).sum()) for s in named["sources"]]
    assert reached[0] > reached[1] > reached[2] > reached[3] == 2


@pytest.mark.parametrize("verts,per", bc.FANS)
def test_fan_levels_sit_at_and_past_the_tiny_thresholds(verts, per):
    n, rows, cols, named = bc.fan(verts, per)
    level, _ = bc.bfs_levels(n, rows, cols, 0)
    assert frontier_edges(n, rows, level, 0) == (1, 32)
    assert frontier_edges(n, rows, level, 1) == (32, verts)
    assert frontier_edges(n, rows, level, 2) == (verts, verts * per)
    np.testing.assert_array_equal(np.nonzero(level == 2)[0], named["layer"])
    tiny = verts <= bc.TINY_VERTS and verts * per <= bc.TINY_EDGES
    assert tiny == ((verts, per) == (1024, 4))
    if (verts, per) == (1024, 4):
        assert verts == bc.TINY_VERTS and verts * per == bc.TINY_EDGES     # exactly at both
    if (verts, per) == (1025, 4):
        assert verts == bc.TINY_VERTS + 1
    if (verts, per) == (1024, 5):
        assert verts * per == bc.TINY_EDGES + bc.TINY_VERTS                # one more edge per vertex
    assert verts * per <= bc.QGATE and bc.level_steps(level) == 5
    assert not bc.coo_is_hyper(n, rows)
    reached = [int((bc.bfs_levels(n, rows, cols, s)[0] >= 0).sum()) for s in named["sources"]]
    assert reached[0] == n and reached[0] > reached[1] > reached[2]


@pytest.mark.parametrize("m", bc.PULL_GATES)
def test_pull_gate_sits_at_and_past_the_append_bound_of_a_pull_level(m):
    n, rows, cols, named = bc.pull_gate(m)
    out, ind = degrees(n, rows, cols)
    level, _ = bc.bfs_levels(n, rows, cols, 0)
    dec = named["decoys"]
    assert (out[dec] == 0).all() and (ind[dec] == 0).all() and (level[dec] == -1).all() and n % 64 != 0
    assert level[named["a"]] == 1 and (level[named["F"]] == 2).all() and level[named["R"][0]] == 3
    assert (level[named["R"]] >= 3).all()
    n_alive, nnz = int((ind > 0).sum()), len(rows)
    assert n_alive == 1 + m + len(named["R"]) == n - 1 - len(dec)
    # The control step after level 1 (reached = 2) opens the queue for level 2, a pull, when at most QGATE vertices are
    # unvisited — the decoys alone are more — or when at most PULL_QGATE of the unvisited ones have an in-edge
    # (n_alive + 1 - reached; never, with bfs_alive_rule = 0): only the second bound decides, and it is met exactly or missed by one
    reached = 2
    unv, alive_unv = n - reached, n_alive + 1 - reached
    assert unv > bc.QGATE and len(dec) > bc.QGATE
    assert alive_unv == m + len(named["R"]) == bc.PULL_QGATE + bc.PULL_GATES.index(m)
    # The push <-> pull rule (pull when frontier edges x alpha > nnz(A') x the unvisited share + the pull floor), for every
    # (alpha, floor) a plan starts with — 48 or 20 and no floor, or, with the blocked push, 6 or 8 and n / 16 — and for the
    # share taken over the vertices with an in-edge (alive rule) or over all of them: level 1 is a push, level 2 a pull,
    # level 3 a push
    assert frontier_edges(n, rows, level, 1) == (1, m) and frontier_edges(n, rows, level, 2) == (m, 1)
    for alpha, floor in ((48, 0), (20, 0), (8, n // 16), (6, n // 16)):
        assert not 1 * alpha > nnz - ind[0]                                # (the begin kernel's rule has no floor)
        for left, base in ((lambda r: n_alive + 1 - r, n_alive), (lambda r: n - r, n)):
            assert m * alpha > nnz * left(2) // base + floor
            assert not 1 * alpha > nnz * left(2 + m) // base + floor
    # A is stored hypersparse by fgpu_mat_from_coo (the GPU tests upload its CSR); no row or column is a hub
    assert bc.coo_is_hyper(n, rows) and out[named["a"]] == m and ind.max() <= 4
    reached = [int((bc.bfs_levels(n, rows, cols, s)[0] >= 0).sum()) for s in named["sources"]]
    assert reached == [2 + m + len(named["R"]), len(named["R"]), 1]


# ---- the source rule --------------------------------------------------------------------------------------------------

def constant(text, name):
    m = re.search(r"constexpr\s+[\w ]+?\b" + name + r"\s*=\s*(\d+)(?:ull|u)?\s*(?:<<\s*(\d+))?\s*;", text)
    assert m, f"{name}: definition not found"
    return int(m.group(1)) << int(m.group(2) or 0)


def test_the_kernel_thresholds_are_the_ones_the_cases_were_built_for():
    src = {f: open(os.path.join(CSRC, f)).read() for f in ("bfs.hip", "common.hpp", "dist.hip")}
    rebuild = {"QGATE": "heavy_push (a b must exceed it), push_ladder / fan (their levels must stay below), pull_gate (decoys)",
               "PULL_QGATE": "pull_gate (PULL_GATES)",
               "PUSH_VPB": "heavy_push (the 1024-vertex item of its bitmap-mode level)",
               "PUSH_HUB_DEG": "push_ladder (PUSH_DEGS)", "PUSH_HUB_CHUNK": "push_ladder (PUSH_DEGS)",
               "HUB_DEG": "pull_ladder (PULL_DEGS) and push_ladder (PUSH_DEGS)",
               "TINY_VERTS": "fan (FANS)", "TINY_EDGES": "fan (FANS)",
               "PULL_H": "pull_ladder (PULL_DEGS: the phase boundaries are PULL_H and PULL_H + 4)",
               "PULL_R": "pull_ladder (hub and ordinary rows in one trip)",
               "HYPER_MIN_ROWS": "push_ladder (uploaded as CSR) and every case above that many vertices"}
    home = {"HUB_DEG": "common.hpp", "PUSH_HUB_DEG": "common.hpp", "PUSH_HUB_CHUNK": "common.hpp",
            "HYPER_MIN_ROWS": "common.hpp"}
    for name, case in rebuild.items():
        got = constant(src[home.get(name, "bfs.hip")], name)
        assert got == getattr(bc, name), f"{name} is {got} in the kernels, bfs_cases.py has {getattr(bc, name)}: rebuild {case}"
    # when a level may append (pull_gate is built on this expression), and the factors and the floor of the push <-> pull rule
    # a plan starts with (pull_gate's levels take their direction under each of them)
    assert ("((nd == 1 ? v1 : unv) <= QGATE || (nd == 2 && alive_unv <= PULL_QGATE))" in src["bfs.hip"]
            and "const u64 unv = n_total > reached ? n_total - reached : 0;" in src["bfs.hip"]), \
        "the append rule of the control step changed: recheck pull_gate and heavy_push"
    assert "c->pull_floor = (a.pb && n_alive) ? a.n / 16u : 0u;" in src["bfs.hip"], "the pull floor changed: recheck pull_gate"
    assert re.findall(r"p->alpha = [^;]*\? (\d+)\.0 : (\d+)\.0;", src["bfs.hip"]) == [("20", "48"), ("6", "8")], \
        "the default alpha changed: recheck pull_gate's directions"
    # the hypersparse rule of fgpu_mat_from_coo
    assert re.search(r"nrows\s*>\s*HYPER_MIN_ROWS\s*&&\s*nvec\s*\*\s*16\s*<=\s*nrows", open(os.path.join(CSRC, "mat.hip")).read()), \
        "prefer_hyper changed: bfs_cases.coo_is_hyper must follow"
    # bitmaps are padded to 4096 vertices: a plan's in fgpu_slab_layout, a vxm's in fgpu_vxm
    body = src["dist.hip"][src["dist.hip"].index("fgpu_info fgpu_slab_layout("):]
    m = re.search(r"\(per\s*\+\s*(\d+)\)\s*&\s*~(\d+)ull", body[:body.index("\n}\n")])
    assert m and int(m.group(1)) == int(m.group(2)) == bc.PAD - 1, "fgpu_slab_layout pads differently: rebuild ragged_random's sizes"
    body = src["bfs.hip"][src["bfs.hip"].index("fgpu_info fgpu_vxm("):]
    m = re.search(r"\(\(n\s*\+\s*(\d+)\)\s*&\s*~(\d+)u\)\s*/\s*64", body[:body.index("\n}\n")])
    assert m and int(m.group(1)) == int(m.group(2)) == bc.PAD - 1, "fgpu_vxm pads differently: rebuild ragged_random's sizes"
    # the sizes straddle every boundary the kernels have: 64-bit words, 1024-vertex items, the padding
    for edge in (64, bc.PUSH_VPB, bc.PAD):
        assert {edge - 1, edge, edge + 1} <= set(bc.RAGGED_SIZES)
    assert any(n % 4 for n in bc.RAGGED_SIZES if n > bc.PAD)
