"""CPU: the catalogue of tests/algo_edges.py holds what it names — the ladder's degrees, chunk counts and word positions, what
every mask leaves of a hub row, the iteration counts of the batch paths — and every condition the comparisons of
tests/test_gpu_algo_edges.py rely on holds for the references alone on these inputs.  Where a procedure has two independent
references they agree on the ladder."""
import math
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import algo_edges as ae  # noqa: E402
import cdlp_check  # noqa: E402
import hc_check  # noqa: E402
import wcc_check  # noqa: E402
from maxflow_check import certify, dinic  # noqa: E402
from msf_check import bits_of, msf  # noqa: E402
from sssp_check import sssp  # noqa: E402

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "falkordb_amd", "csrc")
B = ae.BATCH


def constant(text, name):
    m = re.search(r"constexpr\s+[\w ]+?\b" + name + r"\s*=\s*(\d+)(?:ull|u)?\s*;", text)
    assert m, f"{name}: definition not found"
    return int(m.group(1))


def test_the_constants_are_the_kernels():
    src = {f: open(os.path.join(CSRC, f)).read() for f in ("common.hpp", "wcc.hip", "pagerank.hip", "cdlp.hip", "harmonic.hip",
                                                           "sssp.hip", "maxflow.hip", "algo.hip")}
    assert constant(src["common.hpp"], "HUB_DEG") == ae.HUB_DEG and constant(src["common.hpp"], "HUB_CHUNK") == ae.HUB_CHUNK
    assert constant(src["wcc.hip"], "WCC_AUTO_MIN_N") == ae.WCC_AUTO_MIN_N
    for f, name in (("pagerank.hip", "PR_BATCH"), ("cdlp.hip", "CDLP_BATCH"), ("harmonic.hip", "HC_BATCH"),
                    ("sssp.hip", "SSSP_BATCH"), ("algo.hip", "BATCH")):
        assert constant(src[f], name) == B, f"{name} was retuned: batch_paths must reach 2 B + 1"
    assert constant(src["maxflow.hip"], "MF_BATCH") == ae.MF_BATCH
    assert constant(src["maxflow.hip"], "MF_GLOBAL_EVERY") == ae.MF_GLOBAL_EVERY


# ---- the ladder --------------------------------------------------------------------------------------------------------

def test_ladder_degrees_chunks_and_word_positions():
    n = ae.LADDER_N
    assert n == 256 + 8193 + 37 == 8486 and n % 64 == 38
    hubs = np.array(ae.LADDER_HUBS)
    assert [h % 64 for h in ae.LADDER_HUBS[:5]] == [0, 63, 0, 63, 8]                  # lane 0 and lane 63, twice; mid-word
    assert ae.LADDER_HUBS[5] == n - 1 and (n - 1) // 64 == (n + 63) // 64 - 1          # in the partial last word
    assert tuple(-(-d // ae.HUB_CHUNK) if d >= ae.HUB_DEG else 0 for d in ae.LADDER_DEGS) == ae.LADDER_CHUNKS == (0, 1, 2, 2, 2, 3)
    assert [d % ae.HUB_CHUNK for d in ae.LADDER_DEGS] == [4095, 0, 1, 4095, 0, 1]      # one-entry last chunks, two full chunks
    _, rows, cols = ae.hub_ladder("out")
    assert len(rows) == 36951
    assert tuple(ae.degrees(n, rows)[hubs]) == ae.LADDER_DEGS
    assert ae.degrees(n, rows).sum() - sum(ae.LADDER_DEGS) == 85 + 2                   # every 97th leaf, and the two short rows
    assert ae.degrees(n, cols)[hubs].max() < 64                                        # the other side has no hub row at a hub
    _, irows, icols = ae.hub_ladder("in")
    assert tuple(ae.degrees(n, icols)[hubs]) == ae.LADDER_DEGS                         # rows of the transpose
    assert np.array_equal(np.unique(irows * n + icols), np.unique(cols * n + rows))
    _, srows, scols = ae.hub_ladder("sym")
    assert tuple(ae.degrees(n, srows)[hubs]) == ae.LADDER_DEGS and len(srows) <= 75000
    assert np.array_equal(np.unique(srows * n + scols), np.unique(scols * n + srows))
    other = np.setdiff1d(np.arange(n), hubs)
    for r in (rows, irows, srows):
        assert ae.degrees(n, r)[other].max() < 64                                      # every other row is a short one
        assert np.all(np.diff(r * n) >= 0)
    for r, c in ((rows, cols), (irows, icols), (srows, scols)):
        assert len(np.unique(r * n + c)) == len(r)
    assert set(zip(rows.tolist(), cols.tolist())) >= {(1, 2), (2, 3)}
    # flipped: the same degrees over the last leaves; the leaves all six hubs share are the last 4095 entries of every row
    _, frows, fcols = ae.hub_ladder("sym", flip=True)
    assert tuple(ae.degrees(n, frows)[hubs]) == ae.LADDER_DEGS and len(frows) == len(srows)
    assert ae.degrees(n, frows)[other].max() < 64
    for h, d in zip(ae.LADDER_HUBS, ae.LADDER_DEGS):
        assert np.array_equal(fcols[frows == h], ae.LEAF0 + 8193 - d + np.arange(d))


def test_masks_leave_every_hub_row_partial_and_dirty_bits_sit_past_n():
    n, rows, cols = ae.hub_ladder("out")
    masks = ae.ladder_masks()
    assert [m[0] for m in masks] == ["all", "thirds-off", "low-leaves"]
    assert masks[0][1].all()
    assert not masks[1][1][ae.LADDER_HUBS[1]] and not masks[1][1][ae.LADDER_HUBS[5]]
    for name, act, clean, dirty in masks:
        assert len(clean) == len(dirty) == (n + 63) // 64
        assert np.array_equal(np.unpackbits(clean.view(np.uint8), bitorder="little")[:n].astype(bool), act)
        cb, db = (np.unpackbits(x.view(np.uint8), bitorder="little") for x in (clean, dirty))
        assert np.array_equal(cb[:n], db[:n]) and not cb[n:].any() and db[n:].all() and len(db) - n == 64 - 38
        if name == "all":
            continue
        for h, d in zip(ae.LADDER_HUBS, ae.LADDER_DEGS):
            if act[h]:
                nb = act[cols[rows == h]]
                assert len(nb) == d and nb.any() and not nb.all(), (name, h)
    few = masks[2][1]
    last = cols[rows == ae.LADDER_HUBS[5]]
    assert not few[last[2 * ae.HUB_CHUNK:]].any() and len(last[2 * ae.HUB_CHUNK:]) == 1   # the 8193 row's last chunk is off
    assert all(few[h] for h in ae.LADDER_HUBS)


def test_weights_are_functions_of_the_pair():
    n, rows, cols = ae.hub_ladder("sym")
    w = ae.pair_weights(n, rows, cols, "distinct")
    assert np.array_equal(w, ae.pair_weights(n, cols, rows, "distinct"))
    assert len(np.unique(w[rows < cols])) == int((rows < cols).sum())
    assert (w >= 1).all() and (w == np.floor(w)).all() and w.max() * n < 2 ** 53
    assert (ae.pair_weights(n, rows, cols, "equal") == 4.0).all()


# ---- the references alone ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("direction", ["out", "in"])
def test_harmonic_margin_and_exact_counts_on_the_ladder(direction):
    n, rows, cols = ae.hub_ladder(direction)
    rp, ci = hc_check.csr_of(n, rows, cols)
    for name, act, _, _ in ae.ladder_masks():
        active = None if name == "all" else act
        margin = hc_check.round_margin(n, rp, ci, active)
        assert margin > 1e-6, (name, margin)
        score, reach, _, st = hc_check.harmonic(n, rp, ci, active)
        assert 1 <= st[0] <= 6                                                 # a small diameter: a few 8 MB iterations
        if name != "low-leaves":
            continue
        # plain BFS from every vertex: the sketch counts within four standard errors (1.04 / sqrt(1024) each) of the exact
        # ones — the ladder has a few dozen distinct out-balls, so this bounds a few dozen estimates — and the scores, sums
        # of count differences divided by the distance, within the same share of the exact scores
        es, er = hc_check.exact_harmonic(n, rp, ci, active)
        sigma = 1.04 / 32
        assert (np.abs(reach - er) <= 4 * sigma * np.maximum(er, 1) + 0.5).all()
        assert (np.abs(score - es) <= 4 * sigma * np.maximum(es, 1) + 0.5).all()
        assert np.array_equal(reach < 0, er < 0)


@pytest.mark.parametrize("direction", ["out", "in"])
def test_pagerank_oracle_converges_on_the_ladder(direction):
    import oracle
    from oracle import pagerank as opr
    n, rows, cols = ae.hub_ladder(direction)
    a = oracle.build_csr(n, n, rows.astype(np.uint64), cols.astype(np.uint64))
    for name, act, _, _ in ae.ladder_masks():
        ref, it = opr.pagerank(a, active=None if name == "all" else act)
        assert 1 <= it < 100, (name, it)
        assert abs(float(ref.astype(np.float64).sum()) - 1.0) < 1e-4
        assert (ref[~act] == 0).all() and (ref[act] > 0).all()


@pytest.mark.parametrize("flip", [False, True], ids=["first-leaves", "last-leaves"])
def test_wcc_and_cdlp_references_agree_on_the_ladder(flip):
    n, rows, cols = ae.hub_ladder("out", flip)
    _, srows, scols = ae.hub_ladder("sym", flip)
    rp, ci = wcc_check.csr_of(n, rows, cols)
    srp, sci = cdlp_check.csr_of(n, srows, scols)
    for name, act, _, _ in ae.ladder_masks():
        active = None if name == "all" else act
        want = wcc_check.wcc_labels(n, rp, ci, active)
        assert np.array_equal(want, wcc_check.union_find_labels(n, rows, cols, active))
        assert np.array_equal(want, wcc_check.wcc_labels(n, srp, sci, active))
        if act[0] and not (flip and name == "low-leaves"):                     # (flipped, that mask leaves three hubs alone)
            assert (want[np.array(ae.LADDER_HUBS)[act[list(ae.LADDER_HUBS)]]] == 0).all()   # the hubs share leaves
        for itermax in (1, 10):
            a = cdlp_check.cdlp_labels(n, srp, sci, itermax, active)
            b = cdlp_check.dict_labels(n, srows, scols, itermax, active)
            assert np.array_equal(a[0], b[0]) and a[1:] == b[1:]


def scipy_flow(n, rows, cols, caps, src, sink):
    """a maximum flow by scipy on the capacities x 4 (integers), as certify()'s (value, rows, cols, flows)"""
    import scipy.sparse as sp
    from scipy.sparse.csgraph import maximum_flow
    live = caps > 0
    c4 = np.rint(caps[live] * 4).astype(np.int32)
    assert np.array_equal(c4 / 4, caps[live])
    g = sp.csr_matrix((c4, (rows[live], cols[live])), shape=(n, n))
    res = maximum_flow(g, src, sink)
    f = res.flow.tocoo()
    keep = f.data > 0
    fr, fc, fv = f.row[keep].astype(np.int64), f.col[keep].astype(np.int64), f.data[keep] / 4
    # cancel what a pair carries in both directions
    net = {}
    for u, v, x in zip(fr.tolist(), fc.tolist(), fv.tolist()):
        net[(u, v)] = net.get((u, v), 0.0) + x
    out = []
    for (u, v), x in net.items():
        y = x - net.get((v, u), 0.0)
        if y > 0:
            out.append((u, v, y))
    out.sort()
    return res.flow_value / 4, [o[0] for o in out], [o[1] for o in out], [o[2] for o in out]


@pytest.mark.parametrize("mirror", [False, True], ids=["hubs-fan-out", "hubs-gather"])
def test_dinic_and_certify_agree_on_the_ladder_network(mirror):
    degs = ae.LADDER_DEGS                                                              # (the plain-Python Dinic takes well under a second on the whole ladder)
    n, rows, cols, caps, src, sink, hubs = ae.ladder_flow(degs, mirror)
    assert (caps * 4 == np.floor(caps * 4)).all() and (caps >= 0).all()               # dyadic: every sum is exact
    lo, hi = np.minimum(rows, cols)[caps > 0], np.maximum(rows, cols)[caps > 0]
    pairs = np.unique(lo * n + hi)
    per = np.bincount(np.concatenate([pairs // n, pairs % n]), minlength=n)            # a vertex' row of the residual network
    assert tuple(per[list(hubs)]) == degs
    value = dinic(n, rows, cols, caps, src, sink)
    sv, fr, fc, fv = scipy_flow(n, rows, cols, caps, src, sink)
    assert value == sv and value > 0
    certify(n, rows, cols, caps, src, sink, value, fr, fc, fv)


def test_msf_and_sssp_references_run_on_the_ladder():
    n, rows, cols = ae.hub_ladder("sym")
    for kind in ("distinct", "equal"):
        fr, fc, fb, comp = msf(n, rows, cols, bits_of(ae.pair_weights(n, rows, cols, kind)))
        assert np.array_equal(comp, wcc_check.wcc_labels(n, *wcc_check.csr_of(n, rows, cols)))
        assert len(fr) == n - wcc_check.components(comp)
    n, rows, cols = ae.hub_ladder("out")
    for src, reached in ((0, 8193 + 6), (ae.LEAF0, 8193 + 6), (1, 3)):
        dist, parent, depth = sssp(n, rows, cols, bits_of(ae.pair_weights(n, rows, cols, "distinct")), src)
        assert int(np.isfinite(dist).sum()) == reached and depth.max() <= 8   # a few levels


# ---- word graphs -------------------------------------------------------------------------------------------------------

def test_word_graphs_sit_on_both_sides_of_one_and_two_words():
    g = ae.word_graphs()
    assert tuple(g) == ae.WORD_SIZES == (63, 64, 65, 127, 128, 129)
    for n, (rows, cols, masks) in g.items():
        assert ae.degrees(n, rows).min() >= 1 and (rows < n).all() and (cols < n).all()
        assert set(zip(rows.tolist(), cols.tolist())) >= {(i, (i + 1) % n) for i in range(n)} | {(i, (7 * i + 3) % n) for i in range(n)}
        (_, on, con, don), (_, off, coff, doff) = masks
        assert on[n - 1] and not off[n - 1] and np.array_equal(on[:-1], off[:-1]) and not on.all()
        for act, clean, dirty in ((on, con, don), (off, coff, doff)):
            cb, db = (np.unpackbits(x.view(np.uint8), bitorder="little") for x in (clean, dirty))
            assert np.array_equal(cb[:n].astype(bool), act) and np.array_equal(cb[:n], db[:n]) and not cb[n:].any()
            assert db[n:].all() and (n % 64 == 0) == np.array_equal(clean, dirty)
        rp, ci = hc_check.csr_of(n, rows, cols)
        for act in (None, on, off):
            assert hc_check.round_margin(n, rp, ci, act) > 1e-6                # what test_gpu_hc.check asks of its input


# ---- batch paths -------------------------------------------------------------------------------------------------------

def test_batch_paths_take_every_iteration_count():
    paths = ae.batch_paths()
    assert sorted(paths) == list(range(1, 2 * B + 2))
    assert {B - 1, B, B + 1, 2 * B - 1, 2 * B, 2 * B + 1} <= set(paths)
    for L, g in paths.items():
        n, rows, cols = g["directed"]
        assert n == L + 1
        rp, ci = hc_check.csr_of(n, rows, cols)
        assert hc_check.harmonic(n, rp, ci)[3][0] == L                      # L iterations change a sketch, the next ends the run
        assert hc_check.round_margin(n, rp, ci) > 1e-6
        dist, parent, depth = sssp(n, rows, cols, None, 0)
        assert depth.max() == L and dist[L] == L
        n, rows, cols = g["forest"]
        assert n == 2 ** L + 1 and len(rows) == 2 * (n - 1)
        parent = np.maximum(np.arange(n) - 1, 0)                             # every vertex hooked to its smaller neighbour
        assert ae.pointer_jumps(parent) == L
        assert ae.pointer_jumps(np.maximum(np.arange(2 ** (L - 1) + 1) - 1, 0)) == L - 1   # half the depth: a jump less
        n, rows, cols = g["flood"]
        rp, ci = cdlp_check.csr_of(n, rows, cols)
        label, st = cdlp_check.cdlp_stats(n, rp, ci, 100)
        assert st[0] == L and st[1] == 0 and not label.any()
        if L > 1:
            assert cdlp_check.cdlp_stats(n, rp, ci, L - 1)[1][1] > 0         # cut one iteration short it is still changing
        n, rows, cols = g["swap"]
        rp, ci = cdlp_check.csr_of(n, rows, cols)
        label, st = cdlp_check.cdlp_stats(n, rp, ci, L)
        assert st[0] == L and st[1] == 2 and label.tolist() == ([1, 0] if L % 2 else [0, 1])


def test_pagerank_oracle_runs_exactly_itermax_iterations_at_tol_zero():
    import oracle
    from oracle import pagerank as opr
    n, rows, cols = ae.hub_ladder("in")                                      # (the word graphs are regular: uniform scores at once)
    a = oracle.build_csr(n, n, rows.astype(np.uint64), cols.astype(np.uint64))
    seen = set()
    for L in range(1, 2 * B + 2):
        ref, it = opr.pagerank(a, 0.85, 0.0, L)
        assert it == L
        seen.add(ref.tobytes())
    assert len(seen) == 2 * B + 1                                            # every L gives other scores: a wrong count shows


def test_bottleneck_paths_have_one_minimum():
    for n in (2, 3, 70):
        rows, cols, caps = ae.bottleneck_path(n)
        assert dinic(n, rows, cols, caps, 0, n - 1) == 3.25 and int((caps == 3.25).sum()) == 1
    assert math.isclose(3.25 * 4, 13.0)
