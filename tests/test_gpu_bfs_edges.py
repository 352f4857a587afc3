"""BFS (fgpu_bfs_plan_*, fgpu_bfs) and fgpu_vxm at ragged sizes, at the degree and frontier thresholds of bfs.hip and in every
direction, against the plain numpy references of tests/bfs_cases.py: levels, statistics and vxm words bit for bit, parents
by the parent check (any in-neighbour one level up is a valid parent) and, where a case forces it, the one possible parent.
tests/test_bfs_cases_cpu.py holds the references to the oracle and proves, from the edge lists, that each case reaches
the branch its test names."""
import os
import sys

import numpy as np
import pytest

from falkordb_amd import engine
from falkordb_amd._ffi import FgpuError

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bfs_cases as bc  # noqa: E402
from test_options_cpu import OPTIONS  # noqa: E402

pytestmark = pytest.mark.gpu

TOUCHED = ("bfs_tiny", "bfs_hub_first", "bfs_alive_rule", "bfs_pb", "bfs_pb_min_edges", "bfs_prof_split")
BLOCKED = dict(bfs_pb=2, bfs_pb_min_edges=1, bfs_tiny=0)


class Case:
    """A built graph with its reference searches (computed once, shared by every configuration, never written to)."""

    def __init__(self, built):
        self.n, self.rows, self.cols, self.named = built
        self.sources = self.named["sources"]
        self._ref = {}

    def ref(self, src, max_level=-1):
        if (src, max_level) not in self._ref:
            level, edges = bc.bfs_levels(self.n, self.rows, self.cols, src, max_level)
            level.setflags(write=False)
            self._ref[src, max_level] = (level, edges)
        return self._ref[src, max_level]

    def upload(self, ctx, transpose=True):
        """A through fgpu_mat_from_coo — or, where that would store it hypersparse (a plan takes the dense form only),
        through fgpu_mat_from_csr — and At = its transpose, built on the device."""
        n = self.n
        if bc.coo_is_hyper(n, self.rows):
            rowptr, colidx = bc.csr(n, self.rows, self.cols)
            A = ctx.mat_from_csr(n, n, rowptr, colidx)
        else:
            A = ctx.mat_from_coo(n, n, self.rows, self.cols)
        assert A.nvals == len(self.rows)
        return A, (A.transpose() if transpose else None)


_CASES = {}


def case(name, *args):
    if (name, args) not in _CASES:
        _CASES[name, args] = Case(bc.degenerate()[args[0]] if name == "degenerate" else getattr(bc, name)(*args))
    return _CASES[name, args]


def check_search(c, plan, src, level, parent, max_level=-1):
    """Steps 4 - 6 of every search: levels, parents, statistics against the reference."""
    ref, ref_edges = c.ref(src, max_level)
    np.testing.assert_array_equal(level, ref)
    if parent is not None:
        bc.check_parents(c.n, c.rows, c.cols, src, level, parent)
    st = plan.stats()
    assert st["edges_traversed"] == ref_edges
    assert st["reached"] == int((ref >= 0).sum())
    assert st["levels"] == bc.level_steps(ref, max_level)
    assert st["push_levels"] + st["pull_levels"] == st["levels"]
    return st


def search_all(ctx, c, A, At, force=0, reps=1, evidence=None):
    """One plan, every source of the case in its order (a later search reaches fewer vertices than an earlier one: stale
    levels and parents must be masked), with and without parents, then cut at max_level = 2."""
    plan = engine.BfsPlan(ctx, A, At)
    try:
        plan.tune(force_direction=force)
        for src in c.sources:
            for want_parent in (True, False):
                for rep in range(reps):
                    plan.run(src, -1, want_parent=want_parent)
                    level, parent = plan.fetch(want_parent=want_parent)
                    st = check_search(c, plan, src, level, parent)
                    if force == 1 or At is None:
                        assert st["push_levels"] == st["levels"] and st["pull_levels"] == 0
                    if force == 2:
                        assert st["pull_levels"] == st["levels"] and st["push_levels"] == 0
                    if evidence:
                        evidence(src, rep, st, level, parent)
            plan.run(src, 2, want_parent=True)
            level, parent = plan.fetch(want_parent=True)
            check_search(c, plan, src, level, parent, max_level=2)
    finally:
        plan.free()


def directions(ctx, c, A, At, **kw):
    """force_direction 0 / 1 / 2 over (A, At) and the push-only plan without a transpose."""
    for force in (0, 1, 2):
        search_all(ctx, c, A, At, force=force, **kw)
    search_all(ctx, c, A, None, **kw)


# ---- ragged sizes ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", bc.RAGGED_SIZES)
def test_ragged_sizes_in_every_direction(ctx, n):
    """~3 n random edges at sizes around every boundary of the bitmaps (64-bit words, 1024-vertex push items, the padding
    to 4096 vertices): the last word, item and pull trip are partial, the vertices [n, n_pad) exist only as padding (head
    array, alive bits, level masking), and vertex n - 1 is discovered and expanded.  Sources in the order 0, a vertex
    without out-edges, n - 1: the second search leaves all but one level of the first one stale.  (n <= 3: the edges that
    fit, sources 0 and n - 1.)"""
    c = case("ragged_random", n)
    A, At = c.upload(ctx)
    directions(ctx, c, A, At)


@pytest.mark.parametrize("tiny", [0, 1, 2])
@pytest.mark.parametrize("n", [65, 1025, 4097])
def test_ragged_sizes_under_every_tiny_mode(ctx, n, tiny):
    """bfs_tiny_kernel on ragged sizes: its zeroing of the frontier words and its clamp at n; under bfs_tiny = 2 every search
    runs three times so that the launch sequence sized by the previous search is used."""
    c = case("ragged_random", n)
    with ctx.options(bfs_tiny=tiny):
        A, At = c.upload(ctx)
        for force in (0, 1):
            search_all(ctx, c, A, At, force=force, reps=3 if tiny == 2 else 1)


@pytest.mark.parametrize("n", [65, 1025, 4099])
def test_ragged_sizes_without_the_hub_first_order(ctx, n):
    """bfs_hub_first = 0: the pull levels read the matrix's own column order of A' (no reordered copy, heads taken from
    the ascending rows); forced pull and auto direction."""
    c = case("ragged_random", n)
    with ctx.options(bfs_hub_first=0):
        A, At = c.upload(ctx)
        for force in (2, 0):
            search_all(ctx, c, A, At, force=force)


@pytest.mark.parametrize("name", ["n1_empty", "n1_self_loop", "n2_one_edge", "n65_empty"])
def test_degenerate_graphs(ctx, name):
    """One vertex, one edge, no edge at all: searches that end at level 0 or 1, plans over an empty A' (ensure_pull_order
    and the hub lists return early on nnz == 0), in every direction and tiny mode."""
    c = case("degenerate", name)
    for tiny in (0, 1, 2):
        with ctx.options(bfs_tiny=tiny):
            A, At = c.upload(ctx)
            directions(ctx, c, A, At)
    A, At = c.upload(ctx)
    for src in c.sources:
        level, parent, edges = engine.bfs(ctx, A, At, src, -1, want_parent=True)
        np.testing.assert_array_equal(level, c.ref(src)[0])
        bc.check_parents(c.n, c.rows, c.cols, src, level, parent)
        assert edges == c.ref(src)[1]


@pytest.mark.parametrize("alive", [0, 1])
def test_alive_rule_off_and_on_in_auto_direction(ctx, alive):
    """bfs_alive_rule: the push <-> pull rule takes the unvisited share over all vertices (0) or over those with an in-edge
    (1), and only under 1 may a pull level append because few of the latter are left (PULL_QGATE).  Auto direction on
    ragged sizes, on the ladder whose 4096 decoys have no in-edge, on the heavy push graph — and on pull_gate, where that
    bound is the only one that can open the queue for the pull level: under 0 it stays shut on both sides of the bound,
    under 1 it opens at the bound and not one past it."""
    with ctx.options(bfs_alive_rule=alive):
        for c in (case("ragged_random", 4099), case("ragged_random", 257), case("pull_ladder"), case("heavy_push"),
                  case("pull_gate", bc.PULL_GATES[0]), case("pull_gate", bc.PULL_GATES[1])):
            A, At = c.upload(ctx)
            search_all(ctx, c, A, At, force=0)


# ---- push ------------------------------------------------------------------------------------------------------------------

def test_heavy_push_bitmap_mode_ragged_last_quad(ctx):
    """heavy_push under forced push: the level out of L1 examines 160,000 > QGATE edges, so it does not append and the
    level out of L2 walks the bitmap (push_fused, bitmap mode).  n = 1203: thread 44 of item 1 holds the quad v0 = 1200
    with v0 + 4 > n, all three of its vertices in the frontier and each with an edge into L3 — the `else if (nib)` branch
    reads their row pointers one by one, clamped at n.  Every level is a push, none goes by propagation blocking (off), and
    the same graph in the other directions and without a transpose."""
    c = case("heavy_push")
    with ctx.options(bfs_pb=0):
        A, At = c.upload(ctx)

        def evidence(src, rep, st, level, parent):
            assert ctx.get_option("bfs_pb_last_levels") == 0
            if src == 0:
                assert st["levels"] == 4

        search_all(ctx, c, A, At, force=1, evidence=evidence)
        search_all(ctx, c, A, At, force=0)
        search_all(ctx, c, A, At, force=2)
        search_all(ctx, c, A, None)
        for tiny in (0, 1):
            with ctx.options(bfs_tiny=tiny):
                search_all(ctx, c, A, At, force=1)


def test_heavy_push_blocked_ragged_last_window(ctx):
    """heavy_push by propagation blocking (bfs_pb = 2, one edge is enough, forced push): the level out of L1 is fused
    launch 1, which the host arms; its discoveries are L2 = ids 803 .. 1202, and the last 64-vertex window of
    bfs_pb_apply_kernel, 1152 .. 1202, ends at n % 64 = 51: `vec_ok` is false there and the degrees are read one by one,
    clamped at n - 1.  Every search twice: the second one runs with the launches the first one taught the plan."""
    c = case("heavy_push")
    with ctx.options(**BLOCKED):
        A, At = c.upload(ctx)
        ran = {}

        def evidence(src, rep, st, level, parent):
            ran[src, rep] = ctx.get_option("bfs_pb_last_levels")

        search_all(ctx, c, A, At, force=1, reps=2, evidence=evidence)
        assert ran[0, 1] >= 1, ran
        search_all(ctx, c, A, None, reps=2)
        search_all(ctx, c, A, At, force=0, reps=2)


def test_push_ladder_hub_degree_boundaries(ctx):
    """push_ladder: the level out of {h_k} is a queue-mode push (18,409 <= QGATE edges) whose rows have 1023 (ordinary, one
    item), 1024 and 1025 (PUSH_HUB_DEG: the chunk list, one chunk and one chunk + 1 edge), 2049 (a last chunk of one
    edge), 4095 / 4096 / 4097 (HUB_DEG: the coarse list of the bitmap kernels) out-edges into overlapping ranges of one
    pool: ordinary and hub items race for the same discoveries, and each must be counted once."""
    c = case("push_ladder")
    A, At = c.upload(ctx)
    directions(ctx, c, A, At)
    for tiny in (0, 1):
        with ctx.options(bfs_tiny=tiny):
            search_all(ctx, c, A, At, force=1)
    with ctx.options(**BLOCKED):
        search_all(ctx, c, A, At, force=1, reps=2)


@pytest.mark.parametrize("tiny", [0, 1, 2])
@pytest.mark.parametrize("verts,per", bc.FANS)
def test_fan_levels_at_the_tiny_thresholds(ctx, verts, per, tiny):
    """fan: the level out of the third layer has exactly TINY_VERTS vertices and TINY_EDGES edges (1024 x 4: the tiny kernel
    takes it, its 1024-entry list full), one vertex more (1025 x 4) or one edge per vertex more (1024 x 5): the control
    step hands those to the fused kernel and the tiny kernel must return at once.  bfs_tiny off / on / by history (three
    runs each), auto and forced push."""
    c = case("fan", verts, per)
    with ctx.options(bfs_tiny=tiny):
        A, At = c.upload(ctx)
        for force in (0, 1):
            search_all(ctx, c, A, At, force=force, reps=3 if tiny == 2 else 1)
        search_all(ctx, c, A, None, reps=3 if tiny == 2 else 1)


# ---- pull ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("hub_first", [0, 1])
def test_pull_ladder_every_phase_returns_the_one_parent(ctx, hub_first):
    """pull_ladder under forced pull: at level 2 the only frontier in-neighbour of t_d is x_d, the LAST entry of its row
    in either column order, so the row is found by the head (d = 1), by phase A2 (2, 3, 5: entries 2 .. 5; t_3 = n - 1 is
    the last row of A' and takes the `tail` loads), by phase B (6, 7, 69: one trip; 70, 133, 4095: more), or by the hub
    section (4096, 4097) — whose rows share the 64-bit word 64 with all the others, so that word is published with
    atomics (`hub_here`).  The parent is x_d and nothing else; the 4096 decoys stay unreached."""
    c = case("pull_ladder")
    x, u, t = c.named["x"], c.named["u"], c.named["t"]
    with ctx.options(bfs_hub_first=hub_first):
        A, At = c.upload(ctx)

        def evidence(src, rep, st, level, parent):
            if src != 0:
                return
            assert st["levels"] == 4
            assert (level[c.named["decoys"]] == -1).all()
            if parent is not None:
                for d in bc.PULL_DEGS:
                    assert parent[t[d]] == x[d], d
                    assert parent[u[d]] == t[d], d
                    assert parent[x[d]] == 0, d
                assert (parent[c.named["decoys"]] == -1).all()

        search_all(ctx, c, A, At, force=2, evidence=evidence)
        search_all(ctx, c, A, At, force=0, evidence=evidence)
        search_all(ctx, c, A, At, force=1, evidence=evidence)
        search_all(ctx, c, A, None, evidence=evidence)
        for tiny in (0, 1):
            with ctx.options(bfs_tiny=tiny):
                search_all(ctx, c, A, At, force=2, evidence=evidence)


@pytest.mark.parametrize("m", bc.PULL_GATES)
def test_pull_level_at_and_past_its_append_bound(ctx, m):
    """pull_gate in auto direction (alive rule on): the level out of `a` is a pull.  At the control step that opens the
    queue for it more than QGATE vertices are unvisited (131,077 decoys without an edge), so the bound on all vertices keeps
    the queue shut, and exactly PULL_QGATE (or PULL_QGATE + 1) of them have an in-edge: the pull appends its m discoveries
    (or does not), and the level out of F is a push — from that queue, or from the bitmap.  Nothing counts the appends:
    the CPU test proves the two figures from the edge list, and both sides of the bound must give the reference's vectors
    and statistics.  The plans here have no propagation-blocking launches (bfs_pb = 1 builds them from 2^24 vertices), so the
    pull of listed candidates (direction 4) is never armed.  Pull and push levels are both counted; forced directions, the
    alive rule off (the queue stays shut on both sides) and the tiny kernel give the same vectors."""
    c = case("pull_gate", m)
    A, At = c.upload(ctx)

    def evidence(src, rep, st, level, parent):
        if src == 0:
            assert st["pull_levels"] >= 1 and st["push_levels"] >= 2, st

    search_all(ctx, c, A, At, force=0, evidence=evidence)
    search_all(ctx, c, A, At, force=2)
    search_all(ctx, c, A, At, force=1)
    with ctx.options(bfs_alive_rule=0):
        search_all(ctx, c, A, At, force=0)
    with ctx.options(bfs_tiny=1):
        search_all(ctx, c, A, At, force=0, evidence=evidence)


# ---- the profiled, synchronous path ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("split", [0, 1])
@pytest.mark.parametrize("name,pb", [("heavy_push", 0), ("heavy_push", 2), ("pull_ladder", 0), ("ragged_random", 0)])
def test_profiled_plan_runs_level_by_level(ctx, name, pb, split):
    """plan.profile(True): fgpu_bfs_run steps the search one level at a time between HIP events (profiled_level), with the
    plain instantiation or, under bfs_prof_split, the twins named after the direction.  Same levels, parents and
    statistics; the profile holds one launch per level; profile(False) puts the plan back on the asynchronous path."""
    c = case(name, 1025) if name == "ragged_random" else case(name)
    opts = dict(bfs_prof_split=split, bfs_pb=pb)
    if pb:
        opts.update(bfs_pb_min_edges=1, bfs_tiny=0)
    with ctx.options(**opts):
        A, At = c.upload(ctx)
        plan = engine.BfsPlan(ctx, A, At)
        try:
            for force in (0, 1, 2):
                plan.tune(force_direction=force)
                plan.profile(True)
                with pytest.raises(FgpuError):
                    plan.run_async(c.sources[0])                   # a profiled plan runs synchronously
                steps = 0
                for src in c.sources:
                    for want_parent in (True, False):
                        plan.run(src, -1, want_parent=want_parent)
                        level, parent = plan.fetch(want_parent=want_parent)
                        steps += check_search(c, plan, src, level, parent)["levels"]
                    plan.run(src, 2, want_parent=True)
                    level, parent = plan.fetch(want_parent=True)
                    steps += check_search(c, plan, src, level, parent, max_level=2)["levels"]
                prof = plan.profile_read()
                assert len(prof) == 2 and all(e["kernel"] for e in prof)
                assert sum(int(e["launches"]) for e in prof) == steps
                assert all(e["ms"] > 0 and e["alg_bytes"] > 0 for e in prof if e["launches"])
                if force:
                    assert int(prof[2 - force]["launches"]) == 0   # [0] push levels, [1] pull levels
                plan.profile(False)
                assert sum(int(e["launches"]) for e in plan.profile_read()) == 0
                src = c.sources[0]
                plan.run_async(src, -1, True)
                plan.wait()
                level, parent = plan.fetch(want_parent=True)
                check_search(c, plan, src, level, parent)
        finally:
            plan.free()


# ---- fgpu_bfs, the one-call entry --------------------------------------------------------------------------------------------

def hyper_upload(ctx, n, rows, cols):
    rowptr, colidx = bc.csr(n, rows, cols)
    deg = np.diff(rowptr)
    populated = np.nonzero(deg)[0]
    short = np.concatenate([[0], np.cumsum(deg[populated])])
    return ctx.mat_from_csr(n, n, short, colidx, hyper_rows=populated)


def one_call(ctx, c, A, At, src, max_level=-1, want_parent=True):
    level, parent, edges = engine.bfs(ctx, A, At, src, max_level, want_parent=want_parent)
    ref, ref_edges = c.ref(src, max_level)
    np.testing.assert_array_equal(level, ref)
    if want_parent:
        bc.check_parents(c.n, c.rows, c.cols, src, level, parent)
    assert edges == ref_edges


def test_one_call_bfs_on_hypersparse_and_empty_adjacencies(ctx):
    """fgpu_bfs re-emits a hypersparse A or A' in dense form for the call (DenseInputs) — pull_ladder in the hypersparse
    form, A alone and both — while a plan refuses such a handle; a source == n is refused by a dense plan; and after each
    error the next search on the same context is right."""
    c = case("pull_ladder")
    n = c.n
    A, At = c.upload(ctx)
    hA, hAt = hyper_upload(ctx, n, c.rows, c.cols), hyper_upload(ctx, n, c.cols, c.rows)
    for src in c.sources:
        one_call(ctx, c, hA, None, src)
        one_call(ctx, c, hA, hAt, src)
        one_call(ctx, c, hA, hAt, src, want_parent=False)
        one_call(ctx, c, A, hAt, src)
        one_call(ctx, c, hA, hAt, src, max_level=2)
    for bad_A, bad_At in ((hA, None), (hA, hAt), (A, hAt)):
        with pytest.raises(FgpuError, match="hypersparse"):
            engine.BfsPlan(ctx, bad_A, bad_At)
        one_call(ctx, c, A, At, c.sources[0])
    plan = engine.BfsPlan(ctx, A, At)
    try:
        for bad in (n, n + 1, 2**32 + 5):
            with pytest.raises(FgpuError):
                plan.run(bad)
            plan.run(c.sources[1], -1, want_parent=True)
            level, parent = plan.fetch(want_parent=True)
            check_search(c, plan, c.sources[1], level, parent)
    finally:
        plan.free()
    with pytest.raises(FgpuError):
        engine.bfs(ctx, A, At, n)
    one_call(ctx, c, A, At, 0)
    with pytest.raises(FgpuError):
        engine.bfs(ctx, hA, hAt, n)
    one_call(ctx, c, hA, hAt, 0)
    # no edge at all: only the source has a level — dense and, through fgpu_mat_new, hypersparse
    e = case("degenerate", "n65_empty")
    E, Et = e.upload(ctx)
    H = ctx.mat_new(e.n, e.n)
    for src in e.sources:
        for a_, at_ in ((E, Et), (E, None), (H, None), (H, H), (E, H)):
            level, parent, edges = engine.bfs(ctx, a_, at_, src, -1, want_parent=True)
            want = np.full(e.n, -1, dtype=np.int32)
            want[src] = 0
            np.testing.assert_array_equal(level, want)
            np.testing.assert_array_equal(parent, np.where(want == 0, src, -1))
            assert edges == 0
    with pytest.raises(FgpuError, match="hypersparse"):
        engine.BfsPlan(ctx, H, None)
    one_call(ctx, c, A, At, c.sources[0])


# ---- fgpu_vxm ----------------------------------------------------------------------------------------------------------------

def vxm_inputs(c):
    n, named = c.n, c.named
    rng = np.random.default_rng(7 * n)
    frontiers = {"empty": [], "last": [n - 1], "all": np.arange(n), "half": rng.choice(n, (n + 1) // 2, replace=False)}
    ind = np.bincount(c.cols, minlength=n)
    if "x" in named:                                                        # pull_ladder
        frontiers["x_d"] = list(named["x"].values())
        pair = [named["t"][4096], named["t"][5]]
    elif "h" in named:                                                      # push_ladder
        frontiers["hub rows"] = list(named["h"].values())
        word = named["pool"][named["pool"] // 64 == named["pool"][2000] // 64]
        pair = [int(word[np.argmax(ind[word])]), int(word[np.argmin(ind[word])])]
    else:
        pair = [n - 1, max(n - 2, (n - 1) // 64 * 64)]
    assert pair[0] // 64 == pair[1] // 64 and ind[pair[0]] > 0
    masks = {"none": None, "third": bc.bits_of(n, rng.choice(n, n // 3, replace=False)), "pair": bc.bits_of(n, pair),
             "ones": bc.bits_of(n, np.arange(n))}
    return frontiers, masks


@pytest.mark.parametrize("name,arg", [("ragged_random", 65), ("ragged_random", 1023), ("ragged_random", 4097),
                                      ("pull_ladder", None), ("push_ladder", None)])
def test_vxm_ragged_in_every_direction(ctx, name, arg):
    """fgpu_vxm where n is no multiple of 64: push (1), the CSR pull (2: a wavefront per 64 rows, the last one partial, hub
    rows of A' from the chunk list into words that ordinary rows share), auto with and without A' (0), and the tiled
    pull (3) where A' has the 4096 entries the auto rule asks for.  Empty, single, full, half and the cases' own
    frontiers; no mask, a random one, one that holds a hub destination and an ordinary one of the same word, all ones.
    Word for word, so no bit at or past n comes back.  (The inputs never set such a bit: the header leaves it open.)"""
    c = case(name) if arg is None else case(name, arg)
    n = c.n
    A, At = c.upload(ctx)
    frontiers, masks = vxm_inputs(c)
    runs = [(1, At), (2, At), (0, At), (0, None)] + ([(3, At)] if At.nvals >= 4096 else [])
    assert len(runs) == 5 or n < 4096
    for fname, ids in frontiers.items():
        f = bc.bits_of(n, ids)
        for mname, mk in masks.items():
            want = bc.vxm_bits(n, c.rows, c.cols, f, mk)
            if mname == "ones":
                assert not want.any()
            for direction, at in runs:
                got = engine.vxm(ctx, f, mk, A, at, direction)
                np.testing.assert_array_equal(got, want, err_msg=f"{fname} / {mname} / direction {direction}")


def test_every_option_this_file_touches_is_back_at_its_default(ctx):
    defaults = {name: default for name, _, _, _, default in OPTIONS}
    for k in TOUCHED:
        assert ctx.get_option(k) == defaults[k], k
