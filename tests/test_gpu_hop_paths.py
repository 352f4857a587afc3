"""Every cell of the hop's decision (bitexpand.hip: bp_hop_plan) by name: the result against the oracle, and the profiler scopes
that show the intended path ran.

The graph is the constructed one of tests/hop_graph.py at its base size (split rows, a 256-entry group row, a dp and a dm entry).
Hop 1 is pushed in every variant (check_shape asserts T * 32 <= nnz), so hop 2 is the chain's one mid-chain pull and hop 3 its
counting hop, and which form each takes is read off the graph before anything goes to the device:

  light   after hop 1 fewer than n / 8 rows are non-zero (the sparse forms of hop 2), and after hop 2 fewer still: the
          destinations of the flagged vertices are the split, group and small rows (the sparse form of the counting hop)
  heavy   the sources also reach the 800 filler vertices, whose 80 out-edges each cover the 1100 hop-3 sources: both states hold
          more than n / 8 non-zero rows (the dense forms, and — rows of 2 to 16 words — the partitioned one)

Every source has an out-edge (`cover`), so the rows are ceil(nsrc / 64) words wide: 1, 2 (the narrowest partitioned width), 16, and
32 (the LN = 32 arm, outside the row-group and partitioned forms; nsrc <= expand_scan_min keeps the call a batch).  At one word
the partitioned form does not apply, so there the two partitioned rows assert the plain dense count instead.
"""
import os
import sys

import numpy as np
import pytest

from falkordb_amd import engine

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from hop_graph import N_BASE, Case, Forced  # noqa: E402

pytestmark = pytest.mark.gpu
U64 = np.uint64

DENSE, SPARSE, GROUPS = "bp_pull_kernel<dense>", "bp_pull_kernel<sparse>", "sparse pull: row groups"
RECORDS, ITEM_REC = "bp_records_kernel", "bp_pull_items_rec_kernel"
DENSE_COUNT, SPARSE_COUNT, SIDE = "bp_pull_kernel<dense, count>", "bp_pull_kernel<sparse, count>", "bp_count_kernel<side rows>"
STREAM, FOLD = "xp_stream_kernel", "xp_fold_kernel"
WIDTHS = (64, 128, 1024)

# id: (heavy, options, scopes that must run, scopes that must not, widths)
MID = {
    "1 heavy": (True, {}, [DENSE], [SPARSE, GROUPS], WIDTHS + (2048,)),
    "2 light, no row groups": (False, {"expand_row_groups": 0}, [SPARSE], [GROUPS, DENSE], WIDTHS + (2048,)),
    "3 light, no records": (False, {"expand_records": 0}, [SPARSE, GROUPS], [RECORDS, ITEM_REC, DENSE], WIDTHS),
    "4 light": (False, {}, [SPARSE, GROUPS, RECORDS, ITEM_REC], [DENSE], WIDTHS),
}
# id: (heavy, dirty, options, must run, must not run, widths); the partitioned rows at one word: see the docstring
COUNT = {
    "5 heavy, plain, clean": (True, False, {"expand_xcd": 0}, [DENSE_COUNT], [SPARSE_COUNT, STREAM, FOLD], WIDTHS + (2048,)),
    "6 heavy, plain, dirty": (True, True, {"expand_xcd": 0}, [DENSE_COUNT, SIDE], [SPARSE_COUNT, STREAM, FOLD], WIDTHS),
    "7 light, clean": (False, False, {}, [SPARSE_COUNT], [DENSE_COUNT, STREAM, FOLD], WIDTHS),
    "7 light, dirty": (False, True, {}, [SPARSE_COUNT, SIDE], [DENSE_COUNT, STREAM, FOLD], WIDTHS),
    "8 heavy, partitioned, clean": (True, False, {}, [STREAM, FOLD], [SIDE, DENSE_COUNT, SPARSE_COUNT], WIDTHS),
    "9 heavy, partitioned, dirty": (True, True, {}, [STREAM, FOLD, SIDE], [DENSE_COUNT, SPARSE_COUNT], WIDTHS),
}


def params(table):
    return [pytest.param(k, nsrc, id="%s-%d" % (k, nsrc)) for k, row in table.items() for nsrc in row[-1]]


@pytest.fixture(scope="module")
def cases():
    made = {}

    def get(nsrc, heavy):
        if (nsrc, heavy) not in made:
            c = made[(nsrc, heavy)] = Case(N_BASE, nsrc, heavy=heavy, cover=True)
            # the forms the rows below name, from the graph (a delta entry moves a count by one: the margins are 16)
            n1, n2 = c.nonzero_rows(1), c.nonzero_rows(2)
            assert (n1 * 8 >= c.n + 16 and n2 * 8 >= c.n + 16) if heavy else (n1 * 8 < c.n - 16 and n2 * 8 < c.n - 16), (n1, n2)
        return made[(nsrc, heavy)]

    yield get
    for c in made.values():
        c.free()


def run(ctx, opts, call):
    """call() under the forced options; its result and the launches by profiler scope."""
    with Forced(ctx, **opts):
        ctx.prof_enable(True)
        try:
            out = call()
            launches = {p["kernel"]: p["launches"] for p in ctx.prof_read()}
        finally:
            ctx.prof_enable(False)
    return out, launches


def check_scopes(launches, must, must_not):
    print({k: launches.get(k, 0) for k in must + must_not})
    for k in must:
        assert launches.get(k, 0) >= 1, (k, sorted(launches))
    for k in must_not:
        assert k not in launches, (k, sorted(launches))


@pytest.mark.parametrize("row,nsrc", params(MID))
def test_mid_chain_hop(ctx, cases, row, nsrc):
    heavy, opts, must, must_not, _ = MID[row]
    case = cases(nsrc, heavy)
    want, want_flops = case.refs()["mat"]
    a, _, _ = case.device(ctx)

    def call():
        m, flops = engine.expand_mat(ctx, case.src, [a] * 2)
        rp, ci, _ = m.export_csr()
        m.free()
        return np.asarray(rp).astype(U64), np.asarray(ci).astype(U64), flops

    (rp, ci, flops), launches = run(ctx, opts, call)
    assert np.array_equal(rp, want.rowptr.astype(U64))
    assert np.array_equal(ci, want.colidx.astype(U64))
    assert flops == want_flops
    check_scopes(launches, must, must_not)


@pytest.mark.parametrize("checksum", [True, False], ids=["checksum", "count"])
@pytest.mark.parametrize("row,nsrc", params(COUNT))
def test_count_hop(ctx, cases, row, nsrc, checksum):
    heavy, dirty, opts, must, must_not, _ = COUNT[row]
    case = cases(nsrc, heavy)
    want = case.refs()["count dirty" if dirty else "count"]
    a, dp, dm = case.device(ctx)
    layers = ([a] * 3, [dp] * 3, [dm] * 3) if dirty else ([a] * 3,)
    got, launches = run(ctx, opts, lambda: engine.expand_count(ctx, case.src, *layers, want_checksum=checksum))
    assert got[0] == want[0] and got[2] == want[2], (got, want)
    if checksum:
        assert got[1] == want[1], (got, want)
    if STREAM in must and nsrc == 64:   # 8-byte rows keep the plain pull, which cuts rows into items: its touched rows are counted
        must = [DENSE_COUNT, SIDE]
        must_not = [STREAM, FOLD, SPARSE_COUNT]
    check_scopes(launches, must, must_not)
    # the mid-chain hop before a heavy count is the dense one, before a light count the sparse one
    check_scopes(launches, [DENSE] if heavy else [SPARSE], [SPARSE] if heavy else [DENSE])
