"""The mid-chain hop over a light state when records answer the flag probe (bitexpand.hip: bp_records_kernel writes a record
for EVERY vertex, bp_pull_groups_kernel<.., true> and bp_pull_items_rec_kernel read them behind the LDS flag map).

One constructed graph carries every case; its state after hop 1 is decided by the edges out of the sources, so which vertices
are flagged and how many bits each holds is read off the graph:

  - n = 3 * 2048 + 37: a records tile and a flag word both end part-way; vertex n - 1 is flagged and feeds a split row
  - split rows (more than 256 in-edges: the item kernel's) of in-degree 257, 300, 512 and 600, a group row of exactly 256
  - the 512 row's first item holds unflagged neighbours only, its second item flagged ones only; every other split row mixes
  - flagged vertices with exactly 1, 4, 5 and 17 bits (the record boundary and BP_REC_ESC), each feeding a split and a group row,
    with bits in the first and the last word of the row
  - unflagged neighbours next to a flagged vertex in their map block (they pass the map and must read ~0ull) and in blocks
    with none
  - hop 1 is light enough to be pushed, so hop 2 is the chain's one mid-chain pull: the profiler scopes asserted below are its

The second graph has the same shape on 2^24 + 5 vertices: a block of the 32 KiB map is then 128 vertices (cshift 7), two flag
words, where the base graph's is 8 (cshift 3, the smallest).  The map builder has one form for every shift, so these are its
two ends rather than two branches.
"""
import os
import sys

import numpy as np
import pytest

from falkordb_amd import engine

pytestmark = pytest.mark.gpu
U64 = np.uint64

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from hop_graph import N_BASE, N_LARGE, Case, Forced  # noqa: E402

ITEM_REC, RECORDS = "bp_pull_items_rec_kernel", "bp_records_kernel"


@pytest.fixture(scope="module")
def cases():
    made = {}

    def get(n, nsrc):
        if (n, nsrc) not in made:
            made[(n, nsrc)] = Case(n, nsrc)
        return made[(n, nsrc)]

    yield get
    for c in made.values():
        c.free()


def run(ctx, records, call):
    """call() under the forced path with expand_records = records; the launches by profiler scope next to its result."""
    with Forced(ctx, expand_records=records):
        ctx.prof_enable(True)
        try:
            out = call()
            launches = {p["kernel"]: p["launches"] for p in ctx.prof_read()}
        finally:
            ctx.prof_enable(False)
    print("records", records, {k: v for k, v in launches.items() if k in (ITEM_REC, RECORDS)})
    if records:
        assert launches.get(ITEM_REC, 0) >= 1 and launches.get(RECORDS, 0) >= 1, sorted(launches)
    else:
        assert ITEM_REC not in launches and RECORDS not in launches, sorted(launches)
    return out


def materialised(ctx, case, records):
    a, _, _ = case.device(ctx)

    def call():
        m, flops = engine.expand_mat(ctx, case.src, [a] * 2)
        rp, ci, _ = m.export_csr()
        m.free()
        return np.asarray(rp).astype(U64), np.asarray(ci).astype(U64), flops

    return run(ctx, records, call)


SHAPES = [(N_BASE, 64), (N_BASE, 128), (N_BASE, 256), (N_BASE, 512), (N_BASE, 1024), (N_LARGE, 64)]


@pytest.mark.parametrize("n,nsrc", SHAPES)
def test_two_hops_materialised(ctx, cases, n, nsrc):
    case = cases(n, nsrc)
    want, want_flops = case.refs()["mat"]
    got = {r: materialised(ctx, case, r) for r in (1, 0)}
    for r, (rp, ci, flops) in got.items():
        assert np.array_equal(rp, want.rowptr.astype(U64)), r
        assert np.array_equal(ci, want.colidx.astype(U64)), r
        assert flops == want_flops, r
    assert all(np.array_equal(x, y) for x, y in zip(got[1][:2], got[0][:2]))


@pytest.mark.parametrize("dirty", [False, True], ids=["clean", "dirty"])
@pytest.mark.parametrize("n,nsrc", SHAPES)
def test_three_hops_counted(ctx, cases, n, nsrc, dirty):
    case = cases(n, nsrc)
    want = case.refs()["count dirty" if dirty else "count"]
    a, dp, dm = case.device(ctx)
    layers = ([a] * 3, [dp] * 3, [dm] * 3) if dirty else ([a] * 3,)
    got = {r: run(ctx, r, lambda: engine.expand_count(ctx, case.src, *layers)) for r in (1, 0)}
    assert got[1] == tuple(want), (got[1], want)
    assert got[0] == tuple(want), (got[0], want)
