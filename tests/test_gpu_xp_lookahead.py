"""The stream kernel of the XCD-partitioned count hop with its look-ahead carried into the wavefront's next chunk
(bitpart.hip xp_stream_kernel<.., LA>, option expand_xp_lookahead; expand_xp_stream_wgs caps its workgroups per partition).

A wavefront takes chunks j, j + nwaves, ... of its partition.  With the look-ahead on, the column words and gathers that the last
iteration of chunk j issues ahead are the first two trips of chunk j + nwaves, so what can go wrong is decided by how long a chunk
is (an even or an odd last trip, with or without copies in it), by how short the NEXT chunk is (shorter than a trip, than two),
by whether there is a next chunk at all, and by runs that cross the boundary (their rows meet through atomics).  The graphs below
construct those chunks: the plan's cut is modelled in numpy from the graph (`stream_model`), the constructed lengths are asserted
on the model, and the model's chunk and shared-row counts are asserted against the plan's (expand_xp_last_chunks,
expand_xp_last_shared_rows).

Every case compares (nnz, checksum, flops) of engine.expand_count with the CPU oracle, under expand_xp_lookahead 1 and 0, and
asserts xp_stream_kernel among the profiled kernels.  Sources: 128, 256, 512 and 1024 (rows of 2, 4, 8 and 16 words: QL 1, 2, 4
and 8); 64 sources make one-word rows, which the partitioned form does not take (bitexpand.hip bp_xcd_applies) — that case
asserts the oracle's result and that the plain pull ran."""
import os
import sys

import numpy as np
import pytest

import oracle
from falkordb_amd import FgpuError, engine

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_xp_direct import Forced, device, partition_of_rows  # noqa: E402
from test_gpu_xp_direct import small_graph  # noqa: E402,F401  (the fixture: 8192 vertices, the ranked plan)
from test_gpu_xp_shapes import Refs, build_partition_cases, deltas, launched, prange_of  # noqa: E402

pytestmark = pytest.mark.gpu
U64, I64 = np.uint64, np.int64
XP_SPAN, XP_RUNW, XP_RUNS = 768, 8, 96          # bitpart.hip


# ---- the plan's cut, in numpy ----------------------------------------------------------------------------------------------------
def key_cut(runs):
    """Chunk id = (entry index + XP_RUNW x run index) // XP_SPAN, both counted inside the partition: the chunks' lengths."""
    key = np.arange(runs.sum(), dtype=I64) + XP_RUNW * np.repeat(np.arange(len(runs), dtype=I64), runs)
    return np.bincount(key // XP_SPAN)


def cell_cut(runs):
    """Super-cells of 640 entries from the partition's first entry: one chunk when it touches at most XP_RUNS runs, else its
    128-entry cells.  None when a cell that has to stand alone touches more runs than that."""
    n = int(runs.sum())
    run_of = np.repeat(np.arange(len(runs), dtype=I64), runs)
    touch = lambda b, e: int(run_of[e - 1] - run_of[b]) + 1
    lens = []
    for s0 in range(0, n, 640):
        s1 = min(s0 + 640, n)
        if touch(s0, s1) <= XP_RUNS:
            lens.append(s1 - s0)
            continue
        for c0 in range(s0, s1, 128):
            c1 = min(c0 + 128, s1)
            if touch(c0, c1) > XP_RUNS:
                return None
            lens.append(c1 - c0)
    return np.array(lens, dtype=I64)


class Part:
    """One partition of the model: the streamed runs and its chunks (start and length in entries from the partition's first,
    the run of the first entry counted inside the partition, and whether the chunk begins inside that run)."""

    def __init__(self, runs, lens):
        self.runs, self.lens = runs, lens
        self.starts = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(I64) if len(lens) else np.zeros(0, dtype=I64)
        run_starts = np.concatenate([[0], np.cumsum(runs)[:-1]]).astype(I64) if len(runs) else np.zeros(0, dtype=I64)
        self.run0 = np.searchsorted(run_starts, self.starts, side="right") - 1
        self.shared = (~np.isin(self.starts, run_starts)).astype(I64)
        ends = self.starts + lens - 1
        self.touched = np.searchsorted(run_starts, ends, side="right") - 1 - self.run0 + 1


def stream_model(a: oracle.CSR, direct, part=None, cut=0):
    """(the cut the plan must hold, [Part] * 8) of the plan over `a`: the runs of every partition (rows of A' ascending, the
    single-entry ones taken out under `direct`) and the chunks the asked-for cut makes of them — the key cut for the WHOLE plan
    when one cell of the cell cut would exceed the tile.  `part`: partition of every row of X (default: u // prange)."""
    rows, cols = (x.astype(I64) for x in a.pairs())
    if part is None:
        part = np.arange(a.nrows, dtype=I64) // prange_of(a.nrows)
    cnt = np.bincount(part[rows] * a.ncols + cols, minlength=8 * a.ncols).reshape(8, a.ncols)
    runs = [cnt[k][cnt[k] > (1 if direct else 0)] for k in range(8)]
    lens = [cell_cut(r) if len(r) else np.zeros(0, dtype=I64) for r in runs] if cut else None
    held = 1 if cut and all(l is not None for l in lens) else 0
    if not held:
        lens = [key_cut(r) if len(r) else np.zeros(0, dtype=I64) for r in runs]
    parts = [Part(r, l) for r, l in zip(runs, lens)]
    for p in parts:
        assert len(p.lens) == 0 or (p.lens.min() > 0 and p.lens.max() <= XP_SPAN and p.touched.max() <= XP_RUNS)
        if held and len(p.lens) > 1:
            assert np.all(p.lens[:-1] % 128 == 0)
    return held, parts


def plan_counts(model):
    return sum(len(p.lens) for p in model[1]), sum(int(p.shared.sum()) for p in model[1])


def check_table(tab, model):
    """The chunk table read back from the plan against the model, chunk for chunk; under the cell cut every chunk but a
    partition's last holds a multiple of 128 entries, and no chunk touches more runs than the tile has rows (the model's own
    assertions, which the equality hands on to the plan)."""
    held, parts = model
    assert tab["cut"] == held
    run_base = 0
    for k, p in enumerate(parts):
        c0, c1 = int(tab["cbase"][k]), int(tab["cbase"][k + 1])
        assert c1 - c0 == len(p.lens), (k, c1 - c0, len(p.lens))
        assert int(tab["pstart"][k + 1]) - int(tab["pstart"][k]) == int(p.runs.sum()), k
        np.testing.assert_array_equal(tab["cstart"][c0:c1].astype(I64) - int(tab["pstart"][k]), p.starts)
        np.testing.assert_array_equal(tab["crun0"][c0:c1].astype(I64) - run_base, p.run0)
        np.testing.assert_array_equal(tab["cshared"][c0:c1].astype(I64), p.shared)
        run_base += len(p.runs)


# ---- running a case ----------------------------------------------------------------------------------------------------------------
def count_both(ctx, src, layers, dev, tag, models=None, direct=1, stream=True, label=None, **options):
    """expand_count under expand_xp_lookahead 1 / 0 x expand_xp_cut 1 / 0 against oracle.expand_summary_omp; the stream kernel
    ran (or, stream = False, did not); the plan holds its model's chunks and shared rows.  models = {cut: stream_model}."""
    want = oracle.expand_summary_omp(src, layers, chunk=1024)[:3]
    kw = {}
    if label is not None:
        refs = Refs(src, layers, label)
        assert refs.full == want
        want, kw = refs.lab, dict(dst_label_bitmap=refs.label_bits)
    got = {}
    for cut in (1, 0):
        for la in (1, 0):
            with Forced(ctx, direct, expand_xp_lookahead=la, expand_xp_cut=cut, **options):
                with launched(ctx) as names:
                    got[cut, la] = engine.expand_count(ctx, src, *dev, **kw)
                print(tag, "cut", cut, "lookahead", la, options, got[cut, la], want, sorted(n for n in names if n.startswith("xp_")))
                assert ("xp_stream_kernel" in names) == stream, (tag, cut, la, sorted(names))
                if stream and models is not None:
                    seen = (ctx.get_option("expand_xp_last_chunks"), ctx.get_option("expand_xp_last_shared_rows"))
                    assert seen == plan_counts(models[cut]), (tag, cut, seen)
    for k, g in got.items():
        assert g == want, (tag, "cut, lookahead", k)


def models_of(a, direct, part=None):
    return {cut: stream_model(a, direct, part, cut) for cut in (0, 1)}


def tables_match(ctx, A, models, direct=1):
    for cut in (0, 1):
        with Forced(ctx, direct, expand_xp_cut=cut):
            check_table(A.xp_chunks(), models[cut])


def layers_of(a, dp, dm, hops, dirty):
    host = [(a, dp, dm) if dirty else (a, None, None)] * hops
    return host, lambda A, DP, DM: ([A] * hops, [DP] * hops if dirty else None, [DM] * hops if dirty else None)


# ---- one workgroup per partition on 8192 vertices -----------------------------------------------------------------------------------
@pytest.mark.parametrize("dirty", [False, True])
def test_one_workgroup_per_partition_walks_many_chunks(ctx, small_graph, dirty):
    """8192 vertices of out-degree 16 and one in-hub (a run of 1024 entries in each partition), the ranked plan.  With one
    workgroup per partition each of its four wavefronts walks ten chunks and more, every one but the last opened by the chunk
    before it; the default grid gives every wavefront at most one chunk, so no chunk has a next one."""
    a, dp, dm, label_ids = small_graph
    n = a.nrows
    src = np.arange(0, n, n // 600, dtype=U64)[:600]
    src = src[src != 200]
    model = models_of(a, 1, partition_of_rows(a))
    per_part = [len(p.lens) for p in model[0][1]]
    assert min(per_part) >= 40 and plan_counts(model[0])[1] >= 8       # >= 10 chunks a wavefront; the hub's runs are shared rows
    assert model[1][0] == 1 and plan_counts(model[1])[1] > plan_counts(model[0])[1]
    A, DP, DM = device(ctx, a), device(ctx, dp), device(ctx, dm)
    if not dirty:
        tables_match(ctx, A, model)
    host, dev = layers_of(a, dp, dm, 3, dirty)
    for wgs in (1, 0, 3):
        count_both(ctx, src, host, dev(A, DP, DM), ("8192", dirty, wgs), model, expand_xp_stream_wgs=wgs)
    if dirty:
        count_both(ctx, src, host, dev(A, DP, DM), ("8192 label", dirty), model, label=label_ids, expand_xp_stream_wgs=1)
    # two hops, the result the oracle materialises
    host2, dev2 = layers_of(a, dp, dm, 2, dirty)
    refs = Refs(src, host2, label_ids)
    assert refs.dense
    for cut in (1, 0):
        for la in (1, 0):
            with Forced(ctx, 1, expand_xp_lookahead=la, expand_xp_cut=cut, expand_xp_stream_wgs=1):
                with launched(ctx) as names:
                    assert engine.expand_count(ctx, src, *dev2(A, DP, DM)) == refs.full, ("two hops", cut, la)
                assert "xp_stream_kernel" in names


# ---- constructed chunks ------------------------------------------------------------------------------------------------------------
SN = 32_837             # no multiple of 128: the rows of X keep vertex order, partition(u) = u // 4112
SPR = 4112
BG_LO = 1024            # background destinations are ids >= BG_LO; the scripted ones are 0 .. (rows of A' ascend: they come FIRST)
HUB_V = 0
TAILS = (1, 63, 64, 65)                         # entries of the last chunk of partitions 0 .. 3
HEADS = {4: (15, 610), 5: (15, 611), 6: (7, 690), 7: (7, 691)}   # partition: (two-entry runs, then one long run) = chunk 0
HEAD_LEN = {4: 640, 5: 641, 6: 704, 7: 705}     # 128 k, 128 k + 1, 128 k + 64, 128 k + 65 entries


def scripted(scripts, bg_parts, seed, bg_deg=16):
    """scripts[k][i] in-neighbours of destination i in partition k (the TOP rows of the partition), and bg_deg random
    out-edges into ids >= BG_LO from every vertex of the partitions `bg_parts`.  A partition outside bg_parts streams its
    scripted runs and nothing else; one inside streams them first."""
    assert prange_of(SN) == SPR and SN % 128
    rng = np.random.default_rng(seed)
    rows, cols = [], []
    for k, runs in scripts.items():
        top = min((k + 1) * SPR, SN)
        for i, length in enumerate(runs):
            assert i < BG_LO and length <= 3200
            rows.append(top - 1 - np.arange(length, dtype=I64))
            cols.append(np.full(length, i, dtype=I64))
    for k in bg_parts:
        us = np.arange(k * SPR, min((k + 1) * SPR, SN), dtype=I64)
        rows.append(np.repeat(us, bg_deg))
        cols.append(rng.integers(BG_LO, SN, len(us) * bg_deg))
    a = oracle.build_csr(SN, SN, np.concatenate(rows).astype(U64), np.concatenate(cols).astype(U64))
    return a


def scripted_sources(nsrc, bg_parts):
    lo = min(bg_parts) * SPR
    ids = lo + (np.arange(nsrc, dtype=I64) * (SN - lo)) // nsrc
    ids[-1] = SN - 1
    assert len(np.unique(ids)) == nsrc
    return ids.astype(U64)


def build_chunk_shapes():
    """Partitions 0 .. 3 stream ONE run each, the in-hub 0's: 4 x 768 + r entries, five chunks, the last of r = 1, 63, 64, 65
    entries, every boundary inside the run.  Partitions 4 .. 7 open with two-entry runs and a long one that the key cut closes
    at 640, 641, 704 and 705 entries, then stream the background."""
    scripts = {k: [4 * XP_SPAN + r] for k, r in enumerate(TAILS)}
    for k, (twos, long_run) in HEADS.items():
        scripts[k] = [0] + [2] * twos + [long_run]
    a = scripted(scripts, (4, 5, 6, 7), 0x18A)
    hub_in = [int(u) for u in oracle.transpose(a).row(HUB_V)[:2]]
    # a tombstone and a pending add on the in-hub, whose partial rows are shared rows in partitions 0 .. 3
    dp, dm = deltas(a, 0x18B, banned=range(BG_LO), dm_first=[(hub_in[0], HUB_V)], dp_first=[(5 * SPR + 7, HUB_V)])
    model = {d: models_of(a, d) for d in (0, 1)}
    for d in (0, 1):
        for k, r in enumerate(TAILS):
            p = model[d][0][1][k]
            assert list(p.runs) == [4 * XP_SPAN + r] and list(p.lens) == [XP_SPAN] * 4 + [r] and p.shared.sum() == 4
            q = model[d][1][1][k]                # the cell cut: four super-cells of 640, then 512 + r entries — no multiple of 128
            assert list(q.lens) == [640] * 4 + [512 + r] and q.shared.sum() == 4
        for k, want in HEAD_LEN.items():
            p = model[d][0][1][k]
            assert p.lens[0] == want and len(p.lens) >= 20, (k, p.lens[:3])
            assert p.runs[HEADS[k][0]] == HEADS[k][1] and p.runs[:HEADS[k][0]].tolist() == [2] * HEADS[k][0]
        assert model[d][1][0] == 1
    return a, dp, dm, model


@pytest.fixture(scope="module")
def chunk_shapes():
    return build_chunk_shapes()


@pytest.mark.parametrize("dirty", [False, True])
@pytest.mark.parametrize("nsrc", [128, 256, 512, 1024])
def test_constructed_chunks(ctx, chunk_shapes, nsrc, dirty):
    """With one workgroup per partition wavefront 0 of partitions 0 .. 3 takes chunk 0 and chunk 4: its look-ahead lands in a
    chunk of 1, 63, 64 or 65 entries, inside the run it is itself a piece of.  In partitions 4 .. 7 it takes chunk 0 of 640 /
    641 / 704 / 705 entries (an odd trip that is padding alone, one entry, a full even trip, an even trip and one entry) and
    then chunk 4.  The default grid gives every wavefront one chunk.  Dirty: a tombstone and a pending add name the in-hub."""
    a, dp, dm, model = chunk_shapes
    src = scripted_sources(nsrc, (4, 5, 6, 7))
    A, DP, DM = device(ctx, a), device(ctx, dp), device(ctx, dm)
    host, dev = layers_of(a, dp, dm, 3, dirty)
    if nsrc == 128 and not dirty:
        tables_match(ctx, A, model[1])
        tables_match(ctx, A, model[0], direct=0)
    for wgs in (1, 0):
        count_both(ctx, src, host, dev(A, DP, DM), ("chunks", nsrc, dirty, wgs), model[1], expand_xp_stream_wgs=wgs)
    if nsrc == 512:
        count_both(ctx, src, host, dev(A, DP, DM), ("chunks direct 0", dirty), model[0], direct=0, expand_xp_stream_wgs=1)
        count_both(ctx, src, host, dev(A, DP, DM), ("chunks 2 wgs", dirty), model[1], expand_xp_stream_wgs=2)


def test_one_word_rows_keep_the_plain_pull(ctx, chunk_shapes):
    """64 sources: rows of one word, which the partitioned form does not take — the switches change nothing."""
    a, dp, dm, model = chunk_shapes
    src = scripted_sources(64, (4, 5, 6, 7))
    A = device(ctx, a)
    host, dev = layers_of(a, dp, dm, 3, False)
    count_both(ctx, src, host, dev(A, None, None), ("chunks", 64), stream=False, expand_xp_stream_wgs=1)


def build_sparse_partitions():
    """Partition 0: one run of 300 entries, a single chunk.  Partition 1: no entry, no chunk.  Partition 2: one run of 768
    entries and one of two: under the key cut a second chunk of two entries that begins on a run.  Partition 3: 400 two-entry
    runs, 320 of them in the first super-cell, which the cell cut has to split into 128-entry chunks of 64 runs; then one-entry
    runs, which stay in the stream only under expand_xp_direct = 0 — a cell of 128 runs, more than the tile holds, so THAT plan
    keeps the key cut whole.  Partitions 4 .. 7: the background."""
    a = scripted({0: [300], 2: [0, XP_SPAN, 2], 3: [0, 0, 0] + [2] * 400 + [1] * 300}, (4, 5, 6, 7), 0x18C)
    model = {d: models_of(a, d) for d in (0, 1)}
    key, cell = model[1][0][1], model[1][1][1]
    assert [list(key[k].lens) for k in (0, 1, 2)] == [[300], [], [XP_SPAN, 2]] and key[2].shared.sum() == 0
    assert model[1][1][0] == 1 and list(cell[3].lens) == [128] * 5 + [160] and list(cell[3].touched[:5]) == [64] * 5
    assert [list(cell[k].lens) for k in (0, 1, 2)] == [[300], [], [640, 130]] and cell[2].shared.sum() == 1
    assert model[0][1][0] == 0                               # direct = 0: the cell cut is refused
    assert plan_counts(model[0][1]) == plan_counts(model[0][0])
    return a, model


@pytest.fixture(scope="module")
def sparse_partitions():
    return build_sparse_partitions()


@pytest.mark.parametrize("nsrc", [256, 1024])
def test_partitions_of_one_chunk_and_of_none(ctx, sparse_partitions, nsrc):
    a, model = sparse_partitions
    src = scripted_sources(nsrc, (4, 5, 6, 7))
    A = device(ctx, a)
    host, dev = layers_of(a, None, None, 3, False)
    for direct in (1, 0):
        tables_match(ctx, A, model[direct], direct=direct)   # (direct 0: both plans hold the key cut)
        for wgs in (1, 0):
            count_both(ctx, src, host, dev(A, None, None), ("sparse partitions", nsrc, direct, wgs), model[direct], direct=direct,
                       expand_xp_stream_wgs=wgs)


@pytest.fixture(scope="module")
def tiny_200():
    return build_partition_cases()["tiny"]


@pytest.mark.parametrize("nsrc,hops", [(100, 2), (160, 3)])
def test_200_vertices(ctx, tiny_200, nsrc, hops):
    """The 200-vertex shape of test_gpu_xp_shapes.py: partition 7 has no row of X and no chunk, partition 6 eight rows."""
    a, dp, dm, label_ids = tiny_200
    n = a.nrows
    model = models_of(a, 1)
    key = model[0][1]
    assert len(key[7].lens) == 0 and 0 < len(key[6].lens) < len(key[0].lens)
    ids = (np.arange(nsrc, dtype=I64) * n) // nsrc
    ids[-1] = n - 1
    src = ids.astype(U64)
    A, DP, DM = device(ctx, a), device(ctx, dp), device(ctx, dm)
    for dirty in (False, True):
        host, dev = layers_of(a, dp, dm, hops, dirty)
        for wgs in (1, 0):
            count_both(ctx, src, host, dev(A, DP, DM), ("tiny", nsrc, hops, dirty, wgs), model, expand_xp_stream_wgs=wgs)
    tables_match(ctx, A, model)


def test_switches_are_checked(ctx):
    """A value outside a switch's range is refused by name (the library's own error, naming the option) and changes nothing."""
    for name, bad in (("expand_xp_lookahead", 2), ("expand_xp_lookahead", -1), ("expand_xp_stream_wgs", -1), ("expand_xp_cut", 2),
                      ("expand_xp_cut", -1)):
        before = ctx.get_option(name)
        with pytest.raises(FgpuError, match=name):
            ctx.set_option(name, bad)
        assert ctx.get_option(name) == before
    for name in ("expand_xp_last_chunks", "expand_xp_last_shared_rows"):      # read-only: no such option to set
        with pytest.raises(FgpuError, match="unknown option"):
            ctx.set_option(name, 1)
