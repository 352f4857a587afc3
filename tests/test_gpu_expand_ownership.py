"""GPU: no entry of the k-hop chain keeps device memory past its call, whichever way the chain ends.

Every call below runs once to warm the caches that attach to the input matrices (cached transposes, work-item lists, the
partitioned layouts of the count hop) and to the lanes (pools, staging), then `device_bytes()` is read, the call runs again,
what it returned is freed, and `in_use` must be back at the value read, the second result equal to the first.  The graph is
the smallest at which bp_to_csr takes its sort path (4096 vertices); the 130 source rows make more than two words of bits per
vertex, and enough of them are empty (UINT64_MAX) or without out-edges for compact_source_rows to run."""
import numpy as np
import pytest

from falkordb_amd import _ffi, engine

pytestmark = pytest.mark.gpu

N = 4096          # vertices: bp_to_csr sorts from here up
NEDGES = 32768
NLAYER = 300      # entries of dp and of dm
NOOUT = 64        # vertices 0 .. 63 have no out-edge in any layer
NONE = 2**64 - 1


class _Graph:
    def __init__(self, ctx):
        rng = np.random.default_rng(0x0511E12)
        rows = rng.integers(NOOUT, N, NEDGES, dtype=np.uint64)
        cols = rng.integers(0, N, NEDGES, dtype=np.uint64)
        self.M = ctx.mat_from_coo(N, N, rows, cols)
        pick = rng.choice(NEDGES, NLAYER, replace=False)
        self.DM = ctx.mat_from_coo(N, N, rows[pick], cols[pick])           # tombstones of existing edges
        self.DP = ctx.mat_from_coo(N, N, rng.integers(NOOUT, N, NLAYER, dtype=np.uint64), rng.integers(0, N, NLAYER, dtype=np.uint64))
        # 130 source rows: 8 left empty, 10 on vertices without out-edges, the rest on vertices that have some
        src = rng.choice(np.unique(rows), 130, replace=False).astype(np.uint64)
        src[[3, 17, 40, 64, 65, 100, 128, 129]] = NONE
        src[[0, 9, 31, 63, 66, 77, 90, 101, 120, 127]] = np.arange(10, dtype=np.uint64) * 5
        self.src = src
        self.live_src = rng.choice(np.unique(rows), 130, replace=False).astype(np.uint64)   # every row has out-edges
        self.dst = rng.integers(0, N, 130, dtype=np.uint64)               # pre-bound destinations of the probe
        pin = np.full(130, NONE, dtype=np.uint64)
        pin[::3] = self.dst[::3]
        self.pin = pin
        self.label = rng.integers(0, 2**64, N // 64, dtype=np.uint64)          # about half of the vertices carry the label

    def layers(self, dirty, hops):
        return [self.M] * hops, ([self.DP] * hops if dirty else None), ([self.DM] * hops if dirty else None)


@pytest.fixture(scope="module")
def graph(ctx):
    g = _Graph(ctx)
    yield g
    for m in (g.M, g.DP, g.DM):
        m.free()


def _plain(x):
    """a call's result as something `==` compares: arrays as bytes, containers element-wise"""
    if isinstance(x, np.ndarray):
        return (str(x.dtype), x.shape, x.tobytes())
    if isinstance(x, (tuple, list)):
        return tuple(_plain(v) for v in x)
    if isinstance(x, dict):
        return tuple((k, _plain(v)) for k, v in sorted(x.items()))
    return x


def _expand_mat(ctx, *a, **kw):
    m, flops = engine.expand_mat(ctx, *a, **kw)
    out = (m.export_csr()[:2], flops)
    m.free()
    return out


def _stream(ctx, *a, read=True, **kw):
    s = engine.ExpandStream(ctx, *a, chunk_rows=16, **kw)   # 130 rows: 9 chunks over the 4 slots
    got = [(first, rp.copy(), d.copy()) for first, rp, d in s] if read else []
    out = (s.nnz, s.flops, got)
    s.close()
    return out


def held_and_steady(ctx, call):
    """`call` warmed, then run again between two readings of in_use: nothing is kept, and it answers the same"""
    first = _plain(call())
    ctx.sync()
    in_use, _ = ctx.device_bytes()
    second = _plain(call())
    ctx.sync()
    assert ctx.device_bytes()[0] == in_use
    assert second == first
    return first


@pytest.mark.parametrize("dirty", [False, True], ids=["clean", "dirty"])
@pytest.mark.parametrize("labelled", [False, True], ids=["all", "label"])
@pytest.mark.parametrize("mode", [1, 2, 0])
def test_chain_entries_give_back_what_they_allocate(ctx, graph, mode, labelled, dirty):
    g = graph
    lab = g.label if labelled else None
    with ctx.options(expand_mode=mode):
        for hops in (2, 3):
            m, dp, dm = g.layers(dirty, hops)
            kw = dict(dp=dp, dm=dm, dst_label_bitmap=lab)
            held_and_steady(ctx, lambda: engine.expand(ctx, g.src, m, **kw))
            held_and_steady(ctx, lambda: engine.expand32(ctx, g.src, m, **kw))
            held_and_steady(ctx, lambda: _expand_mat(ctx, g.src, m, **kw))
            held_and_steady(ctx, lambda: engine.expand_pairs(ctx, g.src, m, **kw))
            held_and_steady(ctx, lambda: engine.expand_pairs(ctx, g.src, m, pinned_dest=g.pin, row_bits=32, **kw))
            held_and_steady(ctx, lambda: engine.expand_probe(ctx, g.src, g.dst, m, **kw))
            held_and_steady(ctx, lambda: _stream(ctx, g.src, m, **kw))
            held_and_steady(ctx, lambda: _stream(ctx, g.src, m, read=False, **kw))
        m, dp, dm = g.layers(dirty, 3)
        held_and_steady(ctx, lambda: engine.expand_levels(ctx, g.src, m, dp=dp, dm=dm, dst_label_bitmap=lab))
    # whatever form the chain ran in, it reaches what the sorted-CSR products (mode 1) reach
    m, dp, dm = g.layers(dirty, 2)
    with ctx.options(expand_mode=1):
        rp, dest, _ = engine.expand(ctx, g.src, m, dp=dp, dm=dm, dst_label_bitmap=lab)
    with ctx.options(expand_mode=mode):
        rp2, dest2, _ = engine.expand32(ctx, g.src, m, dp=dp, dm=dm, dst_label_bitmap=lab)
    assert np.array_equal(rp, rp2.astype(np.uint64)) and np.array_equal(dest, dest2.astype(np.uint64))


@pytest.mark.parametrize("dirty", [False, True], ids=["clean", "dirty"])
@pytest.mark.parametrize("labelled", [False, True], ids=["all", "label"])
@pytest.mark.parametrize("mode", [1, 2, 0])
def test_count_gives_back_what_it_allocates_at_every_end(ctx, graph, mode, labelled, dirty):
    g = graph
    lab = g.label if labelled else None
    want = None
    for fuse in (0, 1):
        with ctx.options(expand_mode=mode, expand_fuse_count=fuse):
            for hops in (2, 3):
                m, dp, dm = g.layers(dirty, hops)
                kw = dict(dp=dp, dm=dm, dst_label_bitmap=lab)
                full = held_and_steady(ctx, lambda: engine.expand_count(ctx, g.src, m, **kw))
                bare = held_and_steady(ctx, lambda: engine.expand_count(ctx, g.src, m, want_checksum=False, **kw))
                assert bare[0] == full[0] and bare[1] == 0
                if hops == 3:
                    want = want or full
                    assert full[:2] == want[:2]          # fused or not: the same count and checksum


@pytest.mark.parametrize("dirty", [False, True], ids=["clean", "dirty"])
def test_whole_frontier_count_gives_back_what_it_allocates(ctx, graph, dirty):
    """fgpu_expand_count through expand_count_scan: 64-row passes dealt to two lanes (the calling thread's and a worker's).
    The mixed sources leave 112 live rows, two passes; the all-live ones make three."""
    g = graph
    m, dp, dm = g.layers(dirty, 3)
    for src, passes in ((g.src, 2), (g.live_src, 3)):
        want = engine.expand_count(ctx, src, m, dp=dp, dm=dm)
        with ctx.options(expand_scan_min=64, expand_scan_rows=64, expand_scan_lanes=2):
            for cs in (True, False):
                got = held_and_steady(ctx, lambda: engine.expand_count(ctx, src, m, dp=dp, dm=dm, want_checksum=cs))
                assert ctx.get_option("expand_scan_last_passes") == passes
                assert got[0] == want[0] and got[1] == (want[1] if cs else 0)


@pytest.mark.parametrize("dirty", [False, True], ids=["clean", "dirty"])
def test_trail_counts_give_back_what_they_allocate(ctx, graph, dirty):
    g = graph
    src = g.live_src                                       # (every row needs a source)
    for hops in (1, 2):
        m, dp, dm = g.layers(dirty, hops)
        held_and_steady(ctx, lambda: engine.expand_trail_counts(ctx, src, m, dp=dp, dm=dm))


def test_an_error_after_the_merged_layers_were_built_keeps_nothing(ctx, graph):
    """weighted trail counts over dirty PATTERN layers: FGPU_INVALID once the merged layers exist (they carry no counts)"""
    g = graph
    m, dp, dm = g.layers(True, 2)
    want = _plain(engine.expand_trail_counts(ctx, g.live_src, m, dp=dp, dm=dm))
    ctx.sync()
    in_use, _ = ctx.device_bytes()
    for _ in range(2):
        with pytest.raises(_ffi.FgpuError) as e:
            engine.expand_trail_counts(ctx, g.live_src, m, dp=dp, dm=dm, weighted=True)
        assert e.value.code == _ffi.FGPU_INVALID
        ctx.sync()
        assert ctx.device_bytes()[0] == in_use
    assert _plain(engine.expand_trail_counts(ctx, g.live_src, m, dp=dp, dm=dm)) == want
    ctx.sync()
    assert ctx.device_bytes()[0] == in_use
