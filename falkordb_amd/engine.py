"""Thin Python handles over the C ABI (include/fgpu.h) — test / bench plumbing only.

Everything of substance happens inside libfgpu.so; these classes own handles, convert numpy
arrays to the plain pointers the ABI takes, and raise FgpuError on any non-zero fgpu_info.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import os

import weakref

import numpy as np

from . import _ffi
from ._ffi import FgpuError, check, u64p, u8p, i32p, i64p

U64 = np.uint64


def _u64(x):
    return np.ascontiguousarray(x, dtype=U64)


def _p(a, t=u64p):
    return a.ctypes.data_as(t) if a is not None else None


def _env_options():
    """A/B plumbing for the tools and the test-suite: FGPU_OPTS="name=value,name=value" sets library options on every context this
    process opens (e.g. the whole parity suite under an experiment switch) — the library itself reads no environment for them."""
    opts = []
    for kv in filter(None, os.environ.get("FGPU_OPTS", "").split(",")):
        name, eq, value = kv.partition("=")
        try:
            if not eq or not name.strip():
                raise ValueError
            opts.append((name.strip(), int(value)))
        except ValueError:
            raise ValueError(f"FGPU_OPTS: malformed entry {kv!r}, expected name=integer") from None
    return opts


class Context:
    """fgpu_ctx: one per process+device (matrix::init analogue, matrix.rs:116-185)."""

    def __init__(self, device: int = 0):
        opts = _env_options()         # parsed before anything is opened: a malformed entry leaves no context behind
        self.lib = _ffi.load()
        self._h = C.c_void_p()
        self._live_views = 0          # result arrays handed out as views of library memory (_take) and not yet dropped
        self._close_pending = False
        check(self.lib.fgpu_init(C.byref(self._h), device, None, None))
        try:
            for k, v in opts:
                self.set_option(k, v)
        except Exception:
            self.close()
            raise

    @property
    def handle(self):
        return self._h

    def close(self):
        """fgpu_finalize.  Result arrays are zero-copy views of pinned blocks the context owns: while any of them is alive
        the finalize is put off until the last one is dropped (an array that outlived its context would dangle)."""
        if not self._h:
            return
        if self._live_views > 0:
            self._close_pending = True
            return
        self.lib.fgpu_finalize(self._h)
        self._h = C.c_void_p()
        self._close_pending = False

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def sync(self):
        check(self.lib.fgpu_sync(self._h))

    def set_stream(self, stream_ptr: int | None):
        check(self.lib.fgpu_set_stream(self._h, C.c_void_p(stream_ptr or 0)))

    def set_option(self, name: str, value: int):
        check(self.lib.fgpu_set_option(self._h, name.encode(), int(value)))

    def get_option(self, name: str) -> int:
        v = C.c_int64(0)
        check(self.lib.fgpu_get_option(self._h, name.encode(), C.byref(v)))
        return int(v.value)

    @contextlib.contextmanager
    def options(self, **values):
        """Sets the options in the order given and, on the way out, puts back the values found, in reverse order, whether the
        body returned or raised.  A value refused on entry raises after the options set before it have been put back."""
        found = []
        try:
            for name, value in values.items():
                old = self.get_option(name)
                self.set_option(name, value)
                found.append((name, old))
            yield self
        finally:
            for name, old in reversed(found):
                self.set_option(name, old)

    # ---- multi-GPU communicator (RCCL inside libfgpu.so; dist.hip) ----
    def comm_unique_id(self) -> bytes:
        """ncclGetUniqueId: rank 0 calls it, the launcher's own channel carries the 128 bytes to the other ranks."""
        buf = (C.c_uint8 * 128)()
        check(self.lib.fgpu_comm_unique_id(buf))
        return bytes(buf)

    def comm_init_rank(self, nranks: int, rank: int, uid: bytes):
        buf = (C.c_uint8 * 128).from_buffer_copy(uid)
        check(self.lib.fgpu_comm_init_rank(self._h, nranks, rank, buf))

    def comm_finalize(self):
        check(self.lib.fgpu_comm_finalize(self._h))

    def comm_info(self):
        r, n = C.c_int32(), C.c_int32()
        check(self.lib.fgpu_comm_info(self._h, C.byref(r), C.byref(n)))
        return r.value, n.value

    def prof_enable(self, enable=True):
        """Context-wide kernel profiler (HIP events around the modelled kernels of the non-BFS paths)."""
        check(self.lib.fgpu_prof_enable(self._h, 1 if enable else 0))

    def prof_read(self):
        cap = 64
        names = (C.c_char_p * cap)()
        ms = (C.c_double * cap)()
        launches = (C.c_uint64 * cap)()
        ab = (C.c_uint64 * cap)()
        n = C.c_int()
        check(self.lib.fgpu_prof_read(self._h, names, ms, launches, ab, cap, C.byref(n)))
        return [{"kernel": names[i].decode(), "ms": ms[i], "launches": int(launches[i]), "alg_bytes": int(ab[i])}
                for i in range(n.value)]

    def device_info(self):
        name = C.create_string_buffer(256)
        cus, wave = C.c_int32(), C.c_int32()
        lds, hbm = C.c_int64(), C.c_int64()
        check(self.lib.fgpu_device_info(self._h, name, C.byref(cus), C.byref(wave), C.byref(lds), C.byref(hbm)))
        return {"name": name.value.decode(), "cus": cus.value, "wave": wave.value, "lds_bytes": lds.value,
                "hbm_bytes": hbm.value}

    def device_bytes(self):
        a, b = C.c_uint64(), C.c_uint64()
        check(self.lib.fgpu_device_bytes(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    # ---- helpers to pull caller-owned host buffers back into numpy ----
    def _take(self, ptr, n, dtype=U64):
        """A numpy VIEW of a result array the library handed out (no copy: the arrays of a k-hop batch are hundreds of
        MB); fgpu_free runs when the array — and every view derived from it — is gone."""
        if not ptr or n == 0:
            if ptr:
                self.lib.fgpu_free(self._h, C.cast(ptr, C.c_void_p))
            return np.zeros(0, dtype=dtype)
        addr = C.cast(ptr, C.c_void_p).value
        buf = (C.c_char * (int(n) * np.dtype(dtype).itemsize)).from_address(addr)
        arr = np.frombuffer(buf, dtype=dtype, count=int(n))
        ctx = self                               # (a strong reference: the context outlives its views)
        ctx._live_views += 1

        def release():
            ctx._live_views -= 1
            if ctx._h:
                ctx.lib.fgpu_free(ctx._h, C.c_void_p(addr))
                if ctx._close_pending and ctx._live_views == 0:
                    ctx.close()
        weakref.finalize(buf, release)
        return arr

    def host_array(self, n, dtype):
        """fgpu_host_alloc: a pinned host array from the context's pool, for outputs the caller provides (level[] /
        parent[] of fgpu_bfs): the library fills it by DMA instead of staging + a host copy."""
        p = C.c_void_p()
        check(self.lib.fgpu_host_alloc(self._h, int(n) * np.dtype(dtype).itemsize, C.byref(p)))
        return self._take(p, n, dtype)

    # ---- matrix factories ----
    def mat_new(self, nrows, ncols) -> "Mat":
        h = C.c_void_p()
        check(self.lib.fgpu_mat_new(self._h, C.byref(h), nrows, ncols))
        return Mat(self, h)

    def mat_from_coo(self, nrows, ncols, rows, cols, vals=None) -> "Mat":
        rows, cols = _u64(rows), _u64(cols)
        v = _u64(vals) if vals is not None else None
        h = C.c_void_p()
        check(self.lib.fgpu_mat_from_coo(self._h, C.byref(h), nrows, ncols, _p(rows), _p(cols), _p(v), len(rows)))
        return Mat(self, h)

    def mat_from_csr(self, nrows, ncols, rowptr, colidx, vals=None, hyper_rows=None) -> "Mat":
        rowptr, colidx = _u64(rowptr), _u64(colidx)
        v = _u64(vals) if vals is not None else None
        hr = _u64(hyper_rows) if hyper_rows is not None else None
        h = C.c_void_p()
        check(self.lib.fgpu_mat_from_csr(self._h, C.byref(h), nrows, ncols, len(colidx),
                                         rowptr.ctypes.data_as(C.c_void_p), 64, colidx.ctypes.data_as(C.c_void_p), 64,
                                         _p(v), _p(hr), len(hr) if hr is not None else 0))
        return Mat(self, h)

    def mat_rmat(self, scale, edge_factor=16, seed=None, a16=0, b16=0, c16=0) -> "Mat":
        if seed is None:
            seed = 0x5EED1234 + scale
        h = C.c_void_p()
        check(self.lib.fgpu_mat_rmat(self._h, C.byref(h), scale, edge_factor, seed, a16, b16, c16))
        return Mat(self, h)

    # ---- relationship-emitting traversal (expand_edges.hip) ----
    def multi_new(self, key, off, ids) -> "Multi":
        """fgpu_multi_new: one tensor's multi-edge rows on the device, in fgpu_edges_build's shape (key = src << 32 | dst
        ascending, off[0] = 0, every run at least 2 ascending ids)."""
        key, off, ids = _u64(key).reshape(-1), _u64(off).reshape(-1), _u64(ids).reshape(-1)
        h = C.c_void_p()
        check(self.lib.fgpu_multi_new(self._h, _p(key), _p(off), _p(ids), len(key), C.byref(h)))
        return Multi(self, h)

    def expand_edges(self, from_ids, to_ids, m, dp=None, dm=None, mt_m=None, mt_dp=None, mt_dm=None, multi=None, transposed=False,
                     bidirectional=False, first_only=False, from_bitmap=None, to_bitmap=None, want_pass=False):
        """fgpu_expand_edges: CondTraverse's per-row path for a whole batch.  from_ids / to_ids: node id or None (unbound);
        m .. multi: one entry per relationship type in scan order (Mat / Multi or None; the optional lists may be None whole).
        Returns (row, from, to, id[, pass], stats): numpy views of the engine's result blocks, stats the eight of fgpu.h."""
        enc = lambda v: (1 << 64) - 1 if v is None else int(v)
        f = np.asarray([enc(v) for v in from_ids], dtype=U64)
        t = np.asarray([enc(v) for v in to_ids], dtype=U64)
        assert len(f) == len(t)
        T = len(m)
        arrs = [_hop_arrays(x) if x is not None else None for x in (m, dp, dm, mt_m, mt_dp, mt_dm, multi)]
        assert all(a is None or len(a) == T for a in arrs)
        fb = _u64(from_bitmap) if from_bitmap is not None else None
        tb = _u64(to_bitmap) if to_bitmap is not None else None
        prow, pfrom, pto = _ffi.u32p(), _ffi.u32p(), _ffi.u32p()
        pid, ppass = u64p(), u8p()
        n = C.c_uint64()
        st = (C.c_uint64 * 8)()
        flags = (1 if transposed else 0) | (2 if bidirectional else 0) | (4 if first_only else 0)
        check(self.lib.fgpu_expand_edges(self._h, _p(f), _p(t), len(f), *arrs, T, flags, _p(fb), _p(tb), C.byref(prow),
                                         C.byref(pfrom), C.byref(pto), C.byref(pid), C.byref(ppass) if want_pass else None,
                                         C.byref(n), st))
        cols = [self._take(prow, n.value, np.uint32), self._take(pfrom, n.value, np.uint32),
                self._take(pto, n.value, np.uint32), self._take(pid, n.value, U64)]
        if want_pass:
            cols.append(self._take(ppass, n.value, np.uint8))
        return (*cols, [int(x) for x in st])

    # ---- indegree() / outdegree() (degrees.hip) ----
    def node_degrees(self, nodes, m, dp=None, dm=None, mt_m=None, mt_dp=None, mt_dm=None, multi=None, out=True, incoming=False):
        """fgpu_node_degrees: the relationships that leave (out) and / or enter (incoming) every node of `nodes`; m .. multi as
        for expand_edges.  nodes None is the whole-graph form: position i is node i, for every i below m[0]'s dimension.
        Returns (out, in, stats): uint64 arrays of one entry per position (None for a direction not asked for) and the eight
        stats of fgpu.h."""
        T = len(m)
        arrs = [_hop_arrays(x) if x is not None else None for x in (m, dp, dm, mt_m, mt_dp, mt_dm, multi)]
        assert all(a is None or len(a) == T for a in arrs)
        if nodes is None:
            ids, k = None, (m[0].nrows if T else 0)
        else:
            ids = _u64(nodes).reshape(-1)
            k = len(ids)
        o = np.zeros(k, dtype=U64) if out else None
        i = np.zeros(k, dtype=U64) if incoming else None
        st = (C.c_uint64 * 8)()
        flags = (_ffi.FGPU_DEGREE_OUT if out else 0) | (_ffi.FGPU_DEGREE_IN if incoming else 0)
        check(self.lib.fgpu_node_degrees(self._h, _p(ids), k, *arrs, T, flags, _p(o), _p(i), st))
        return o, i, [int(x) for x in st]

    # ---- variable-length traversal (expand_trails.hip) ----
    def expand_trails(self, starts, dests, m, dp=None, dm=None, mt_m=None, mt_dp=None, mt_dm=None, multi=None, reversed=False,
                      bidirectional=False, paths=False, min_hops=1, max_hops=None, dst_label_bitmap=None, max_items=1 << 22,
                      stats_out=None):
        """fgpu_expand_trails: CondVarLenTraverse for a whole batch.  starts: node ids; dests: None, or per row a node id or
        None (unbound); m .. multi as for expand_edges; max_hops None = unbounded.  Returns (row, from, to, hops[, path_off,
        path_node, path_edge], stats): numpy views of the engine's result blocks, stats the eight of fgpu.h.  stats_out (a
        list) receives the eight whatever the call returns: FGPU_INSUFFICIENT_SPACE raises with the counts so far in it."""
        s = _u64(starts).reshape(-1)
        d = None
        if dests is not None:
            d = np.asarray([(1 << 64) - 1 if v is None else int(v) for v in dests], dtype=U64)
            assert len(d) == len(s)
        T = len(m)
        arrs = [_hop_arrays(x) if x is not None else None for x in (m, dp, dm, mt_m, mt_dp, mt_dm, multi)]
        assert all(a is None or len(a) == T for a in arrs)
        bm = _u64(dst_label_bitmap) if dst_label_bitmap is not None else None
        prow, pfrom, pto, phops, pnode = _ffi.u32p(), _ffi.u32p(), _ffi.u32p(), _ffi.u32p(), _ffi.u32p()
        poff, pedge = u64p(), u64p()
        n = C.c_uint64()
        st = (C.c_uint64 * 8)()
        flags = (1 if reversed else 0) | (2 if bidirectional else 0) | (4 if paths else 0)
        code = self.lib.fgpu_expand_trails(self._h, _p(s), _p(d), len(s), *arrs, T, flags, min_hops,
                                           0xFFFFFFFF if max_hops is None else max_hops, _p(bm), max_items, C.byref(prow),
                                           C.byref(pfrom), C.byref(pto), C.byref(phops), C.byref(poff) if paths else None,
                                           C.byref(pnode) if paths else None, C.byref(pedge) if paths else None, C.byref(n), st)
        if stats_out is not None:
            stats_out[:] = [int(x) for x in st]
        check(code)
        cols = [self._take(prow, n.value, np.uint32), self._take(pfrom, n.value, np.uint32),
                self._take(pto, n.value, np.uint32), self._take(phops, n.value, np.uint32)]
        if paths:
            off = self._take(poff, n.value + 1 if n.value else 0, U64)
            total = int(off[-1]) if n.value else 0
            cols += [off, self._take(pnode, total + n.value, np.uint32), self._take(pedge, max(total, 1) if n.value else 0, U64)[:total]]
        return (*cols, [int(x) for x in st])

    # ---- the algorithms' weighted pair matrix (pair_weights.hip) ----
    def pair_weights(self, m, dp=None, dm=None, multi=None, *, out=True, inc=False, negate=False, drop_nonfinite=False,
                     refuse_negative=False, active_bitmap=None, attr_ids=None, attr_vals=None, missing=1.0, want_w=True,
                     want_k=True):
        """fgpu_pair_weights: per ordered node pair the smallest weight over the relationship types m .. multi (one entry per
        type, as for expand_edges), their multi-edges and the direction (out / inc), and the relationship kept.  attr_ids
        (strictly ascending) / attr_vals: the weight attribute, an id that is not listed weighs `missing`; attr_ids None: every
        relationship weighs 1.0 and W is a BOOL pattern.  Returns (W, K, stats): two Mats of one pattern (None where want_w /
        want_k is False) and the eight stats of fgpu.h.  A refused negative weight raises FgpuError with the smallest refused
        relationship id in its `refused_id`."""
        T = len(m)
        arrs = [_hop_arrays(x) if x is not None else None for x in (m, dp, dm, multi)]
        assert all(a is None or len(a) == T for a in arrs)
        act = _u64(active_bitmap) if active_bitmap is not None else None
        ids = vals = None
        n_attr = 0
        if attr_ids is not None:
            ids = _u64(attr_ids).reshape(-1)
            n_attr = len(ids)
            vals = np.ascontiguousarray(attr_vals, dtype=np.float64).reshape(-1)
            assert len(ids) == len(vals)
            if len(ids) == 0:   # (a list of nothing is still a list: keep the pointer non-NULL)
                ids, vals = np.zeros(1, dtype=U64), np.zeros(1, dtype=np.float64)
        flags = ((1 if out else 0) | (2 if inc else 0) | (4 if negate else 0) | (8 if drop_nonfinite else 0) |
                 (16 if refuse_negative else 0))
        w, k = C.c_void_p(), C.c_void_p()
        refused = C.c_uint64((1 << 64) - 1)
        st = (C.c_uint64 * 8)()
        code = self.lib.fgpu_pair_weights(self._h, *arrs, T, flags, _p(act), _p(ids), _p(vals, C.POINTER(C.c_double)),
                                          n_attr, float(missing),
                                          C.byref(w) if want_w else None, C.byref(k) if want_k else None, C.byref(refused), st)
        try:
            check(code)
        except _ffi.FgpuError as e:
            e.refused_id = None if refused.value == (1 << 64) - 1 else int(refused.value)
            raise
        return (Mat(self, w) if want_w else None, Mat(self, k) if want_k else None, [int(x) for x in st])


class Mat:
    """fgpu_mat: immutable device snapshot of one matrix layer."""

    def __init__(self, ctx: Context, h):
        self.ctx, self._h = ctx, h

    @property
    def handle(self):
        return self._h

    def free(self):
        if self._h:
            self.ctx.lib.fgpu_mat_free(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            if self.ctx._h:
                self.free()
        except Exception:
            pass

    def _get(self, fn):
        v = C.c_uint64()
        check(fn(self._h, C.byref(v)))
        return v.value

    @property
    def nrows(self):
        return self._get(self.ctx.lib.fgpu_mat_nrows)

    @property
    def ncols(self):
        return self._get(self.ctx.lib.fgpu_mat_ncols)

    @property
    def nvals(self):
        return self._get(self.ctx.lib.fgpu_mat_nvals)

    @property
    def has_values(self) -> bool:
        """True for a UINT64 snapshot (also an empty one), False for BOOL."""
        v = C.c_int32()
        check(self.ctx.lib.fgpu_mat_has_values(self._h, C.byref(v)))
        return bool(v.value)

    def min_val(self):
        """fgpu_mat_min_val: the smallest stored value read as binary64 (-0.0 counts as +0.0), None without entries."""
        bits, found = C.c_uint64(), C.c_int()
        check(self.ctx.lib.fgpu_mat_min_val(self.ctx._h, self._h, C.byref(bits), C.byref(found)))
        return float(np.array([bits.value], dtype=U64).view(np.float64)[0]) if found.value else None

    def export_csr(self):
        lib = self.ctx.lib
        rp, ci, vv = u64p(), u64p(), u64p()
        nnz = C.c_uint64()
        check(lib.fgpu_mat_export_csr(self.ctx._h, self._h, C.byref(rp), C.byref(ci), C.byref(vv), C.byref(nnz)))
        nrows = self.nrows
        rowptr = self.ctx._take(rp, nrows + 1)
        colidx = self.ctx._take(ci, max(nnz.value, 1))[: nnz.value]
        vals = self.ctx._take(vv, nnz.value) if vv else None
        return rowptr, colidx, vals

    def group_items(self):
        """The packed items of the cached transpose (fgpu_mat_group_items): hdr as (n, 4), cols as (n, 256), both uint32."""
        hp, cp = C.POINTER(C.c_uint32)(), C.POINTER(C.c_uint32)()
        n = C.c_uint64()
        check(self.ctx.lib.fgpu_mat_group_items(self.ctx._h, self._h, C.byref(hp), C.byref(cp), C.byref(n)))
        hdr = self.ctx._take(hp, max(n.value, 1) * 4, np.uint32)[: n.value * 4].reshape(-1, 4)
        cols = self.ctx._take(cp, max(n.value, 1) * 256, np.uint32)[: n.value * 256].reshape(-1, 256)
        return hdr, cols

    def xp_chunks(self):
        """The chunk table of the partitioned count hop's plan on the cached transpose (fgpu_mat_xp_chunks), under the options in
        force: dict(cut, pstart[9], cbase[9], cstart, crun0, cshared), the last three one entry per chunk."""
        wp = C.POINTER(C.c_uint32)()
        n = C.c_uint64()
        check(self.ctx.lib.fgpu_mat_xp_chunks(self.ctx._h, self._h, C.byref(wp), C.byref(n)))
        w = self.ctx._take(wp, n.value, np.uint32)
        nc = int(w[0])
        return dict(cut=int(w[1]), pstart=w[2:11].copy(), cbase=w[11:20].copy(), cstart=w[20:20 + nc].copy(),
                    crun0=w[20 + nc:20 + 2 * nc].copy(), cshared=w[20 + 2 * nc:20 + 3 * nc].copy())

    def extract(self, min_row=0, max_row=2**64 - 1):
        lib = self.ctx.lib
        r, c, v = u64p(), u64p(), u64p()
        n = C.c_uint64()
        check(lib.fgpu_mat_extract(self.ctx._h, self._h, min_row, max_row, C.byref(r), C.byref(c), C.byref(v),
                                   C.byref(n)))
        rows = self.ctx._take(r, n.value)
        cols = self.ctx._take(c, n.value)
        vals = self.ctx._take(v, n.value) if v else None
        return rows, cols, vals

    def transpose(self) -> "Mat":
        h = C.c_void_p()
        check(self.ctx.lib.fgpu_mat_transpose(self.ctx._h, C.byref(h), self._h))
        return Mat(self.ctx, h)

    def balanced_splits(self, nparts: int):
        """nnz-balanced boundaries of the destination vertices (columns) for `nparts` column slabs (multiples of 4096)."""
        out = np.zeros(nparts + 1, dtype=U64)
        check(self.ctx.lib.fgpu_mat_balanced_splits(self.ctx._h, self._h, nparts, _p(out)))
        return out

    def sample(self, seed: int, denom: int) -> "Mat":
        """Entries (r, c) with mix64(seed ^ mix64(r << 32 | c)) % denom == 0 (bench / test data)."""
        h = C.c_void_p()
        check(self.ctx.lib.fgpu_mat_sample(self.ctx._h, C.byref(h), self._h, C.c_uint64(seed), C.c_uint32(denom)))
        return Mat(self.ctx, h)

    def probe(self, rows, cols, want_vals=False):
        rows, cols = _u64(rows), _u64(cols)
        present = np.zeros(len(rows), dtype=np.uint8)
        vals = np.zeros(len(rows), dtype=U64) if want_vals else None
        check(self.ctx.lib.fgpu_mat_probe(self.ctx._h, self._h, _p(rows), _p(cols), len(rows), _p(present, u8p),
                                          _p(vals)))
        return (present, vals) if want_vals else present

    def merge(self, dp: "Mat | None", dm: "Mat | None", dm_masks_dp=False) -> "Mat":
        h = C.c_void_p()
        check(self.ctx.lib.fgpu_mat_merge(self.ctx._h, C.byref(h), self._h, dp._h if dp else None,
                                          dm._h if dm else None, 1 if dm_masks_dp else 0))
        return Mat(self.ctx, h)

    def merge_pattern(self, dp: "Mat | None", dm: "Mat | None", dm_masks_dp=False) -> "Mat":
        h = C.c_void_p()
        check(self.ctx.lib.fgpu_mat_merge_pattern(self.ctx._h, C.byref(h), self._h, dp._h if dp else None,
                                                  dm._h if dm else None, 1 if dm_masks_dp else 0))
        return Mat(self.ctx, h)

    def resize(self, nrows, ncols) -> "Mat":
        h = C.c_void_p()
        check(self.ctx.lib.fgpu_mat_resize(self.ctx._h, C.byref(h), self._h, nrows, ncols))
        return Mat(self.ctx, h)

    def intersect(self, b: "Mat") -> "Mat":
        h = C.c_void_p()
        check(self.ctx.lib.fgpu_mat_intersect(self.ctx._h, C.byref(h), self._h, b._h))
        return Mat(self.ctx, h)

    def intersect_nvals(self, b: "Mat") -> int:
        v = C.c_uint64()
        check(self.ctx.lib.fgpu_mat_intersect_nvals(self.ctx._h, self._h, b._h, C.byref(v)))
        return v.value

    def mxm(self, b: "Mat") -> "Mat":
        h = C.c_void_p()
        check(self.ctx.lib.fgpu_mxm(self.ctx._h, C.byref(h), self._h, b._h))
        return Mat(self.ctx, h)

    def delta_lmxm(self, m: "Mat", dp: "Mat | None", dm: "Mat | None") -> "Mat":
        h = C.c_void_p()
        check(self.ctx.lib.fgpu_delta_lmxm(self.ctx._h, C.byref(h), self._h, m._h, dp._h if dp else None,
                                           dm._h if dm else None))
        return Mat(self.ctx, h)

    def build_tiles(self, tile_bits=0, vec=0, k=0):
        check(self.ctx.lib.fgpu_mat_build_tiles(self.ctx._h, self._h, tile_bits, vec, k))
        return self.tiles_info()

    def tiles_info(self):
        s = np.zeros(8, dtype=U64)
        check(self.ctx.lib.fgpu_mat_tiles_info(self._h, _p(s)))
        keys = ["tile_bits", "tiles", "groups", "items", "entries", "vec", "k", "bytes"]
        return dict(zip(keys, (int(x) for x in s)))

    def row_degrees(self, out_dev_ptr: int):
        """deg[r] = stored entries of row r, written to DEVICE memory (uint32[nrows], e.g. a torch int32 tensor)."""
        check(self.ctx.lib.fgpu_mat_row_degrees(self.ctx._h, self._h, C.c_void_p(out_dev_ptr)))

    def col_slab(self, lo, hi) -> "Mat":
        h = C.c_void_p()
        check(self.ctx.lib.fgpu_mat_col_slab(self.ctx._h, C.byref(h), self._h, lo, hi))
        return Mat(self.ctx, h)

    def row_slab(self, lo, hi) -> "Mat":
        h = C.c_void_p()
        check(self.ctx.lib.fgpu_mat_row_slab(self.ctx._h, C.byref(h), self._h, lo, hi))
        return Mat(self.ctx, h)


class Multi:
    """fgpu_multi: one tensor's multi-edge rows, resident on the device (Context.multi_new)."""

    def __init__(self, ctx: Context, h):
        self.ctx, self._h = ctx, h

    def size(self):
        """(rows, ids) held"""
        a, b = C.c_uint64(), C.c_uint64()
        check(self.ctx.lib.fgpu_multi_size(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def free(self):
        if self._h:
            self.ctx.lib.fgpu_multi_free(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            if self.ctx._h:
                self.free()
        except Exception:
            pass


def _hop_arrays(mats):
    arr = (C.c_void_p * len(mats))()
    for i, m in enumerate(mats):
        arr[i] = m._h if m is not None else None
    return arr


def expand(ctx: Context, src_ids, m, dp=None, dm=None, dst_label_bitmap=None):
    """fgpu_expand: the device core of CondTraverseOp::expand_batch.  Returns (rowptr, dest, flops)."""
    src = _u64(src_ids)
    nh = len(m)
    am = _hop_arrays(m)
    adp = _hop_arrays(dp) if dp is not None else None
    adm = _hop_arrays(dm) if dm is not None else None
    lab = _u64(dst_label_bitmap) if dst_label_bitmap is not None else None
    rp, ci = u64p(), u64p()
    nnz, flops = C.c_uint64(), C.c_uint64()
    check(ctx.lib.fgpu_expand(ctx._h, _p(src), len(src), am, adp, adm, nh, _p(lab), C.byref(rp), C.byref(ci),
                              C.byref(nnz), C.byref(flops)))
    rowptr = ctx._take(rp, len(src) + 1)
    dest = ctx._take(ci, max(nnz.value, 1))[: nnz.value]
    return rowptr, dest, flops.value


def expand32(ctx: Context, src_ids, m, dp=None, dm=None, dst_label_bitmap=None):
    """fgpu_expand32: the same result in the device's own 32-bit form — (rowptr uint32[nsrc + 1], dest uint32[nnz], flops):
    two DMAs of the arrays as they lie, half the PCIe bytes of fgpu_expand."""
    src = _u64(src_ids)
    nh = len(m)
    am = _hop_arrays(m)
    adp = _hop_arrays(dp) if dp is not None else None
    adm = _hop_arrays(dm) if dm is not None else None
    lab = _u64(dst_label_bitmap) if dst_label_bitmap is not None else None
    u32p = C.POINTER(C.c_uint32)
    rp, ci = u32p(), u32p()
    nnz, flops = C.c_uint64(), C.c_uint64()
    check(ctx.lib.fgpu_expand32(ctx._h, _p(src), len(src), am, adp, adm, nh, _p(lab), C.byref(rp), C.byref(ci),
                                C.byref(nnz), C.byref(flops)))
    rowptr = ctx._take(rp, len(src) + 1, dtype=np.uint32)
    dest = ctx._take(ci, max(nnz.value, 1), dtype=np.uint32)[: nnz.value]
    return rowptr, dest, flops.value


class ExpandStream:
    """fgpu_expand_stream_*: the chain's result handed over in chunks of whole source rows while later chunks are still
    on the link.  Iterating yields (first_row, rowptr, dest) — views valid until the next step."""

    def __init__(self, ctx: Context, src_ids, m, dp=None, dm=None, dst_label_bitmap=None, chunk_rows=64, dest_bits=64):
        src = _u64(src_ids)
        am = _hop_arrays(m)
        adp = _hop_arrays(dp) if dp is not None else None
        adm = _hop_arrays(dm) if dm is not None else None
        lab = _u64(dst_label_bitmap) if dst_label_bitmap is not None else None
        self.ctx, self._h, self.dest_bits = ctx, C.c_void_p(), dest_bits
        nnz, flops = C.c_uint64(), C.c_uint64()
        check(ctx.lib.fgpu_expand_stream_open(ctx._h, _p(src), len(src), am, adp, adm, len(m), _p(lab), chunk_rows, dest_bits,
                                              C.byref(self._h), C.byref(nnz), C.byref(flops)))
        self.nnz, self.flops = nnz.value, flops.value

    def __iter__(self):
        return self

    def __next__(self):
        first, nrows = C.c_uint64(), C.c_uint64()
        rp, dest = u64p(), C.c_void_p()
        code = self.ctx.lib.fgpu_expand_stream_next(self._h, C.byref(first), C.byref(nrows), C.byref(rp), C.byref(dest))
        if code == _ffi.FGPU_NO_VALUE:
            raise StopIteration
        check(code)
        rowptr = np.ctypeslib.as_array(rp, shape=(nrows.value + 1,))
        n = int(rowptr[-1])
        dt = np.uint64 if self.dest_bits == 64 else np.uint32
        d = np.ctypeslib.as_array(C.cast(dest, C.POINTER(C.c_uint64 if self.dest_bits == 64 else C.c_uint32)), shape=(n,)) \
            if n else np.zeros(0, dtype=dt)
        return first.value, rowptr, d

    def close(self):
        if self._h:
            self.ctx.lib.fgpu_expand_stream_close(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            if self.ctx._h:
                self.close()
        except Exception:
            pass


def expand_mat(ctx: Context, src_ids, m, dp=None, dm=None, dst_label_bitmap=None):
    """fgpu_expand_mat: the same chain with F left on the device as a matrix handle (cond_traverse.rs:602-608).
    Returns (Mat with len(src_ids) rows, flops)."""
    src = _u64(src_ids)
    am = _hop_arrays(m)
    adp = _hop_arrays(dp) if dp is not None else None
    adm = _hop_arrays(dm) if dm is not None else None
    lab = _u64(dst_label_bitmap) if dst_label_bitmap is not None else None
    h = C.c_void_p()
    flops = C.c_uint64()
    check(ctx.lib.fgpu_expand_mat(ctx._h, _p(src), len(src), am, adp, adm, len(m), _p(lab), C.byref(h), C.byref(flops)))
    return Mat(ctx, h), flops.value


def expand_count(ctx: Context, src_ids, m, dp=None, dm=None, dst_label_bitmap=None, want_checksum=True):
    """fgpu_expand_count: (nnz, checksum, flops) of the k-hop result without materialising it on the host;
    want_checksum=False skips the per-entry hashing (count only: `RETURN count(c)`), checksum comes back 0."""
    src = _u64(src_ids)
    am = _hop_arrays(m)
    adp = _hop_arrays(dp) if dp is not None else None
    adm = _hop_arrays(dm) if dm is not None else None
    lab = _u64(dst_label_bitmap) if dst_label_bitmap is not None else None
    nnz, cs, flops = C.c_uint64(), C.c_uint64(), C.c_uint64()
    check(ctx.lib.fgpu_expand_count(ctx._h, _p(src), len(src), am, adp, adm, len(m), _p(lab), C.byref(nnz),
                                    C.byref(cs) if want_checksum else None, C.byref(flops)))
    return nnz.value, cs.value, flops.value


def expand_trail_counts(ctx: Context, src_ids, m, dp=None, dm=None, weighted=False):
    """fgpu_expand_trail_counts: trails of exactly len(m) (1 or 2) hops per (source row, destination).
    Returns (rowptr, dest, count)."""
    src = _u64(src_ids)
    am = _hop_arrays(m)
    adp = _hop_arrays(dp) if dp is not None else None
    adm = _hop_arrays(dm) if dm is not None else None
    rp, ci, cv = u64p(), u64p(), u64p()
    nnz = C.c_uint64()
    check(ctx.lib.fgpu_expand_trail_counts(ctx._h, _p(src), len(src), am, adp, adm, len(m), 1 if weighted else 0,
                                           C.byref(rp), C.byref(ci), C.byref(cv), C.byref(nnz)))
    rowptr = ctx._take(rp, len(src) + 1)
    dest = ctx._take(ci, max(nnz.value, 1))[: nnz.value]
    count = ctx._take(cv, max(nnz.value, 1))[: nnz.value]
    return rowptr, dest, count


def expand_levels(ctx: Context, src_ids, m, dp=None, dm=None, dst_label_bitmap=None):
    """fgpu_expand_levels: per-hop (nnz, checksum) of the chain and the DISTINCT union over the hops."""
    src = _u64(src_ids)
    nh = len(m)
    am = _hop_arrays(m)
    adp = _hop_arrays(dp) if dp is not None else None
    adm = _hop_arrays(dm) if dm is not None else None
    lab = _u64(dst_label_bitmap) if dst_label_bitmap is not None else None
    hn, hc = np.zeros(nh, dtype=U64), np.zeros(nh, dtype=U64)
    un, uc, fl = C.c_uint64(), C.c_uint64(), C.c_uint64()
    check(ctx.lib.fgpu_expand_levels(ctx._h, _p(src), len(src), am, adp, adm, nh, _p(lab), _p(hn), _p(hc),
                                     C.byref(un), C.byref(uc), C.byref(fl)))
    return {"hop_nnz": hn.tolist(), "hop_checksum": hc.tolist(), "union_nnz": un.value,
            "union_checksum": uc.value, "flops": fl.value}


def vxm(ctx: Context, f_bits, mask_bits, A: Mat, At: Mat | None = None, direction=0):
    f = _u64(f_bits)
    mk = _u64(mask_bits) if mask_bits is not None else None
    w = np.zeros(len(f), dtype=U64)
    check(ctx.lib.fgpu_vxm(ctx._h, _p(w), _p(f), _p(mk), A._h, At._h if At else None, direction))
    return w


def bfs(ctx: Context, A: Mat, At: Mat | None, src: int, max_level: int = -1, want_parent: bool = True, level_out=None,
        parent_out=None):
    """fgpu_bfs.  level_out / parent_out: arrays to fill instead of fresh numpy ones — pass Context.host_array() blocks
    (pinned) and the library DMAs into them."""
    n = A.nrows
    level = level_out if level_out is not None else np.zeros(n, dtype=np.int32)
    parent = (parent_out if parent_out is not None else np.zeros(n, dtype=np.int64)) if want_parent else None
    edges = C.c_uint64()
    check(ctx.lib.fgpu_bfs(ctx._h, A._h, At._h if At else None, src, max_level, _p(level, i32p),
                           _p(parent, i64p), C.byref(edges)))
    return level, parent, edges.value


def pagerank(ctx: Context, A: Mat, At: Mat | None = None, active_bitmap=None, damping: float = 0.85,
             tol: float = 1e-4, itermax: int = 100):
    """fgpu_pagerank: LAGr_PageRank's numbers for algo.pageRank (FP32).  Returns (scores float32[n], iters)."""
    n = A.nrows
    out = np.zeros(n, dtype=np.float32)
    act = _u64(active_bitmap) if active_bitmap is not None else None
    it = C.c_int32()
    check(ctx.lib.fgpu_pagerank(ctx._h, A._h, At._h if At else None, _p(act), C.c_float(damping), C.c_float(tol),
                                C.c_int32(itermax), out.ctypes.data_as(C.POINTER(C.c_float)), C.byref(it)))
    return out, it.value


def wcc(ctx: Context, A: Mat, At: Mat | None = None, active_bitmap=None, stats: bool = False, out=None):
    """fgpu_wcc: LAGr_ConnectedComponents' partition for algo.WCC, every component labelled by its smallest vertex id (-1 for
    vertices outside active_bitmap).  At = None promises a symmetric pattern.  out: an int64 array to fill instead of a fresh
    one (a Context.host_array() block is filled by DMA).  Returns (component int64[n], stats) — stats the four counters
    [components, entries read, link launches, sampled giant size] when stats=True, else None."""
    n = A.nrows
    comp = out if out is not None else np.zeros(n, dtype=np.int64)
    act = _u64(active_bitmap) if active_bitmap is not None else None
    st = np.zeros(4, dtype=np.uint64)
    check(ctx.lib.fgpu_wcc(ctx._h, A._h, At._h if At else None, _p(act), _p(comp, i64p), _p(st)))
    return comp, ([int(x) for x in st] if stats else None)


def cdlp(ctx: Context, S: Mat, active_bitmap=None, itermax: int = 10, stats: bool = False, out=None):
    """fgpu_cdlp: LAGraph_cdlp's labels for algo.labelPropagation over the symmetric pattern S — synchronous label propagation
    from label[v] = v, the most frequent neighbour label winning, ties to the smallest (-1 for vertices outside
    active_bitmap).  out: an int64 array to fill instead of a fresh one (a Context.host_array() block is filled by DMA).
    Returns (label int64[n], stats) — stats the four counters [iterations run, labels changed in the last iteration, entries
    read, distinct labels] when stats=True, else None."""
    n = S.nrows
    lab = out if out is not None else np.zeros(n, dtype=np.int64)
    act = _u64(active_bitmap) if active_bitmap is not None else None
    st = np.zeros(4, dtype=np.uint64)
    check(ctx.lib.fgpu_cdlp(ctx._h, S._h, _p(act), C.c_int32(itermax), _p(lab, i64p), _p(st)))
    return lab, ([int(x) for x in st] if stats else None)


def harmonic(ctx: Context, A: Mat, active_bitmap=None, stats: bool = False, registers: bool = False, out=None):
    """fgpu_harmonic: LAGr_HarmonicCentrality's HyperBall scores for algo.HarmonicCentrality over the directed pattern A — a
    1024-register HyperLogLog sketch of every vertex' out-ball, merged along the out-entries until no sketch changes (0.0 / -1
    for vertices outside active_bitmap).  out: a (score float64[n], reachable int64[n]) pair to fill instead of fresh arrays
    (Context.host_array() blocks are filled by DMA).  Returns (score, reachable, registers, stats) — registers the final
    uint8[n, 1024] sketches when registers=True, stats the four counters [iterations that changed a sketch, sketch changes,
    largest reachable, vertices with a non-zero score] when stats=True, else None."""
    n = A.nrows
    score, reach = out if out is not None else (np.zeros(n, dtype=np.float64), np.zeros(n, dtype=np.int64))
    act = _u64(active_bitmap) if active_bitmap is not None else None
    regs = np.zeros((n, 1024), dtype=np.uint8) if registers else None
    st = np.zeros(4, dtype=np.uint64)
    check(ctx.lib.fgpu_harmonic(ctx._h, A._h, _p(act), _p(score, C.POINTER(C.c_double)), _p(reach, i64p),
                                _p(regs, C.POINTER(C.c_uint8)), _p(st)))
    return score, reach, regs, ([int(x) for x in st] if stats else None)


def msf(ctx: Context, W: Mat, active_bitmap=None, stats: bool = False, out=None):
    """fgpu_msf: LAGraph_msf's forest for algo.MSF over the symmetric weighted matrix W — a valued snapshot carries one binary64
    bit pattern per entry, a BOOL one means every weight is 1.0; ties go to the smaller (min, max) pair, so the forest is
    unique.  out: an int64 array to fill with the components instead of a fresh one (a Context.host_array() block is filled by
    DMA).  Returns (component int64[n], rows uint64[k], cols uint64[k], weights float64[k], stats) — component labelled as by
    wcc (-1 outside active_bitmap), the forest once per edge as row < col sorted by (row, col), stats the four counters
    [rounds, forest edges, entries read, components] when stats=True, else None."""
    n = W.nrows
    comp = out if out is not None else np.zeros(n, dtype=np.int64)
    act = _u64(active_bitmap) if active_bitmap is not None else None
    r, c, w = u64p(), u64p(), C.POINTER(C.c_double)()
    k = C.c_uint64()
    st = np.zeros(4, dtype=np.uint64)
    check(ctx.lib.fgpu_msf(ctx._h, W._h, _p(act), _p(comp, i64p), C.byref(r), C.byref(c), C.byref(w), C.byref(k), _p(st)))
    rows = ctx._take(r, k.value)
    cols = ctx._take(c, k.value)
    weights = ctx._take(w, k.value, dtype=np.float64)
    return comp, rows, cols, weights, ([int(x) for x in st] if stats else None)


def edges_build(ctx: Context, nrows: int, ncols: int, srcs, dsts, ids, stats: bool = False):
    """fgpu_edges_build: one relationship type's bulk batch of (src, dst, edge id) tuples as a Tensor holds it.  Returns (fwd,
    bwd, multi_key, multi_off, multi_ids[, stats]) — fwd the UINT64 matrix with the edge id of a pair that has one edge and
    MULTI_EDGE (~0) for a pair that has several, bwd the BOOL transposed pattern, multi_key the ascending compound keys
    (src << 32 | dst) of the multi-edge pairs, multi_ids[multi_off[r] : multi_off[r + 1]] the ascending ids of pair r; stats the
    eight counters of include/fgpu.h when stats=True."""
    srcs, dsts, ids = _u64(srcs), _u64(dsts), _u64(ids)
    if not (len(srcs) == len(dsts) == len(ids)):
        raise ValueError("edges_build: srcs, dsts and ids differ in length")
    fwd, bwd = C.c_void_p(), C.c_void_p()
    mk, mo, mi = u64p(), u64p(), u64p()
    nm = C.c_uint64()
    st = np.zeros(8, dtype=np.uint64)
    check(ctx.lib.fgpu_edges_build(ctx._h, C.c_uint64(nrows), C.c_uint64(ncols), _p(srcs), _p(dsts), _p(ids), len(srcs),
                                   C.byref(fwd), C.byref(bwd), C.byref(mk), C.byref(mo), C.byref(mi), C.byref(nm), _p(st)))
    off = ctx._take(mo, nm.value + 1)
    total = int(off[-1])
    out = (Mat(ctx, fwd), Mat(ctx, bwd), ctx._take(mk, nm.value), off, ctx._take(mi, total))
    return out + ([int(x) for x in st],) if stats else out


def nodes_detach(ctx: Context, m: Mat, mt: "Mat | None", nodes, sides: int = 3, want_list: bool = True, stats: bool = False):
    """fgpu_nodes_detach: the matrix m (and its transposed pattern mt, or None) without the entries whose row (sides bit 0) or
    column (bit 1) is one of `nodes`.  Returns (m_out, mt_out or None, rem_row, rem_col, rem_val, n_rem_out[, stats]): the
    first n_rem_out triples of the removal list are the out entries in ascending (src, dst), the others the in entries in
    ascending (dst, src); want_list=False asks for no list (three empty arrays, n_rem_out 0); stats the eight counters of
    include/fgpu.h when stats=True."""
    nodes = _u64(nodes).reshape(-1)
    mo, mto = C.c_void_p(), C.c_void_p()
    rr, rc, rv = u64p(), u64p(), u64p()
    n, n_out = C.c_uint64(), C.c_uint64()
    st = np.zeros(8, dtype=np.uint64)
    check(ctx.lib.fgpu_nodes_detach(ctx._h, m._h, mt._h if mt is not None else None, _p(nodes), len(nodes), int(sides),
                                    C.byref(mo), C.byref(mto) if mt is not None else None,
                                    C.byref(rr) if want_list else None, C.byref(rc) if want_list else None,
                                    C.byref(rv) if want_list else None, C.byref(n) if want_list else None,
                                    C.byref(n_out) if want_list else None, _p(st)))
    out = (Mat(ctx, mo), Mat(ctx, mto) if mt is not None else None, ctx._take(rr, n.value), ctx._take(rc, n.value),
           ctx._take(rv, n.value), int(n_out.value))
    return out + ([int(x) for x in st],) if stats else out


def edges_remove(ctx: Context, m: Mat, mt: "Mat | None", srcs, dsts, ids, multi_key=(), multi_off=(0,), multi_ids=(),
                 want_hit: bool = True, stats: bool = False):
    """fgpu_edges_remove: the tensor base m (UINT64: inline edge id or MULTI_EDGE) and its transposed pattern mt without the
    edges the (src, dst, id) triples name; multi_key / multi_off / multi_ids are the multi-edge rows of the touched pairs in
    edges_build's shape.  Returns (m_out, mt_out, hit uint8[n] or None, multi_taken uint8[len(multi_ids)], emp_row, emp_col[,
    stats]): hit[k] = triple k named a stored edge, multi_taken[j] = multi_ids[j] was removed, (emp_row, emp_col) the pairs that
    left m in ascending (src, dst); stats the eight counters of include/fgpu.h when stats=True."""
    srcs, dsts, ids = _u64(srcs).reshape(-1), _u64(dsts).reshape(-1), _u64(ids).reshape(-1)
    if not (len(srcs) == len(dsts) == len(ids)):
        raise ValueError("edges_remove: srcs, dsts and ids differ in length")
    mk, mo, mi = _u64(multi_key).reshape(-1), _u64(multi_off).reshape(-1), _u64(multi_ids).reshape(-1)
    if len(mo) != len(mk) + 1 or (len(mk) and int(mo[-1]) != len(mi)):
        raise ValueError("edges_remove: multi_off does not describe multi_key / multi_ids")
    mout, mtout = C.c_void_p(), C.c_void_p()
    hit = np.zeros(len(srcs), dtype=np.uint8) if want_hit else None
    taken = np.zeros(len(mi), dtype=np.uint8)
    er, ec = u64p(), u64p()
    ne = C.c_uint64()
    st = np.zeros(8, dtype=np.uint64)
    check(ctx.lib.fgpu_edges_remove(ctx._h, m._h, mt._h if mt is not None else None, _p(srcs), _p(dsts), _p(ids), len(srcs),
                                    _p(mk), _p(mo), _p(mi), len(mk), C.byref(mout), C.byref(mtout), _p(hit, u8p), _p(taken, u8p),
                                    C.byref(er), C.byref(ec), C.byref(ne), _p(st)))
    out = (Mat(ctx, mout), Mat(ctx, mtout), hit, taken, ctx._take(er, ne.value), ctx._take(ec, ne.value))
    return out + ([int(x) for x in st],) if stats else out


def _rows(name, key, off, ids):
    key, off, ids = _u64(key).reshape(-1), _u64(off).reshape(-1), _u64(ids).reshape(-1)
    if len(off) != len(key) + 1 or (len(key) and int(off[-1]) != len(ids)):
        raise ValueError(f"edges_union: {name}_off does not describe {name}_key / {name}_ids")
    return key, off, ids


def edges_union(ctx: Context, m: Mat, mt: "Mat | None", a_key, a_off, a_ids, fwd: Mat, bwd: "Mat | None", b_key, b_off, b_ids,
                stats: bool = False):
    """fgpu_edges_union: the tensor base m and its transposed pattern mt joined with one built batch (fwd, bwd, b rows: what
    edges_build returned); a_key / a_off / a_ids are the multi-edge rows of the pairs of m the batch touches.  Returns (m_out,
    mt_out, o_key, o_off, o_ids[, stats]): a pair new to m enters with fwd's value, a pair stored in both holds MULTI_EDGE and
    its ids are o_ids[o_off[r] : o_off[r + 1]] — the ascending merge of both sides — under o_key[r]; stats the eight counters of
    include/fgpu.h when stats=True."""
    ak, ao, ai = _rows("a", a_key, a_off, a_ids)
    bk, bo, bi = _rows("b", b_key, b_off, b_ids)
    mout, mtout = C.c_void_p(), C.c_void_p()
    ok, oo, oi = u64p(), u64p(), u64p()
    no = C.c_uint64()
    st = np.zeros(8, dtype=np.uint64)
    check(ctx.lib.fgpu_edges_union(ctx._h, m._h, mt._h if mt is not None else None, _p(ak), _p(ao), _p(ai), len(ak), fwd._h,
                                   bwd._h if bwd is not None else None, _p(bk), _p(bo), _p(bi), len(bk), C.byref(mout),
                                   C.byref(mtout), C.byref(ok), C.byref(oo), C.byref(oi), C.byref(no), _p(st)))
    off = ctx._take(oo, no.value + 1)
    out = (Mat(ctx, mout), Mat(ctx, mtout), ctx._take(ok, no.value), off, ctx._take(oi, int(off[-1])))
    return out + ([int(x) for x in st],) if stats else out


def maxflow(ctx: Context, C_: Mat, src: int, sink: int, stats: bool = False):
    """fgpu_maxflow: LAGr_MaxFlow's result for algo.maxFlow over the capacity matrix C_ — a valued snapshot carries one binary64
    bit pattern per entry, a BOOL one means capacity 1.0; diagonal entries and capacities <= 0 are ignored, a NaN or infinite
    one is an error.  Returns (value, rows uint64[k], cols uint64[k], flows float64[k], stats) — the arcs that carry flow > 0
    sorted by (row, col); the value is unique, the assignment is one of the maximum flows; stats the four counters [pulses,
    global relabels, residual arcs, pushes] when stats=True, else None."""
    r, c, f = u64p(), u64p(), C.POINTER(C.c_double)()
    k = C.c_uint64()
    val = C.c_double()
    st = np.zeros(4, dtype=np.uint64)
    check(ctx.lib.fgpu_maxflow(ctx._h, C_._h, C.c_uint64(src), C.c_uint64(sink), C.byref(val), C.byref(r), C.byref(c),
                               C.byref(f), C.byref(k), _p(st)))
    rows = ctx._take(r, k.value)
    cols = ctx._take(c, k.value)
    flows = ctx._take(f, k.value, dtype=np.float64)
    return val.value, rows, cols, flows, ([int(x) for x in st] if stats else None)


def sssp(ctx: Context, W: Mat, src: int, want_parent: bool = True, stats: bool = False, out=None):
    """fgpu_sssp: single-source shortest paths for algo.SPpaths over the weight matrix W — a valued snapshot carries one binary64
    bit pattern per entry (non-negative; a NaN or negative one is an error), a BOOL one means every weight is 1.0.  out: a
    (dist float64[n], parent int64[n] | None) pair to fill instead of fresh arrays (Context.host_array() blocks are filled by
    DMA).  Returns (dist, parent) — dist +inf and parent -1 where no route reaches, parent[src] = src, parent None when
    want_parent=False — and, when stats=True, a third item: the four counters [relaxation launches, vertices taken off a
    worklist, entries read, deepest tight-entry depth]."""
    n = W.nrows
    if out is not None:
        dist, parent = out
    else:
        dist, parent = np.zeros(n, dtype=np.float64), (np.zeros(n, dtype=np.int64) if want_parent else None)
    if not want_parent:
        parent = None
    st = np.zeros(4, dtype=np.uint64) if stats else None
    check(ctx.lib.fgpu_sssp(ctx._h, W._h, C.c_uint64(src), _p(dist, C.POINTER(C.c_double)), _p(parent, i64p), _p(st)))
    if stats:
        return dist, parent, [int(x) for x in st]
    return dist, parent


def sssp_hops(ctx: Context, W: Mat, src: int, max_hops: int, stats: bool = False, out=None):
    """fgpu_sssp_hops: the hop-bounded shortest-path table from src over the weight matrix W (fgpu_sssp's rules for W) — row h
    holds, per vertex, the weight of the cheapest route of at most h arcs, +inf where there is none; max_hops is 0 .. 32.  out: a
    (max_hops + 1, n) float64 array to fill instead of a fresh one (a Context.host_array() block is filled by DMA).  Returns the
    (max_hops + 1, n) float64 table and, when stats=True, a second item: the four counters [rounds with a frontier, frontier
    entries taken, entries read, the first h whose row equals the one before (max_hops + 1: none)]."""
    n = W.nrows
    rows = int(max_hops) + 1 if 0 <= max_hops <= 32 else 1   # (out of range: the call refuses before it writes)
    table = out if out is not None else np.zeros((rows, n), dtype=np.float64)
    assert table.dtype == np.float64 and table.shape == (rows, n) and table.flags.c_contiguous
    st = np.zeros(4, dtype=np.uint64) if stats else None
    check(ctx.lib.fgpu_sssp_hops(ctx._h, W._h, C.c_uint64(src), C.c_int32(max_hops), _p(table, C.POINTER(C.c_double)), _p(st)))
    if stats:
        return table, [int(x) for x in st]
    return table


def shortest_dag(ctx: Context, A: Mat, At: Mat | None, src: int, dst: int, max_hops: int = -1, stats: bool = False):
    """fgpu_shortest_dag: the shortest-path DAG between src and dst over the pattern A (At its transpose, None = built for the
    call) — what allShortestPaths' predecessor walk reads.  src == dst asks for the shortest cycle through src.  Returns
    (length, from uint64[k], to uint64[k], depth uint64[k]) — length -1 and empty arrays when no path of at most max_hops
    (< 0: unbounded) exists, else the pairs (u, v) with an entry u -> v on some shortest path, sorted by (from, to), depth =
    d(src, from) — and, when stats=True, a fifth item: the eight counters [forward levels, backward levels, vertices claimed
    forward, claimed backward, entries scanned by the expansions, by the sweeps, meeting vertices, DAG vertices]."""
    f, t, d = u64p(), u64p(), u64p()
    k = C.c_uint64()
    length = C.c_int64()
    st = np.zeros(8, dtype=np.uint64) if stats else None
    check(ctx.lib.fgpu_shortest_dag(ctx._h, A._h, At._h if At else None, C.c_uint64(src), C.c_uint64(dst), C.c_int64(max_hops),
                                    C.byref(length), C.byref(k), C.byref(f), C.byref(t), C.byref(d), _p(st)))
    out = (length.value, ctx._take(f, k.value), ctx._take(t, k.value), ctx._take(d, k.value))
    return out + ([int(x) for x in st],) if stats else out


def shortest_dag_batch(ctx: Context, A: Mat, At: Mat | None, srcs, dsts, max_hops: int = -1, slots: int = 0, stats: bool = False):
    """fgpu_shortest_dag_batch: shortest_dag for the queries (srcs[i], dsts[i]) in one call, `slots` of them searched together
    (0 = derived from the vertex count, at most 64).  Returns a list with, per query, the tuple shortest_dag returns for it:
    (length, from, to, depth) and, when stats=True, its eight counters.  The arrays of the queries are slices of three
    arrays the call returned."""
    s, d = _u64(srcs), _u64(dsts)
    assert len(s) == len(d)
    count = len(s)
    f, t, dep = u64p(), u64p(), u64p()
    length = np.zeros(count, dtype=np.int64)
    off = np.zeros(count + 1, dtype=np.uint64)
    st = np.zeros(count * 8, dtype=np.uint64) if stats else None
    check(ctx.lib.fgpu_shortest_dag_batch(ctx._h, A._h, At._h if At else None, _p(s) if count else None, _p(d) if count else None,
                                          C.c_uint64(count), C.c_int64(max_hops), C.c_uint32(slots),
                                          length.ctypes.data_as(C.POINTER(C.c_int64)), _p(off), C.byref(f), C.byref(t), C.byref(dep),
                                          _p(st)))
    total = int(off[count])
    cols = [ctx._take(x, total) for x in (f, t, dep)]
    out = []
    for i in range(count):
        lo, hi = int(off[i]), int(off[i + 1])
        row = (int(length[i]), cols[0][lo:hi], cols[1][lo:hi], cols[2][lo:hi])
        out.append(row + ([int(x) for x in st[8 * i:8 * i + 8]],) if stats else row)
    return out


def shortest_path_batch(ctx: Context, F: Mat, B: Mat | None, srcs, dsts, max_hops: int = -1, slots: int = 0, stats: bool = False):
    """fgpu_shortest_path_batch: the reference's shortestPath() for the queries (srcs[i], dsts[i]) in one call — the ONE path its
    bidirectional search returns, to the vertex.  F is the pattern the forward side walks, B the one the backward side walks
    (None = F's transpose, built for the call; an undirected pattern passes S = F U F' for both), `slots` the queries searched
    together (0 = derived from the vertex count, at most 64).  Returns a list with, per query, the node ids of its path as a
    uint64 array (length + 1 of them), or None without a path within max_hops (< 0: unbounded) — and, when stats=True, a
    (path, stats) tuple with the eight counters [forward levels, backward levels, vertices claimed forward, claimed backward,
    entries walked, meeting vertex (2^64 - 1: none), meeting candidates of the last level, 0]."""
    s, d = _u64(srcs), _u64(dsts)
    assert len(s) == len(d)
    count = len(s)
    nodes = u64p()
    length = np.zeros(count, dtype=np.int64)
    off = np.zeros(count + 1, dtype=np.uint64)
    st = np.zeros(count * 8, dtype=np.uint64) if stats else None
    check(ctx.lib.fgpu_shortest_path_batch(ctx._h, F._h, B._h if B else None, _p(s) if count else None, _p(d) if count else None,
                                           C.c_uint64(count), C.c_int64(max_hops), C.c_uint32(slots),
                                           length.ctypes.data_as(C.POINTER(C.c_int64)), _p(off), C.byref(nodes), _p(st)))
    flat = ctx._take(nodes, int(off[count]))
    out = []
    for i in range(count):
        path = flat[int(off[i]):int(off[i + 1])] if length[i] >= 0 else None
        out.append((path, [int(x) for x in st[8 * i:8 * i + 8]]) if stats else path)
    return out


def betweenness(ctx: Context, A: Mat, sources, At: Mat | None = None, active_bitmap=None, stats: bool = False, out=None):
    """fgpu_betweenness: LAGr_Betweenness' unnormalised scores for algo.betweenness — the sum over `sources` (vertex ids, taken
    as given: a duplicate counts twice) of every vertex's dependency, 0 outside active_bitmap.  At = None uses A's cached
    transpose.  out: a float64 array to fill instead of a fresh one (a Context.host_array() block is filled by DMA).  Returns
    (centrality float64[n], stats) — stats the four counters [batches, forward levels, adjacency entries read, deepest level]
    when stats=True, else None."""
    n = A.nrows
    cent = out if out is not None else np.zeros(n, dtype=np.float64)
    src = _u64(sources)
    act = _u64(active_bitmap) if active_bitmap is not None else None
    st = np.zeros(4, dtype=np.uint64)
    check(ctx.lib.fgpu_betweenness(ctx._h, A._h, At._h if At else None, _p(act), _p(src) if len(src) else None, len(src),
                                   cent.ctypes.data_as(C.POINTER(C.c_double)), _p(st)))
    return cent, ([int(x) for x in st] if stats else None)


VEC_METRICS = {"euclidean": 0, "cosine": 1, "ip": 2}


class VecIndex:
    """fgpu_vecidx: a dense store of f32 vectors under ids below 2^32 - 1, searched exhaustively on the device — the core of
    db.idx.vector.queryNodes / queryRelationships (the rules are in include/fgpu.h)."""

    def __init__(self, ctx: Context, dim: int, metric="euclidean"):
        self.ctx = ctx
        self._h = C.c_void_p()
        m = VEC_METRICS[metric] if isinstance(metric, str) else int(metric)
        check(ctx.lib.fgpu_vecidx_new(ctx._h, C.byref(self._h), C.c_uint32(dim), C.c_int(m)))

    def free(self):
        if self._h and self.ctx._h:
            self.ctx.lib.fgpu_vecidx_free(self._h)
        self._h = C.c_void_p()

    def __del__(self):
        try:
            if self.ctx._h:   # (the index points into its context: never touched after fgpu_finalize)
                self.free()
        except Exception:
            pass

    def info(self):
        """(dim, metric, count)"""
        d, m, n = C.c_uint32(), C.c_int(), C.c_uint64()
        check(self.ctx.lib.fgpu_vecidx_info(self._h, C.byref(d), C.byref(m), C.byref(n)))
        return d.value, m.value, n.value

    @property
    def dim(self):
        return self.info()[0]

    @property
    def count(self):
        return self.info()[2]

    def _vecs(self, vecs, rows=None):
        v = np.ascontiguousarray(vecs, dtype=np.float32)
        v = v.reshape(1, -1) if v.ndim == 1 else v
        if v.ndim != 2 or v.shape[1] != self.dim or (rows is not None and v.shape[0] != rows):
            raise ValueError(f"expected {'n' if rows is None else rows} rows of {self.dim} float32 components, got {v.shape}")
        return v

    def set(self, ids, vecs):
        """Upsert: vecs[i] becomes the vector of ids[i]; of an id given twice the last row wins."""
        i = _u64(np.atleast_1d(ids))
        v = self._vecs(vecs, len(i))
        check(self.ctx.lib.fgpu_vecidx_set(self.ctx._h, self._h, _p(i), _p(v, C.POINTER(C.c_float)), len(i)))

    def remove(self, ids) -> int:
        """Removes the ids that are present and returns how many were."""
        i = _u64(np.atleast_1d(ids))
        gone = C.c_uint64()
        check(self.ctx.lib.fgpu_vecidx_remove(self.ctx._h, self._h, _p(i), len(i), C.byref(gone)))
        return gone.value

    def get(self, id_: int):
        """The stored vector of id_ (float32[dim]), or None."""
        v = np.zeros(self.dim, dtype=np.float32)
        present = C.c_int()
        check(self.ctx.lib.fgpu_vecidx_get(self.ctx._h, self._h, C.c_uint64(id_), _p(v, C.POINTER(C.c_float)), C.byref(present)))
        return v if present.value else None

    def knn(self, queries, k: int, stats: bool = False):
        """The kk = min(k, count) nearest stored vectors of every query: (ids uint64[nq, kk], dist float64[nq, kk]), each row in
        ascending (dist, id) — and, when stats=True, a third item: the four counters [scoring launches, query tiles, bytes of
        vectors read by scoring, tied entries the id order decided]."""
        q = self._vecs(queries)
        nq = q.shape[0]
        kk = min(max(int(k), 0), self.count)
        ids = np.zeros((nq, kk), dtype=np.uint64)
        dist = np.zeros((nq, kk), dtype=np.float64)
        got = C.c_uint64()
        st = np.zeros(4, dtype=np.uint64) if stats else None
        check(self.ctx.lib.fgpu_vecidx_knn(self.ctx._h, self._h, _p(q, C.POINTER(C.c_float)), nq, C.c_uint64(max(int(k), 0)),
                                           _p(ids), _p(dist, C.POINTER(C.c_double)), C.byref(got), _p(st)))
        assert got.value == (kk if nq else 0)
        if stats:
            return ids, dist, [int(x) for x in st]
        return ids, dist


class BfsPlan:
    """fgpu_bfs_plan: resident BFS workspace (+ slab partition state for multi-rank runs)."""

    def __init__(self, ctx: Context, A: Mat, At: Mat | None, rank=0, nranks=1, splits=None):
        self.ctx, self.A, self.At = ctx, A, At
        self._h = C.c_void_p()
        self.rank, self.nranks = rank, nranks
        if splits is None:
            check(ctx.lib.fgpu_bfs_plan_create(ctx._h, C.byref(self._h), A._h, At._h if At else None, rank, nranks))
        else:   # caller-chosen (nnz-balanced) slab boundaries
            sp = _u64(splits)
            assert len(sp) == nranks + 1
            check(ctx.lib.fgpu_bfs_plan_create_slab(ctx._h, C.byref(self._h), A._h, At._h if At else None, rank,
                                                    nranks, _p(sp)))
        self.n = A.nrows

    def dist_times(self):
        """(level-kernel ms, collective ms, level launches) of this rank's last bfs_dist_run (HIP-event sums)."""
        lm, cm, nl = C.c_double(), C.c_double(), C.c_uint64()
        check(self.ctx.lib.fgpu_bfs_dist_times(self._h, C.byref(lm), C.byref(cm), C.byref(nl)))
        return lm.value, cm.value, nl.value

    def free(self):
        if self._h:
            self.ctx.lib.fgpu_bfs_plan_free(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            if self.ctx._h:
                self.free()
        except Exception:
            pass

    def tune(self, alpha=0.0, beta=0.0, force_direction=0):
        check(self.ctx.lib.fgpu_bfs_plan_tune(self._h, alpha, beta, force_direction))

    def run(self, src, max_level=-1, want_parent=False):
        check(self.ctx.lib.fgpu_bfs_run(self._h, src, max_level, 1 if want_parent else 0))

    def run_async(self, src, max_level=-1, want_parent=False, levels=0):
        check(self.ctx.lib.fgpu_bfs_run_async(self._h, src, max_level, 1 if want_parent else 0, levels))

    def wait(self):
        check(self.ctx.lib.fgpu_bfs_wait(self._h))

    def fetch(self, want_parent=False):
        level = np.zeros(self.n, dtype=np.int32)
        parent = np.zeros(self.n, dtype=np.int64) if want_parent else None
        check(self.ctx.lib.fgpu_bfs_fetch(self._h, _p(level, i32p), _p(parent, i64p)))
        return level, parent

    def stats(self):
        s = np.zeros(8, dtype=U64)
        check(self.ctx.lib.fgpu_bfs_stats(self._h, _p(s)))
        keys = ["levels", "reached", "edges_traversed", "push_levels", "pull_levels", "scanned_push",
                "scanned_pull", "last_frontier"]
        return dict(zip(keys, (int(x) for x in s)))

    def profile(self, enable=True):
        check(self.ctx.lib.fgpu_bfs_plan_profile(self._h, 1 if enable else 0))

    def profile_read(self):
        cap = 8
        names = (C.c_char_p * cap)()
        ms = (C.c_double * cap)()
        launches = (C.c_uint64 * cap)()
        ab = (C.c_uint64 * cap)()
        n = C.c_int()
        check(self.ctx.lib.fgpu_bfs_plan_profile_read(self._h, names, ms, launches, ab, cap, C.byref(n)))
        return [{"kernel": names[i].decode(), "ms": ms[i], "launches": launches[i], "alg_bytes": ab[i]}
                for i in range(n.value)]

    # ---- multi-rank stepping ----
    def part_buffers(self):
        lw, gw = C.c_void_p(), C.c_void_p()
        wpr = C.c_uint64()
        check(self.ctx.lib.fgpu_bfs_part_buffers(self._h, C.byref(lw), C.byref(gw), C.byref(wpr)))
        return lw.value, gw.value, wpr.value

    def part_set_buffers(self, local_ptr: int, global_ptr: int):
        check(self.ctx.lib.fgpu_bfs_part_set_buffers(self._h, C.c_void_p(local_ptr), C.c_void_p(global_ptr)))

    def part_begin(self, src, max_level=-1):
        check(self.ctx.lib.fgpu_bfs_part_begin(self._h, src, max_level))

    def part_step(self):
        check(self.ctx.lib.fgpu_bfs_part_step(self._h))

    def part_commit(self):
        check(self.ctx.lib.fgpu_bfs_part_commit(self._h))

    # ---- fused slab path (multi-rank v2: one kernel + one all-gather per level) ----
    def slab_set_buffers(self, send0_ptr: int, send1_ptr: int, global_ptr: int):
        check(self.ctx.lib.fgpu_bfs_slab_set_buffers(self._h, C.c_void_p(send0_ptr), C.c_void_p(send1_ptr),
                                                     C.c_void_p(global_ptr)))

    def slab_set_degrees(self, deg_ptr: int | None):
        check(self.ctx.lib.fgpu_bfs_slab_set_degrees(self._h, C.c_void_p(deg_ptr or 0)))

    def slab_begin(self, src, max_level=-1, want_parent=False):
        check(self.ctx.lib.fgpu_bfs_slab_begin(self._h, src, max_level, 1 if want_parent else 0))

    def slab_level(self) -> int:
        idx = C.c_int()
        check(self.ctx.lib.fgpu_bfs_slab_level(self._h, C.byref(idx)))
        return idx.value

    def part_done(self):
        d, l = C.c_int32(), C.c_int32()
        check(self.ctx.lib.fgpu_bfs_part_done(self._h, C.byref(d), C.byref(l)))
        return bool(d.value), l.value


def comm_init_all(ctxs):
    """fgpu_comm_init_all: one communicator over the contexts of ONE process (rank i = ctxs[i]) — the single-process
    gang form of the multi-GPU BFS (ncclCommInitAll inside libfgpu.so)."""
    ctxs = list(ctxs)
    arr = (C.c_void_p * len(ctxs))(*[c._h for c in ctxs])
    check(ctxs[0].lib.fgpu_comm_init_all(arr, len(ctxs)))


def bfs_dist_run(plans, src: int, max_level: int = -1, want_parent: bool = False):
    """fgpu_bfs_dist_run: one whole search over a column-slab partition, level loop and frontier exchange inside the
    library.  `plans` = this process' ranks: one BfsPlan (one process per GPU, RCCL communicator on its context) or
    the plans of every rank in rank order (one process drives them all)."""
    plans = list(plans)
    arr = (C.c_void_p * len(plans))(*[p._h for p in plans])
    check(plans[0].ctx.lib.fgpu_bfs_dist_run(arr, len(plans), C.c_uint64(src), C.c_int64(max_level),
                                             1 if want_parent else 0))


def bench_spmv(ctx: Context, A: Mat, which=0, iters=20):
    ms = C.c_double()
    ab = C.c_uint64()
    check(ctx.lib.fgpu_bench_spmv(ctx._h, A._h, which, iters, C.byref(ms), C.byref(ab)))
    return ms.value, ab.value


def expand_pairs(ctx: Context, src_ids, m, dp=None, dm=None, dst_label_bitmap=None, pinned_dest=None, row_bits=16):
    """fgpu_expand_pairs: the (active_row, dest) columns CondTraverseOp::expand_batch hands on, built on the device;
    pinned_dest[i] = a pre-bound destination of source row i, or 2**64 - 1.  Returns (rows, dest, flops) as numpy arrays."""
    src = _u64(src_ids)
    am = _hop_arrays(m)
    adp = _hop_arrays(dp) if dp is not None else None
    adm = _hop_arrays(dm) if dm is not None else None
    lab = _u64(dst_label_bitmap) if dst_label_bitmap is not None else None
    pin = _u64(pinned_dest) if pinned_dest is not None else None
    prow, pdest = C.c_void_p(), u64p()
    n, flops = C.c_uint64(), C.c_uint64()
    check(ctx.lib.fgpu_expand_pairs(ctx._h, _p(src), len(src), am, adp, adm, len(m), _p(lab), _p(pin), int(row_bits),
                                    C.byref(prow), C.byref(pdest), C.byref(n), C.byref(flops)))
    k = n.value
    if k == 0:
        return np.zeros(0, dtype=np.uint64), np.zeros(0, dtype=np.uint64), flops.value
    rt = np.uint16 if row_bits == 16 else np.uint32
    rows = np.ctypeslib.as_array(C.cast(prow, C.POINTER(C.c_uint16 if row_bits == 16 else C.c_uint32)), shape=(k,)).astype(np.uint64)
    dest = np.ctypeslib.as_array(pdest, shape=(k,)).copy()
    ctx.lib.fgpu_free(ctx._h, prow)
    ctx.lib.fgpu_free(ctx._h, pdest)
    return rows, dest, flops.value


def expand_exists(ctx: Context, src_ids, m, dp=None, dm=None, dst_label_bitmap=None):
    """fgpu_expand_exists: match[i] = row i of fgpu_expand over the same arguments is non-empty (the pattern predicate of
    SemiApply); the last hop is not expanded.  Returns (match as a bool array, flops of the hops that ran, stats = [rows
    matched, undecided rows sent through the exact pass, adjacency entries the last step read, 0 CSR frontier / 1 bit state])."""
    src = _u64(src_ids)
    am = _hop_arrays(m)
    adp = _hop_arrays(dp) if dp is not None else None
    adm = _hop_arrays(dm) if dm is not None else None
    lab = _u64(dst_label_bitmap) if dst_label_bitmap is not None else None
    words = np.full(max((len(src) + 63) // 64, 1), 2**64 - 1, dtype=np.uint64)   # (the call clears its words, padding included)
    flops = C.c_uint64()
    stats = np.zeros(4, dtype=np.uint64)
    check(ctx.lib.fgpu_expand_exists(ctx._h, _p(src), len(src), am, adp, adm, len(m), _p(lab), words.ctypes.data_as(u64p),
                                     C.byref(flops), stats.ctypes.data_as(u64p)))
    if len(src) == 0:
        return np.zeros(0, dtype=bool), flops.value, [int(x) for x in stats]
    bits = np.unpackbits(words.view(np.uint8), bitorder="little")
    assert not bits[len(src):].any(), "fgpu_expand_exists left padding bits set"
    return bits[:len(src)].astype(bool), flops.value, [int(x) for x in stats]


def expand_probe(ctx: Context, src_ids, dst_ids, m, dp=None, dm=None, dst_label_bitmap=None):
    """fgpu_expand_probe: present[i] = dst_ids[i] is reached from src_ids[i] by the chain (every row of the batch has a
    pre-bound destination); returns (present as a bool array, flops of the hops that ran)."""
    src, dst = _u64(src_ids), _u64(dst_ids)
    assert len(src) == len(dst)
    am = _hop_arrays(m)
    adp = _hop_arrays(dp) if dp is not None else None
    adm = _hop_arrays(dm) if dm is not None else None
    lab = _u64(dst_label_bitmap) if dst_label_bitmap is not None else None
    out = np.zeros(max(len(src), 1), dtype=np.uint8)
    flops = C.c_uint64()
    check(ctx.lib.fgpu_expand_probe(ctx._h, _p(src), _p(dst), len(src), am, adp, adm, len(m), _p(lab),
                                    out.ctypes.data_as(u8p), C.byref(flops)))
    return out[:len(src)].astype(bool), flops.value
