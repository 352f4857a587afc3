"""ctypes handles over libfalkor_host.so (include/falkor_host.h) — the C++ host layer that mirrors
FalkorDB's Matrix / VersionedMatrix / Tensor / Graph slice and the CondTraverse / ExpandInto / algo.BFS
operators above the device C ABI.  Test and embedding plumbing only; nothing is computed here."""
from __future__ import annotations

import ctypes as C
import os
import re

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libfalkor_host.so")
HEADER = os.path.join(os.path.dirname(_HERE), "include", "falkor_host.h")
_lib = None

u64p = C.POINTER(C.c_uint64)
i64p = C.POINTER(C.c_int64)


class HostError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"falkor_host error {code}: {msg}")
        self.code = code


def declared_symbols():
    """Function names declared in include/falkor_host.h."""
    with open(HEADER) as f:
        src = f.read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(fh_[a-z0-9_]+)\s*\(", src)))


def load():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            from . import build
            build.build_host()
        L = C.CDLL(LIB_PATH)
        L.fh_last_error.restype = C.c_char_p
        L.fh_free.argtypes = [C.c_void_p]
        L.fh_free.restype = None
        for name in declared_symbols():
            fn = getattr(L, name)  # raises if the library lacks a declared symbol
            if name not in ("fh_last_error", "fh_free", "fh_finalize", "fh_mat_free", "fh_vm_free", "fh_graph_free",
                            "fh_last_op_ns", "fh_mat_cursor_free", "fh_tn_free"):
                fn.restype = C.c_int
        for name in ("fh_finalize", "fh_mat_free", "fh_vm_free", "fh_graph_free", "fh_mat_cursor_free", "fh_tn_free"):
            getattr(L, name).restype = None
            getattr(L, name).argtypes = [C.c_void_p]
        L.fh_last_op_ns.restype = C.c_uint64
        _lib = L
    return _lib


def _attr_arrays(attr):
    """an attribute as the C API takes it, (ids uint64[], values float64[]): a {relationship id: number} dict, or a sequence of
    (relationship id, number) pairs in any order — of a repeated id the last pair stands"""
    pairs = list(attr.items()) if hasattr(attr, "items") else list(attr)
    return (np.ascontiguousarray([int(k) for k, _ in pairs], dtype=np.uint64),
            np.ascontiguousarray([float(v) for _, v in pairs], dtype=np.float64))


def _ck(code, allow=(0,)):
    if code not in allow:
        raise HostError(code, (load().fh_last_error() or b"").decode())
    return code


def _u64(x):
    return np.ascontiguousarray(x, dtype=np.uint64)


def _p(a):
    return a.ctypes.data_as(u64p)


def _take(ptr, n, dtype=np.uint64):
    L = load()
    if not ptr:
        return np.zeros(0, dtype=dtype)
    out = np.ctypeslib.as_array(ptr, shape=(max(n, 1),))[:n].astype(dtype, copy=True)
    L.fh_free(C.cast(ptr, C.c_void_p))
    return out


def _f32(x):
    return np.ascontiguousarray(x, dtype=np.float32).reshape(-1)


def _pf(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def vec_distance(metric, a, b):
    """vec.euclideanDistance / vec.cosineDistance (and the ip metric) in FP64 on the host (fh_vec_distance; no GPU)"""
    x, y = _f32(a), _f32(b)
    out = C.c_double()
    _ck(load().fh_vec_distance(metric.encode(), _pf(x), C.c_uint64(x.size), _pf(y), C.c_uint64(y.size), C.byref(out)))
    return out.value


def betweenness_sources(n_nodes, sampling_size=16, sampling_seed=0):
    """algo.betweenness' source indices out of 0..n_nodes (fh_betweenness_sources; no GPU)"""
    out = u64p()
    n = C.c_uint64()
    _ck(load().fh_betweenness_sources(C.c_uint64(n_nodes), C.c_int64(sampling_size), C.c_int64(sampling_seed), C.byref(out),
                                      C.byref(n)))
    return _take(out, n.value)


def should_fold(d, tx, base):
    return bool(load().fh_should_fold(C.c_uint64(d), C.c_uint64(tx), C.c_uint64(base)))


def should_fold_read(d, tx, base):
    return bool(load().fh_should_fold_read(C.c_uint64(d), C.c_uint64(tx), C.c_uint64(base)))


def delta_dominates_base(d, base):
    return bool(load().fh_delta_dominates_base(C.c_uint64(d), C.c_uint64(base)))


def compound_key(src, dst):
    k = C.c_uint64()
    _ck(load().fh_compound_key(C.c_uint64(src), C.c_uint64(dst), C.byref(k)))
    return k.value


class Context:
    def __init__(self, device=0):
        self.L = load()
        self.h = C.c_void_p()
        _ck(self.L.fh_init(C.byref(self.h), device))

    def close(self):
        if self.h:
            self.L.fh_finalize(self.h)
            self.h = C.c_void_p()


class MatrixCursor:
    """fh_mat_cursor_*: Iter::new / seek / next (matrix.rs:1471-1605); keeps its matrix alive."""

    def __init__(self, m, min_row, max_row, batch=4096):
        self.m, self.L, self.batch = m, m.L, batch
        self.h = C.c_void_p()
        _ck(self.L.fh_mat_cursor_new(m.h, C.c_uint64(min_row), C.c_uint64(max_row), C.byref(self.h)))

    def seek(self, min_row, max_row):
        _ck(self.L.fh_mat_cursor_seek(self.h, C.c_uint64(min_row), C.c_uint64(max_row)))
        return self

    def __iter__(self):
        r, c, v = (np.zeros(self.batch, dtype=np.uint64) for _ in range(3))
        n = C.c_uint64()
        while True:
            _ck(self.L.fh_mat_cursor_next(self.h, C.c_uint64(self.batch), _p(r), _p(c), _p(v), C.byref(n)))
            yield from zip(r[:n.value].tolist(), c[:n.value].tolist(), v[:n.value].tolist())
            if n.value < self.batch:
                return

    def __del__(self):
        try:
            if self.h:
                self.L.fh_mat_cursor_free(self.h)
        except Exception:
            pass


class Matrix:
    BOOL, UINT64 = 0, 1

    def __init__(self, ctx, typ=0, nrows=0, ncols=0, _h=None):
        self.ctx, self.L = ctx, ctx.L
        self.h = _h if _h is not None else C.c_void_p()
        if _h is None:
            _ck(self.L.fh_mat_new(ctx.h, C.byref(self.h), typ, C.c_uint64(nrows), C.c_uint64(ncols)))

    def __del__(self):
        try:
            if self.h and self.ctx.h:
                self.L.fh_mat_free(self.h)
        except Exception:
            pass

    def _wrap(self, h):
        return Matrix(self.ctx, _h=h)

    def build(self, rows, cols, vals=None):
        r, c = _u64(rows), _u64(cols)
        v = _u64(vals) if vals is not None else None
        _ck(self.L.fh_mat_build(self.h, _p(r), _p(c), _p(v) if v is not None else None, C.c_uint64(len(r))))

    def set(self, i, j, v=1):
        _ck(self.L.fh_mat_set(self.h, C.c_uint64(i), C.c_uint64(j), C.c_uint64(v)))

    def remove(self, i, j):
        _ck(self.L.fh_mat_remove(self.h, C.c_uint64(i), C.c_uint64(j)))

    def get(self, i, j):
        v = C.c_uint64()
        code = _ck(self.L.fh_mat_get(self.h, C.c_uint64(i), C.c_uint64(j), C.byref(v)), allow=(0, 1))
        return None if code == 1 else v.value

    def nvals(self):
        v = C.c_uint64()
        _ck(self.L.fh_mat_nvals(self.h, C.byref(v)))
        return v.value

    def dims(self):
        a, b = C.c_uint64(), C.c_uint64()
        _ck(self.L.fh_mat_dims(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def pending(self):
        v = C.c_int()
        _ck(self.L.fh_mat_pending(self.h, C.byref(v)))
        return bool(v.value)

    def wait(self):
        _ck(self.L.fh_mat_wait(self.h))

    def iter(self, min_row=0, max_row=2**64 - 1):
        r, c, v = u64p(), u64p(), u64p()
        n = C.c_uint64()
        _ck(self.L.fh_mat_iter(self.h, C.c_uint64(min_row), C.c_uint64(max_row), C.byref(r), C.byref(c), C.byref(v),
                               C.byref(n)))
        return list(zip(_take(r, n.value).tolist(), _take(c, n.value).tolist(), _take(v, n.value).tolist()))

    def cursor(self, min_row=0, max_row=2**64 - 1):
        """matrix::Iter as a reusable streaming cursor: .seek(min, max), iteration yields (row, col, val)."""
        return MatrixCursor(self, min_row, max_row)

    def _unary(self, fn, *args):
        h = C.c_void_p()
        _ck(fn(self.h, *args, C.byref(h)))
        return self._wrap(h)

    def dup(self):
        return self._unary(self.L.fh_mat_dup)

    def transpose(self):
        return self._unary(self.L.fh_mat_transpose)

    def grown(self, nrows, ncols):
        return self._unary(self.L.fh_mat_grown, C.c_uint64(nrows), C.c_uint64(ncols))

    def resize(self, nrows, ncols):
        _ck(self.L.fh_mat_resize(self.h, C.c_uint64(nrows), C.c_uint64(ncols)))

    def lmxm(self, b):
        _ck(self.L.fh_mat_lmxm(self.h, b.h))

    def rmxm(self, b):
        _ck(self.L.fh_mat_rmxm(self.h, b.h))

    def delta_lmxm(self, m, dp, dm):
        _ck(self.L.fh_mat_delta_lmxm(self.h, m.h, dp.h, dm.h))

    def intersection_nvals(self, b):
        v = C.c_uint64()
        _ck(self.L.fh_mat_intersection_nvals(self.h, b.h, C.byref(v)))
        return v.value


class VersionedMatrix:
    def __init__(self, ctx, nrows=0, ncols=0, _h=None):
        self.ctx, self.L = ctx, ctx.L
        self.h = _h if _h is not None else C.c_void_p()
        if _h is None:
            _ck(self.L.fh_vm_new(ctx.h, C.byref(self.h), C.c_uint64(nrows), C.c_uint64(ncols)))

    @classmethod
    def from_coo(cls, ctx, nrows, ncols, rows, cols):
        r, c = _u64(rows), _u64(cols)
        h = C.c_void_p()
        _ck(ctx.L.fh_vm_from_coo(ctx.h, C.byref(h), C.c_uint64(nrows), C.c_uint64(ncols), _p(r), _p(c),
                                 C.c_uint64(len(r))))
        return cls(ctx, _h=h)

    def __del__(self):
        try:
            if self.h and self.ctx.h:
                self.L.fh_vm_free(self.h)
        except Exception:
            pass

    def set(self, i, j, _v=True):
        _ck(self.L.fh_vm_set(self.h, C.c_uint64(i), C.c_uint64(j)))

    def remove(self, i, j):
        _ck(self.L.fh_vm_remove(self.h, C.c_uint64(i), C.c_uint64(j)))

    def get(self, i, j):
        return True if _ck(self.L.fh_vm_get(self.h, C.c_uint64(i), C.c_uint64(j)), allow=(0, 1)) == 0 else None

    def nvals(self):
        v = C.c_uint64()
        _ck(self.L.fh_vm_nvals(self.h, C.byref(v)))
        return v.value

    def iter(self, min_row=0, max_row=2**64 - 1):
        r, c = u64p(), u64p()
        n = C.c_uint64()
        _ck(self.L.fh_vm_iter(self.h, C.c_uint64(min_row), C.c_uint64(max_row), C.byref(r), C.byref(c), C.byref(n)))
        return list(zip(_take(r, n.value).tolist(), _take(c, n.value).tolist()))

    def set_all(self, entries, new=False):
        e = list(entries)
        r, c = _u64([x[0] for x in e]), _u64([x[1] for x in e])
        _ck(self.L.fh_vm_set_all(self.h, _p(r), _p(c), C.c_uint64(len(e)), 1 if new else 0))

    def remove_mask(self, entries):
        e = list(entries)
        r, c = _u64([x[0] for x in e]), _u64([x[1] for x in e])
        _ck(self.L.fh_vm_remove_mask(self.h, _p(r), _p(c), C.c_uint64(len(e))))

    def dup(self):
        h = C.c_void_p()
        _ck(self.L.fh_vm_dup(self.h, C.byref(h)))
        return VersionedMatrix(self.ctx, _h=h)

    def transpose(self):
        h = C.c_void_p()
        _ck(self.L.fh_vm_transpose(self.h, C.byref(h)))
        return VersionedMatrix(self.ctx, _h=h)

    def wait(self):
        _ck(self.L.fh_vm_wait(self.h))

    def flush(self):
        _ck(self.L.fh_vm_flush(self.h))

    def fold_oversized(self):
        _ck(self.L.fh_vm_fold_oversized(self.h))

    def extract(self):
        h = C.c_void_p()
        _ck(self.L.fh_vm_extract(self.h, C.byref(h)))
        return Matrix(self.ctx, _h=h)

    def state(self):
        s = (C.c_uint64 * 4)()
        _ck(self.L.fh_vm_state(self.h, s))
        return {"m": s[0], "dp": s[1], "dm": s[2], "needs_flush": bool(s[3])}


def cond_spec(src_labels=(), hops=((), ()), optional=False, bind=False, emit=False, bidir=False, siblings=False,
              attrs=False, transposed=False):
    """hops: sequence of (types, dst_labels); hop 0 is the operator's own pattern, the rest the fused chain."""
    parts = ["src=" + ",".join(src_labels)]
    for types, labels in hops:
        parts.append("hop=" + ",".join(types) + "|" + ",".join(labels))
    for k, v in (("optional", optional), ("bind", bind), ("emit", emit), ("bidir", bidir), ("siblings", siblings),
                 ("attrs", attrs), ("transposed", transposed)):
        parts.append(f"{k}={1 if v else 0}")
    return ";".join(parts).encode()


class Graph:
    def __init__(self, ctx, node_cap):
        self.ctx, self.L = ctx, ctx.L
        self.h = C.c_void_p()
        self.n = node_cap
        _ck(self.L.fh_graph_new(ctx.h, C.byref(self.h), C.c_uint64(node_cap)))

    def __del__(self):
        try:
            if self.h and self.ctx.h:
                self.L.fh_graph_free(self.h)
        except Exception:
            pass

    def add_label(self, name):
        v = C.c_uint64()
        _ck(self.L.fh_graph_add_label(self.h, name.encode(), C.byref(v)))
        return v.value

    def add_type(self, name):
        v = C.c_uint64()
        _ck(self.L.fh_graph_add_type(self.h, name.encode(), C.byref(v)))
        return v.value

    def label_node(self, node, label_id):
        _ck(self.L.fh_graph_label_node(self.h, C.c_uint64(node), C.c_uint64(label_id)))

    def delete_node(self, node):
        _ck(self.L.fh_graph_delete_node(self.h, C.c_uint64(node)))

    def create_edge(self, type_id, src, dst, edge_id):
        _ck(self.L.fh_graph_create_edge(self.h, C.c_uint64(type_id), C.c_uint64(src), C.c_uint64(dst),
                                        C.c_uint64(edge_id)))

    def create_edges(self, type_id, srcs, dsts, ids):
        s, d, i = _u64(srcs), _u64(dsts), _u64(ids)
        _ck(self.L.fh_graph_create_edges(self.h, C.c_uint64(type_id), _p(s), _p(d), _p(i), C.c_uint64(len(s))))

    def bulk_insert_edges(self, type_id, srcs, dsts, ids):
        """fh_graph_bulk_insert_edges: one type's bulk batch through the device build; returns what it did as a dict."""
        s, d, i = _u64(srcs), _u64(dsts), _u64(ids)
        if not (len(s) == len(d) == len(i)):
            raise ValueError("bulk_insert_edges: srcs, dsts and ids differ in length")
        st = (C.c_uint64 * 6)()
        _ck(self.L.fh_graph_bulk_insert_edges(self.h, C.c_uint64(type_id), _p(s), _p(d), _p(i), C.c_uint64(len(s)), st))
        return dict(zip(("device_edges", "fallback_edges", "distinct_pairs", "multi_pairs", "unsorted_runs", "host_sorted_runs"),
                        (int(x) for x in st)))

    def last_bulk_phases_ms(self):
        """fh_last_bulk_phases_ns: host-clock ms of the last bulk_insert_edges of this thread, by phase."""
        ns = (C.c_uint64 * 4)()
        _ck(self.L.fh_last_bulk_phases_ns(ns))
        return dict(zip(("edges_build", "fold_adopt", "me_fill", "adjacency_union"), (x / 1e6 for x in ns)))

    def append_edges_bulk(self, type_id, srcs, dsts, ids):
        """fh_graph_append_edges_bulk: one type's batch onto a graph that holds edges, every edge through the device (pairs that
        hold an edge already are promoted or extended there); returns what it did as a dict."""
        s, d, i = _u64(srcs).reshape(-1), _u64(dsts).reshape(-1), _u64(ids).reshape(-1)
        if not (len(s) == len(d) == len(i)):
            raise ValueError("append_edges_bulk: srcs, dsts and ids differ in length")
        st = (C.c_uint64 * 8)()
        _ck(self.L.fh_graph_append_edges_bulk(self.h, C.c_uint64(type_id), _p(s), _p(d), _p(i), C.c_uint64(len(s)), st))
        return dict(zip(("edges", "distinct_pairs", "multi_pairs", "colliding_pairs", "promoted_pairs", "extended_pairs", "me_rows",
                         "host_sorted_runs"), (int(x) for x in st)))

    def last_append_phases_ms(self):
        """fh_last_append_phases_ns: host-clock ms of the last append_edges_bulk of this thread, by phase."""
        ns = (C.c_uint64 * 4)()
        _ck(self.L.fh_last_append_phases_ns(ns))
        return dict(zip(("edges_build", "fold_union", "me_rewrite", "adjacency_union"), (x / 1e6 for x in ns)))

    def delete_nodes_bulk(self, nodes, skip_ids=(), stats=False, as_arrays=False):
        """fh_graph_delete_nodes_bulk: DETACH DELETE of a node set in one call.  Returns the removed edges as a list of
        (edge id, src, dst) in the reference's order (ids in skip_ids are removed too, but not listed) — as three uint64
        arrays (ids, srcs, dsts) with as_arrays=True; with stats=True also what it did as a dict."""
        v, k = _u64(nodes).reshape(-1), _u64(list(skip_ids)).reshape(-1)
        i, s, d = u64p(), u64p(), u64p()
        n = C.c_uint64()
        st = (C.c_uint64 * 6)()
        _ck(self.L.fh_graph_delete_nodes_bulk(self.h, _p(v), C.c_uint64(len(v)), _p(k), C.c_uint64(len(k)), C.byref(i), C.byref(s),
                                              C.byref(d), C.byref(n), st))
        rels = (_take(i, n.value), _take(s, n.value), _take(d, n.value))
        if not as_arrays:
            rels = list(zip(*(x.tolist() for x in rels)))
        if not stats:
            return rels
        return rels, dict(zip(("nodes", "edges_removed", "edges_listed", "label_entries", "adjacency_entries", "multi_pairs"),
                              (int(x) for x in st)))

    def tensor_version(self, type_id):
        """fh_graph_tensor_version: the dup() Graph::new_version takes of one type's tensor, as a Tensor of its own."""
        h = C.c_void_p()
        _ck(self.L.fh_graph_tensor_version(self.h, C.c_uint64(type_id), C.byref(h)))
        return Tensor(self.ctx, _h=h)

    def last_detach_phases_ms(self):
        """fh_last_detach_phases_ns: host-clock ms of the last delete_nodes_bulk of this thread, by phase."""
        ns = (C.c_uint64 * 4)()
        _ck(self.L.fh_last_detach_phases_ns(ns))
        return dict(zip(("tensors_detach", "list_expand", "labels", "adjacency"), (x / 1e6 for x in ns)))

    def delete_edges_bulk(self, types, srcs, dsts, ids, stats=False, as_arrays=False):
        """fh_graph_delete_edges_bulk: DELETE r of a batch of edges in one call; `types` is one type id per edge, or one id for
        all.  Returns the removed edges as a list of (edge id, src, dst) — types ascending, input order within a type — as three
        uint64 arrays (ids, srcs, dsts) with as_arrays=True; with stats=True also what it did as a dict."""
        s, d, i = _u64(srcs).reshape(-1), _u64(dsts).reshape(-1), _u64(ids).reshape(-1)
        t = _u64(types).reshape(-1)
        if t.size == 1 and len(s) != 1:
            t = np.full(len(s), t[0], dtype=np.uint64)
        if not (len(t) == len(s) == len(d) == len(i)):
            raise ValueError("delete_edges_bulk: types, srcs, dsts and ids differ in length")
        oi, os_, od, pt = u64p(), u64p(), u64p(), u64p()
        n, nt = C.c_uint64(), C.c_uint64()
        st = (C.c_uint64 * 5)()
        _ck(self.L.fh_graph_delete_edges_bulk(self.h, _p(t), _p(s), _p(d), _p(i), C.c_uint64(len(s)), C.byref(oi), C.byref(os_),
                                              C.byref(od), C.byref(n), st, C.byref(pt), C.byref(nt)))
        rels = (_take(oi, n.value), _take(os_, n.value), _take(od, n.value))
        per_type = _take(pt, nt.value).tolist()
        if not as_arrays:
            rels = list(zip(*(x.tolist() for x in rels)))
        if not stats:
            return rels
        out = dict(zip(("edges_named", "edges_removed", "pairs_emptied", "pairs_demoted", "adjacency_entries"), (int(x) for x in st)))
        out["per_type"] = per_type
        return rels, out

    def last_edge_delete_phases_ms(self):
        """fh_last_edge_delete_phases_ns: host-clock ms of the last delete_edges_bulk of this thread, by phase."""
        ns = (C.c_uint64 * 4)()
        _ck(self.L.fh_last_edge_delete_phases_ns(ns))
        return dict(zip(("gather_rows", "edges_remove", "me_rewrite", "adjacency"), (x / 1e6 for x in ns)))

    def delete_edge(self, type_id, src, dst, edge_id):
        _ck(self.L.fh_graph_delete_edge(self.h, C.c_uint64(type_id), C.c_uint64(src), C.c_uint64(dst),
                                        C.c_uint64(edge_id)))

    def commit(self):
        _ck(self.L.fh_graph_commit(self.h))

    def node_has_label(self, node, label_id):
        return _ck(self.L.fh_graph_node_has_label(self.h, C.c_uint64(node), C.c_uint64(label_id)), allow=(0, 1)) == 0

    def tensor_get(self, type_id, src, dst):
        p, n = u64p(), C.c_uint64()
        _ck(self.L.fh_tensor_get(self.h, C.c_uint64(type_id), C.c_uint64(src), C.c_uint64(dst), C.byref(p),
                                 C.byref(n)))
        return _take(p, n.value).tolist()

    def tensor_edge_count(self, type_id):
        v = C.c_uint64()
        _ck(self.L.fh_tensor_edge_count(self.h, C.c_uint64(type_id), C.byref(v)))
        return v.value

    def tensor_iter_edges(self, type_id):
        s, d, i = u64p(), u64p(), u64p()
        n = C.c_uint64()
        _ck(self.L.fh_tensor_iter_edges(self.h, C.c_uint64(type_id), C.byref(s), C.byref(d), C.byref(i), C.byref(n)))
        return list(zip(_take(s, n.value).tolist(), _take(d, n.value).tolist(), _take(i, n.value).tolist()))

    def tensor_state(self, type_id):
        s = (C.c_uint64 * 5)()
        _ck(self.L.fh_tensor_state(self.h, C.c_uint64(type_id), s))
        return {"m": s[0], "dp": s[1], "dm": s[2], "multi_pairs": s[3], "mt": s[4]}

    def layer(self, type_id, which):
        """Raw (row, col, val) entries of one layer: type_id None = adjacency; which in 'm', 'dp', 'dm'."""
        r, c, v = u64p(), u64p(), u64p()
        n = C.c_uint64()
        _ck(self.L.fh_graph_layer_iter(self.h, C.c_int64(-1 if type_id is None else type_id),
                                       {"m": 0, "dp": 1, "dm": 2}[which], C.byref(r), C.byref(c), C.byref(v),
                                       C.byref(n)))
        return list(zip(_take(r, n.value).tolist(), _take(c, n.value).tolist(), _take(v, n.value).tolist()))

    # ---- operators -----------------------------------------------------------------------------
    def cond_traverse_batch(self, spec, src, to_bound=None, as_arrays=False):
        """src / to_bound: node id, None = bound to NULL / non-node (src) or unbound (to_bound).
        Returns None when the batched path bails to the per-row one, else (rows, null_rows, flops) with
        rows = [(active_row, dest[, edge])]."""
        k = len(src)
        s = np.asarray([(-2 if v is None else v) for v in src], dtype=np.int64)
        tb = None if to_bound is None else np.asarray([(-1 if v is None else v) for v in to_bound], dtype=np.int64)
        batched = C.c_int()
        orow, odst, onull = u64p(), u64p(), u64p()
        oedge = i64p()
        n, nn, fl = C.c_uint64(), C.c_uint64(), C.c_uint64()
        _ck(self.L.fh_cond_traverse_batch(self.h, spec, s.ctypes.data_as(i64p),
                                          tb.ctypes.data_as(i64p) if tb is not None else None, C.c_uint64(k),
                                          C.byref(batched), C.byref(orow), C.byref(odst), C.byref(oedge), C.byref(n),
                                          C.byref(onull), C.byref(nn), C.byref(fl)))
        if as_arrays:   # numpy views of the result columns (no per-row Python objects)
            res = (_take(orow, n.value), _take(odst, n.value), _take(oedge, n.value, np.int64))
            nulls = _take(onull, nn.value)
            return (res, nulls, fl.value) if batched.value else None
        rows, dst = _take(orow, n.value).tolist(), _take(odst, n.value).tolist()
        edge = _take(oedge, n.value, np.int64).tolist()
        nulls = _take(onull, nn.value).tolist()
        if not batched.value:
            return None
        out = [(r, d) if e < 0 else (r, d, e) for r, d, e in zip(rows, dst, edge)]
        return out, nulls, fl.value

    def cond_traverse_row(self, spec, from_id=None, to_id=None, transposed=False):
        f, t, e = u64p(), u64p(), u64p()
        n = C.c_uint64()
        _ck(self.L.fh_cond_traverse_row(self.h, spec, C.c_int64(-1 if from_id is None else from_id),
                                        C.c_int64(-1 if to_id is None else to_id), 1 if transposed else 0,
                                        C.byref(f), C.byref(t), C.byref(e), C.byref(n)))
        return list(zip(_take(f, n.value).tolist(), _take(t, n.value).tolist(), _take(e, n.value).tolist()))

    def cond_traverse_rows(self, spec, from_ids, to_ids, transposed=False, used_edges=(), dedup_src=None):
        """The per-row fallback over one input batch: from / to = node id, None (unbound) or "x" (bound to a non-node).
        Returns [(row, from, to, edge)] in emission order."""
        enc = lambda v: -1 if v is None else (-2 if isinstance(v, str) else int(v))
        k = len(from_ids)
        f = (C.c_int64 * k)(*[enc(v) for v in from_ids])
        t = (C.c_int64 * k)(*[enc(v) for v in to_ids])
        dd = (C.c_int64 * k)(*[enc(v) for v in dedup_src]) if dedup_src is not None else None
        used = _u64(list(used_edges))
        orow, of, ot, oe = u64p(), u64p(), u64p(), u64p()
        n = C.c_uint64()
        _ck(self.L.fh_cond_traverse_rows(self.h, spec, f, t, dd, C.c_uint64(k), 1 if transposed else 0, _p(used),
                                         C.c_uint64(len(used)), C.byref(orow), C.byref(of), C.byref(ot), C.byref(oe),
                                         C.byref(n)))
        return list(zip(_take(orow, n.value).tolist(), _take(of, n.value).tolist(), _take(ot, n.value).tolist(),
                        _take(oe, n.value).tolist()))

    def cond_traverse_edges_batch(self, spec, from_ids, to_ids, transposed=False, used_edges=None, dedup=False,
                                  as_arrays=False):
        """The same input batch through ONE fgpu_expand_edges (fh_cond_traverse_edges_batch): from / to as cond_traverse_rows
        takes them; used_edges = None or one list of sibling-bound ids PER ROW; dedup = the caller would pass dedup_src.
        Returns None when the op declines (nothing ran), else (rows, null_rows, stats) with rows = [(row, from, to, edge)] in
        emission order — four arrays with as_arrays — and stats = fgpu_expand_edges' eight."""
        enc = lambda v: -1 if v is None else (-2 if isinstance(v, str) else int(v))
        k = len(from_ids)
        f = np.asarray([enc(v) for v in from_ids], dtype=np.int64)
        t = np.asarray([enc(v) for v in to_ids], dtype=np.int64)
        used, n_used = None, 0
        if used_edges is not None:
            n_used = max((len(u) for u in used_edges), default=0)
            used = np.full((k, max(n_used, 1)), (1 << 64) - 1, dtype=np.uint64)
            for i, u in enumerate(used_edges):
                used[i, :len(u)] = list(u)
            used = np.ascontiguousarray(used[:, :n_used]) if n_used else None
        batched = C.c_int()
        orow, of, ot, oe, onull = u64p(), u64p(), u64p(), u64p(), u64p()
        n, nn = C.c_uint64(), C.c_uint64()
        st = (C.c_uint64 * 8)()
        _ck(self.L.fh_cond_traverse_edges_batch(self.h, spec, f.ctypes.data_as(i64p), t.ctypes.data_as(i64p), C.c_uint64(k),
                                                1 if transposed else 0, 1 if dedup else 0, _p(used) if used is not None else None,
                                                C.c_uint64(n_used), C.byref(batched), C.byref(orow), C.byref(of), C.byref(ot),
                                                C.byref(oe), C.byref(n), C.byref(onull), C.byref(nn), st))
        cols = [_take(p, n.value) for p in (orow, of, ot, oe)]
        nulls = _take(onull, nn.value)
        if not batched.value:
            return None
        if as_arrays:
            return cols, nulls, list(st)
        return list(zip(*(c.tolist() for c in cols))), nulls.tolist(), list(st)

    SEMI_TIERS = {0: "none", 1: "exists", 2: "collect", 3: "rows"}

    def semi_apply(self, spec, from_ids, to_ids=None, anti=False, transposed=False, device_exists=True):
        """SemiApplyOp::filter_batch (fh_semi_apply): the rows that pass the pattern predicate `spec` — from / to as
        cond_traverse_rows takes them (None unbound, a str Null / non-node), to_ids=None when no row has it bound.  Returns
        (passing rows ascending, tier name, [fgpu_expand_exists' four stats summed, calls])."""
        enc = lambda v: -1 if v is None else (-2 if isinstance(v, str) else int(v))
        k = len(from_ids)
        f = np.asarray([enc(v) for v in from_ids], dtype=np.int64)
        t = np.asarray([enc(v) for v in to_ids], dtype=np.int64) if to_ids is not None else None
        out, n, tier = u64p(), C.c_uint64(), C.c_int()
        st = (C.c_uint64 * 5)()
        _ck(self.L.fh_semi_apply(self.h, spec, 1 if anti else 0, 1 if device_exists else 0, f.ctypes.data_as(i64p),
                                 t.ctypes.data_as(i64p) if t is not None else None, C.c_uint64(k), 1 if transposed else 0,
                                 C.byref(out), C.byref(n), C.byref(tier), st))
        return _take(out, n.value).tolist(), self.SEMI_TIERS[tier.value], list(st)

    def or_apply(self, branches, from_ids, to_ids=None, device_exists=True):
        """OrApplyMultiplexerOp::filter_batch (fh_or_apply).  branches: (spec or a boolean column, anti) or (spec, anti,
        transposed).  Returns (passing rows ascending, [tier name per branch], [stats per branch])."""
        enc = lambda v: -1 if v is None else (-2 if isinstance(v, str) else int(v))
        k, nb = len(from_ids), len(branches)
        f = np.asarray([enc(v) for v in from_ids], dtype=np.int64)
        t = np.asarray([enc(v) for v in to_ids], dtype=np.int64) if to_ids is not None else None
        specs = (C.c_char_p * nb)()
        cols = (C.POINTER(C.c_uint8) * nb)()
        anti, tr = (C.c_int * nb)(), (C.c_int * nb)()
        keep = []
        for b, br in enumerate(branches):
            what = br[0]
            anti[b] = 1 if br[1] else 0
            tr[b] = 1 if len(br) > 2 and br[2] else 0
            if isinstance(what, (bytes, str)):
                specs[b] = what if isinstance(what, bytes) else what.encode()
            else:
                col = np.ascontiguousarray(np.asarray(what, dtype=bool).astype(np.uint8))
                assert len(col) == k
                keep.append(col)
                cols[b] = col.ctypes.data_as(C.POINTER(C.c_uint8))
        out, n = u64p(), C.c_uint64()
        tiers = (C.c_int * nb)()
        st = (C.c_uint64 * (5 * nb))()
        _ck(self.L.fh_or_apply(self.h, specs, cols, anti, tr, nb, 1 if device_exists else 0, f.ctypes.data_as(i64p),
                               t.ctypes.data_as(i64p) if t is not None else None, C.c_uint64(k), C.byref(out), C.byref(n),
                               tiers, st))
        return (_take(out, n.value).tolist(), [self.SEMI_TIERS[x] for x in tiers],
                [list(st[5 * b:5 * b + 5]) for b in range(nb)])

    def expand_into(self, types, srcs, dsts, bidirectional=False, emit_relationship=True, batched=True):
        s, d = _u64(srcs), _u64(dsts)
        orow, osrc, odst, oedge = u64p(), u64p(), u64p(), u64p()
        n = C.c_uint64()
        _ck(self.L.fh_expand_into(self.h, ",".join(types).encode(), 1 if bidirectional else 0,
                                  1 if emit_relationship else 0, 1 if batched else 0, _p(s), _p(d),
                                  C.c_uint64(len(s)), C.byref(orow), C.byref(osrc), C.byref(odst), C.byref(oedge),
                                  C.byref(n)))
        return list(zip(_take(orow, n.value).tolist(), _take(osrc, n.value).tolist(),
                        _take(odst, n.value).tolist(), _take(oedge, n.value).tolist()))

    def var_len_traverse(self, start, types=(), dest=None, min_hops=1, max_hops=None, reversed=False,
                         bidirectional=False, dst_labels=(), emit_path=False, prune=True):
        """CondVarLenTraverse over one input row (cond_var_len_traverse.rs:81-387): [(from, to, path | None)] in the
        reference's emission order, plus {frames, pruned, reach_products}."""
        of, ot, op_, off = u64p(), u64p(), u64p(), u64p()
        n = C.c_uint64()
        st = (C.c_uint64 * 3)()
        _ck(self.L.fh_var_len_traverse(self.h, ",".join(types).encode(), ",".join(dst_labels).encode(),
                                       1 if reversed else 0, 1 if bidirectional else 0, C.c_uint32(min_hops),
                                       C.c_uint32(0xFFFFFFFF if max_hops is None else max_hops), C.c_uint64(start),
                                       C.c_int64(-1 if dest is None else dest), 1 if emit_path else 0, 1 if prune else 0,
                                       C.byref(of), C.byref(ot), C.byref(op_), C.byref(off), C.byref(n), st))
        k = n.value
        offs = _take(off, k + 1).tolist()
        f, t = _take(of, k).tolist(), _take(ot, k).tolist()
        p = _take(op_, offs[-1]).tolist()
        rows = [(f[i], t[i], p[offs[i]:offs[i + 1]] if emit_path else None) for i in range(k)]
        return rows, {"frames": int(st[0]), "pruned": int(st[1]), "reach_products": int(st[2])}

    def var_len_traverse_batch(self, starts, dests=None, types=(), min_hops=1, max_hops=None, reversed=False, bidirectional=False,
                               dst_labels=(), emit_path=False, prune=True, device_budget=None, as_arrays=False):
        """CondVarLenTraverse over an input batch on the device (fh_var_len_traverse_batch, fgpu_expand_trails underneath):
        [(row, from, to, path | None)] — row i's part is what var_len_traverse(starts[i], dest=dests[i]) gives — plus {frames,
        pruned, reach_products, device_calls}.  dests: None, or per row a node id or None.  device_budget: frames + emissions
        one device call may hold (None = the operator's default); a batch past it is bisected.  as_arrays: the columns (row,
        from, to, path, path_off) as numpy arrays instead of the row tuples."""
        s = _u64(starts)
        d = None if dests is None else np.asarray([-1 if v is None else int(v) for v in dests], dtype=np.int64)
        orow, of, ot, op_, off = u64p(), u64p(), u64p(), u64p(), u64p()
        n, calls = C.c_uint64(), C.c_uint64()
        st = (C.c_uint64 * 3)()
        _ck(self.L.fh_var_len_traverse_batch(self.h, ",".join(types).encode(), ",".join(dst_labels).encode(),
                                             1 if reversed else 0, 1 if bidirectional else 0, C.c_uint32(min_hops),
                                             C.c_uint32(0xFFFFFFFF if max_hops is None else max_hops), _p(s),
                                             d.ctypes.data_as(i64p) if d is not None else None, C.c_uint64(len(s)),
                                             1 if emit_path else 0, 1 if prune else 0, C.c_uint64(device_budget or 0),
                                             C.byref(orow), C.byref(of), C.byref(ot), C.byref(op_), C.byref(off), C.byref(n), st,
                                             C.byref(calls)))
        k = n.value
        stats = {"frames": int(st[0]), "pruned": int(st[1]), "reach_products": int(st[2]), "device_calls": int(calls.value)}
        if as_arrays:
            offs = _take(off, k + 1)
            return (_take(orow, k), _take(of, k), _take(ot, k), _take(op_, int(offs[-1])), offs), stats
        offs = _take(off, k + 1).tolist()
        r, f, t = _take(orow, k).tolist(), _take(of, k).tolist(), _take(ot, k).tolist()
        p = _take(op_, offs[-1]).tolist()
        rows = [(r[i], f[i], t[i], p[offs[i]:offs[i + 1]] if emit_path else None) for i in range(k)]
        return rows, stats

    def all_shortest_paths(self, src, dst, types=(), bidirectional=False, reversed=False, max_hops=None, limit=0):
        """AllShortestPathsOp over one input row (all_shortest_paths.rs:82-303): (length, [[relationship id, ...], ...]) — the
        shortest paths of allShortestPaths((src)-[:types*..max_hops]->(dst)) in the reference's emission order, src / dst the
        pattern's from / to node (src == dst: the shortest cycles); length -1 and no path when dst is out of reach.  limit > 0
        stops after that many paths."""
        oe, off = u64p(), u64p()
        n, length = C.c_uint64(), C.c_int64()
        _ck(self.L.fh_all_shortest_paths(self.h, ",".join(types).encode(), 1 if bidirectional else 0, 1 if reversed else 0,
                                         C.c_uint32(0xFFFFFFFF if max_hops is None else max_hops), C.c_uint64(src),
                                         C.c_uint64(dst), C.c_uint64(limit), C.byref(length), C.byref(oe), C.byref(off),
                                         C.byref(n)))
        offs = _take(off, n.value + 1).tolist()
        e = _take(oe, offs[-1]).tolist()
        return length.value, [e[offs[i]:offs[i + 1]] for i in range(n.value)]

    def all_shortest_paths_batch(self, srcs, dsts, types=(), bidirectional=False, reversed=False, max_hops=None, limit=0,
                                 stats=False):
        """AllShortestPathsOp over a parent batch of input rows: [(length, paths), ...], row i what all_shortest_paths(srcs[i],
        dsts[i], ...) returns.  The adjacency is built once and one device call serves every row; a row with an out-of-range or
        deleted node, and every row under an unknown type, is (-1, []).  stats=True: a second item {"device_calls": 0 | 1}."""
        s, d = np.ascontiguousarray(srcs, dtype=np.uint64), np.ascontiguousarray(dsts, dtype=np.uint64)
        assert len(s) == len(d)
        count = len(s)
        oe, off = u64p(), u64p()
        lengths = np.zeros(count, dtype=np.int64)
        row_off = np.zeros(count + 1, dtype=np.uint64)
        calls = C.c_uint64()
        _ck(self.L.fh_all_shortest_paths_batch(self.h, ",".join(types).encode(), 1 if bidirectional else 0, 1 if reversed else 0,
                                               C.c_uint32(0xFFFFFFFF if max_hops is None else max_hops),
                                               s.ctypes.data_as(u64p), d.ctypes.data_as(u64p), C.c_uint64(count), C.c_uint64(limit),
                                               lengths.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(oe), C.byref(off),
                                               row_off.ctypes.data_as(u64p), C.byref(calls)))
        ro = row_off.tolist()
        offs = _take(off, ro[-1] + 1).tolist()
        e = _take(oe, offs[-1]).tolist()
        rows = [(int(lengths[i]), [e[offs[p]:offs[p + 1]] for p in range(ro[i], ro[i + 1])]) for i in range(count)]
        return (rows, {"device_calls": int(calls.value)}) if stats else rows

    @staticmethod
    def _sp_endpoint(v):
        """an endpoint of shortest_path: a node id, None for Null, anything else for a value that is not a node"""
        if v is None:
            return -1
        return int(v) if isinstance(v, (int, np.integer)) and not isinstance(v, bool) and v >= 0 else -2

    def shortest_path(self, src, dst, types=(), directed=True, min_hops=1, max_hops=None):
        """shortestPath((src)-[:types*min_hops..max_hops]->(dst)) for one row, on the host (eval.rs:1301-1513): (nodes, edges) —
        the node ids of the ONE path the reference returns and the relationship of each consecutive pair (a pair without one
        adds none) — or None without a path.  src / dst: a node id, None for Null (-> None); any other value raises "A
        shortestPath requires bound nodes".  min_hops 0 with src == dst is ([src], [])."""
        on, oe = u64p(), u64p()
        nn, ne, null = C.c_uint64(), C.c_uint64(), C.c_int()
        _ck(self.L.fh_shortest_path(self.h, ",".join(types).encode(), 1 if directed else 0, C.c_uint32(min_hops),
                                    C.c_uint32(0xFFFFFFFF if max_hops is None else max_hops), C.c_int64(self._sp_endpoint(src)),
                                    C.c_int64(self._sp_endpoint(dst)), C.byref(null), C.byref(on), C.byref(nn), C.byref(oe),
                                    C.byref(ne)))
        nodes, edges = _take(on, nn.value).tolist(), _take(oe, ne.value).tolist()
        return None if null.value else (nodes, edges)

    def shortest_path_batch(self, srcs, dsts, types=(), directed=True, min_hops=1, max_hops=None, stats=False):
        """shortestPath() over a parent batch of rows: [(nodes, edges) | None, ...], row i what shortest_path(srcs[i], dsts[i],
        ...) returns.  The patterns are built once and ONE fgpu_shortest_path_batch call serves every row whose two nodes are in
        range, alive and different; the other rows are evaluated on the host.  stats=True: a second item {"device_calls":
        0 | 1}."""
        s = np.asarray([self._sp_endpoint(v) for v in srcs], dtype=np.int64)
        d = np.asarray([self._sp_endpoint(v) for v in dsts], dtype=np.int64)
        assert len(s) == len(d)
        count = len(s)
        on, oe = u64p(), u64p()
        null = np.zeros(max(count, 1), dtype=np.uint8)
        noff, eoff = np.zeros(count + 1, dtype=np.uint64), np.zeros(count + 1, dtype=np.uint64)
        calls = C.c_uint64()
        _ck(self.L.fh_shortest_path_batch(self.h, ",".join(types).encode(), 1 if directed else 0, C.c_uint32(min_hops),
                                          C.c_uint32(0xFFFFFFFF if max_hops is None else max_hops), s.ctypes.data_as(i64p),
                                          d.ctypes.data_as(i64p), C.c_uint64(count), null.ctypes.data_as(C.POINTER(C.c_uint8)),
                                          C.byref(on), noff.ctypes.data_as(u64p), C.byref(oe), eoff.ctypes.data_as(u64p),
                                          C.byref(calls)))
        no, eo = noff.tolist(), eoff.tolist()
        nodes, edges = _take(on, no[-1]).tolist(), _take(oe, eo[-1]).tolist()
        rows = [None if null[i] else (nodes[no[i]:no[i + 1]], edges[eo[i]:eo[i + 1]]) for i in range(count)]
        return (rows, {"device_calls": int(calls.value)}) if stats else rows

    def node_degrees(self, ids, incoming=False, types=(), batched=True, stats=False):
        """outdegree(n [, types]) / indegree(n [, types]) (entity.rs:268-381) for the node ids `ids`: a uint64 array, one count
        per id, the relationships of a multi-edge pair counted one by one.  types: none = every tensor, a name listed twice
        counts once, unknown names are dropped, no known name answers 0.  batched: ONE fgpu_node_degrees call per 64 resolved
        tensors; False: one row at a time on the host, the reference's loop.  stats=True: a second item {"device_calls": n}."""
        v = np.ascontiguousarray(ids, dtype=np.uint64).reshape(-1)
        out = np.zeros(len(v), dtype=np.uint64)
        calls = C.c_uint64()
        _ck(self.L.fh_node_degrees(self.h, ",".join(types).encode(), 1 if incoming else 0, v.ctypes.data_as(u64p), C.c_uint64(len(v)),
                                   1 if batched else 0, out.ctypes.data_as(u64p), C.byref(calls)))
        return (out, {"device_calls": int(calls.value)}) if stats else out

    def node_degrees_all(self, incoming=False, types=()):
        """The same for every node id below the node capacity, through fgpu_node_degrees' whole-graph form: a uint64 array
        indexed by node id."""
        p, n = u64p(), C.c_uint64()
        _ck(self.L.fh_node_degrees_all(self.h, ",".join(types).encode(), 1 if incoming else 0, C.byref(p), C.byref(n)))
        return _take(p, n.value)

    def build_adjacency(self, types=(), symmetric=False):
        """Graph::build_adjacency_matrix / build_symmetric_adjacency_matrix (graph.rs:3870-3907) -> Matrix"""
        h = C.c_void_p()
        _ck(self.L.fh_graph_build_adjacency(self.h, ",".join(types).encode(), 1 if symmetric else 0, C.byref(h)))
        return Matrix(self.ctx, _h=h)

    def algo_pagerank(self, label=None, rel_type=None):
        """CALL algo.pageRank(label, relationshipType) YIELD node, score -> (nodes, scores float64)."""
        nodes = u64p()
        scores = C.POINTER(C.c_double)()
        n = C.c_uint64()
        _ck(self.L.fh_algo_pagerank(self.h, label.encode() if label is not None else None,
                                    rel_type.encode() if rel_type is not None else None, C.byref(nodes),
                                    C.byref(scores), C.byref(n)))
        return _take(nodes, n.value), _take(scores, n.value, np.float64)

    def algo_wcc(self, labels=(), types=()):
        """CALL algo.WCC({nodeLabels, relationshipTypes}) YIELD node, componentId -> (nodes, component_ids int64).  Several
        labels select the union of their nodes; with labels the componentId is a compact index (see fh_algo_wcc)."""
        nodes = u64p()
        comp = C.POINTER(C.c_int64)()
        n = C.c_uint64()
        _ck(self.L.fh_algo_wcc(self.h, ",".join(labels).encode(), ",".join(types).encode(), C.byref(nodes), C.byref(comp),
                               C.byref(n)))
        return _take(nodes, n.value), _take(comp, n.value, np.int64)

    def algo_label_propagation(self, labels=(), types=(), max_iterations=10):
        """CALL algo.labelPropagation({nodeLabels, relationshipTypes, maxIterations}) YIELD node, communityId ->
        (nodes, community_ids int64).  Several labels select the union of their nodes; with labels the communityId is a compact
        index (see fh_algo_cdlp)."""
        nodes = u64p()
        comm = C.POINTER(C.c_int64)()
        n = C.c_uint64()
        _ck(self.L.fh_algo_cdlp(self.h, ",".join(labels).encode(), ",".join(types).encode(), C.c_int64(max_iterations),
                                C.byref(nodes), C.byref(comm), C.byref(n)))
        return _take(nodes, n.value), _take(comm, n.value, np.int64)

    def algo_harmonic_centrality(self, labels=(), types=()):
        """CALL algo.HarmonicCentrality({nodeLabels, relationshipTypes}) YIELD node, score, reachable ->
        (nodes, scores float64, reachable int64).  Several labels select the union of their nodes; an unknown relationship type
        is an error (see fh_algo_harmonic_centrality)."""
        nodes = u64p()
        scores = C.POINTER(C.c_double)()
        reach = C.POINTER(C.c_int64)()
        n = C.c_uint64()
        _ck(self.L.fh_algo_harmonic_centrality(self.h, ",".join(labels).encode(), ",".join(types).encode(), C.byref(nodes),
                                               C.byref(scores), C.byref(reach), C.byref(n)))
        return _take(nodes, n.value), _take(scores, n.value, np.float64), _take(reach, n.value, np.int64)

    def algo_msf(self, labels=(), types=(), maximize=False, weights=None):
        """CALL algo.MSF({nodeLabels, relationshipTypes, weightAttribute, objective}) YIELD nodes, edges -> a list of
        (nodes uint64[], edges uint64[]) per tree, in ascending order of the trees' smallest node id.  weights: None = no
        weightAttribute, else a {relationship id: number} dict — a relationship that is missing from it has no attribute (see
        fh_algo_msf).  An unknown relationship type is an error."""
        ids = wts = None
        if weights is not None:
            ids, wts = _attr_arrays(weights)
        nt = C.c_uint64()
        noff, nodes, eoff, edges = u64p(), u64p(), u64p(), u64p()
        _ck(self.L.fh_algo_msf(self.h, ",".join(labels).encode(), ",".join(types).encode(), C.c_int(1 if maximize else 0),
                               ids.ctypes.data_as(u64p) if ids is not None else None,
                               wts.ctypes.data_as(C.POINTER(C.c_double)) if wts is not None else None,
                               C.c_uint64(len(ids) if ids is not None else 0), C.byref(nt), C.byref(noff), C.byref(nodes),
                               C.byref(eoff), C.byref(edges)))
        t = nt.value
        no, eo = _take(noff, t + 1), _take(eoff, t + 1)
        nv, ev = _take(nodes, int(no[-1])), _take(edges, int(eo[-1]))
        return [(nv[int(no[i]):int(no[i + 1])], ev[int(eo[i]):int(eo[i + 1])]) for i in range(t)]

    def pair_stats(self):
        """The eight stats of the last fgpu_pair_weights call algo_msf / algo_sp_paths / algo_sp_paths_rows made on this graph
        (fh_graph_pair_stats): [2] candidates and [3] pairs of the weight matrix the device built."""
        st = (C.c_uint64 * 8)()
        _ck(self.L.fh_graph_pair_stats(self.h, st))
        return [int(x) for x in st]

    def algo_maxflow(self, sources, targets, types, capacities=None, default_capacity=None, labels=(), attribute_exists=None):
        """CALL algo.maxFlow({sourceNodes, targetNodes, relationshipTypes, capacityProperty, defaultCapacity, nodeLabels})
        YIELD nodes, edges, edgeFlows, maxFlow -> (nodes uint64[], edges uint64[], flows float64[], max_flow).  capacities: a
        {relationship id: value} dict standing for the capacity attribute — a value that is no number (a string, a list) counts
        as missing, like an id that is not listed; attribute_exists: whether the graph knows the attribute name at all
        (default: capacities is not None).  See fh_algo_maxflow for the rules and the failures."""
        if attribute_exists is None:
            attribute_exists = capacities is not None
        num = {k: float(v) for k, v in (capacities or {}).items() if isinstance(v, (int, float)) and not isinstance(v, bool)}
        ids = np.ascontiguousarray(list(num.keys()), dtype=np.uint64)
        cps = np.ascontiguousarray(list(num.values()), dtype=np.float64)
        src = np.ascontiguousarray(list(sources), dtype=np.uint64)
        dst = np.ascontiguousarray(list(targets), dtype=np.uint64)
        nodes, edges = u64p(), u64p()
        flows = C.POINTER(C.c_double)()
        nn, ne = C.c_uint64(), C.c_uint64()
        val = C.c_double()
        _ck(self.L.fh_algo_maxflow(self.h, ",".join(labels).encode(), ",".join(types).encode(), src.ctypes.data_as(u64p),
                                   C.c_uint64(len(src)), dst.ctypes.data_as(u64p), C.c_uint64(len(dst)),
                                   C.c_int(1 if attribute_exists else 0), ids.ctypes.data_as(u64p),
                                   cps.ctypes.data_as(C.POINTER(C.c_double)), C.c_uint64(len(ids)),
                                   C.c_int(0 if default_capacity is None else 1),
                                   C.c_double(0.0 if default_capacity is None else float(default_capacity)), C.byref(nodes),
                                   C.byref(nn), C.byref(edges), C.byref(flows), C.byref(ne), C.byref(val)))
        return _take(nodes, nn.value), _take(edges, ne.value), _take(flows, ne.value, np.float64), val.value

    def algo_sp_paths(self, source, target, types=(), direction="outgoing", weights=None, costs=None):
        """CALL algo.SPpaths({sourceNode, targetNode, relTypes, relDirection, weightProp, costProp, pathCount: 1}) YIELD path,
        pathWeight, pathCost -> None when there is no path, else (nodes uint64[], edges uint64[], weight, cost).  Only the
        single-cheapest-path shape is served (no maxLen, no maxCost; see fh_algo_sp_paths).  weights / costs: None = no
        weightProp / costProp, else a {relationship id: number} dict — a relationship missing from it weighs 1.0 / costs 0.0.
        A negative weight is an error."""
        def attr(d):
            if d is None:
                return None, None, 0
            ids, vals = _attr_arrays(d)
            return ids.ctypes.data_as(u64p), vals.ctypes.data_as(C.POINTER(C.c_double)), len(ids), (ids, vals)
        w, c = attr(weights), attr(costs)
        found = C.c_int()
        nodes, edges = u64p(), u64p()
        nn = C.c_uint64()
        weight, cost = C.c_double(), C.c_double()
        _ck(self.L.fh_algo_sp_paths(self.h, C.c_uint64(source), C.c_uint64(target), ",".join(types).encode(),
                                    C.c_int({"outgoing": 0, "incoming": 1, "both": 2}[direction]), w[0], w[1], C.c_uint64(w[2]),
                                    c[0], c[1], C.c_uint64(c[2]), C.byref(found), C.byref(nodes), C.byref(nn), C.byref(edges),
                                    C.byref(weight), C.byref(cost)))
        nv = _take(nodes, nn.value)
        ev = _take(edges, max(nn.value, 1) - 1)
        if not found.value:
            return None
        return nv, ev, weight.value, cost.value

    def _path_rows(self, fn, head, types, direction, max_len, max_cost, path_count, weights, costs, tail, stats):
        def attr(d):
            if d is None:
                return None, None, 0
            ids, vals = _attr_arrays(d)
            return ids.ctypes.data_as(u64p), vals.ctypes.data_as(C.POINTER(C.c_double)), len(ids), (ids, vals)
        w, c = attr(weights), attr(costs)
        n = C.c_uint64()
        off, nodes, edges = u64p(), u64p(), u64p()
        pw, pc = C.POINTER(C.c_double)(), C.POINTER(C.c_double)()
        st = (C.c_int64 * 4)()
        _ck(fn(self.h, *head, ",".join(types).encode(), C.c_int({"outgoing": 0, "incoming": 1, "both": 2}[direction]),
               C.c_int64(-1 if max_len is None else max_len), C.c_int(0 if max_cost is None else 1),
               C.c_double(0.0 if max_cost is None else float(max_cost)), C.c_int64(path_count), w[0], w[1], C.c_uint64(w[2]),
               c[0], c[1], C.c_uint64(c[2]), *tail, C.byref(n), C.byref(off), C.byref(nodes), C.byref(edges), C.byref(pw),
               C.byref(pc), st))
        k = n.value
        o = _take(off, k + 1)
        total = int(o[-1])
        nv, ev = _take(nodes, total + k), _take(edges, total)
        ws, cs = _take(pw, k, np.float64), _take(pc, k, np.float64)
        rows = [(nv[int(o[r]) + r:int(o[r + 1]) + r + 1], ev[int(o[r]):int(o[r + 1])], float(ws[r]), float(cs[r])) for r in range(k)]
        if stats:
            return rows, {"examined": st[0], "pruned_hops": st[1], "pruned_weight": st[2], "table_rows": st[3]}
        return rows

    def algo_sp_paths_rows(self, source, target, types=(), direction="outgoing", max_len=None, max_cost=None, path_count=1,
                           weights=None, costs=None, prune=True, max_examined=0, stats=False):
        """CALL algo.SPpaths({sourceNode, targetNode, relTypes, relDirection, weightProp, costProp, maxLen, maxCost, pathCount})
        YIELD path, pathWeight, pathCost in every shape -> a list of (nodes uint64[], edges uint64[], weight, cost) in the
        procedure's order; with stats=True also the walk's counters (see fh_algo_sp_paths_rows).  max_len / max_cost None = not
        given; weights / costs as algo_sp_paths takes them; prune=False walks as the reference does, without the device's
        table; max_examined: a budget of examined successors, 0 = none."""
        return self._path_rows(self.L.fh_algo_sp_paths_rows, (C.c_uint64(source), C.c_uint64(target)), types, direction, max_len,
                               max_cost, path_count, weights, costs, (C.c_int(1 if prune else 0), C.c_uint64(max_examined)), stats)

    def algo_ss_paths(self, source, types=(), direction="outgoing", max_len=None, max_cost=None, path_count=1, weights=None,
                      costs=None, max_examined=0, stats=False):
        """CALL algo.SSpaths({sourceNode, relTypes, relDirection, weightProp, costProp, maxLen, maxCost, pathCount}) YIELD path,
        pathWeight, pathCost -> rows as algo_sp_paths_rows returns them (see fh_algo_ss_paths)."""
        return self._path_rows(self.L.fh_algo_ss_paths, (C.c_uint64(source),), types, direction, max_len, max_cost, path_count,
                               weights, costs, (C.c_uint64(max_examined),), stats)

    def algo_betweenness(self, labels=(), types=(), sampling_size=16, sampling_seed=0):
        """CALL algo.betweenness({nodeLabels, relationshipTypes, samplingSize, samplingSeed}) YIELD node, score ->
        (nodes, scores float64).  Several labels select the union of their nodes (see fh_algo_betweenness)."""
        nodes = u64p()
        scores = C.POINTER(C.c_double)()
        n = C.c_uint64()
        _ck(self.L.fh_algo_betweenness(self.h, ",".join(labels).encode(), ",".join(types).encode(), C.c_int64(sampling_size),
                                       C.c_int64(sampling_seed), C.byref(nodes), C.byref(scores), C.byref(n)))
        return _take(nodes, n.value), _take(scores, n.value, np.float64)

    # ---- vector indexes: db.idx.vector.queryNodes / queryRelationships (fh_graph_vector_*, fh_vector_query_*) ----
    def vector_index_create(self, is_edge, label_or_type_id, attr, dim, similarity=None):
        _ck(self.L.fh_graph_vector_index_create(self.h, 1 if is_edge else 0, C.c_uint64(label_or_type_id), attr.encode(),
                                                C.c_uint64(dim), similarity.encode() if similarity is not None else None))

    def vector_index_drop(self, is_edge, label_or_type_id, attr):
        return _ck(self.L.fh_graph_vector_index_drop(self.h, 1 if is_edge else 0, C.c_uint64(label_or_type_id), attr.encode()),
                   allow=(0, 1)) == 0

    def vector_set_node(self, label_id, attr, node, vec):
        v = _f32(vec)
        _ck(self.L.fh_graph_vector_set_node(self.h, C.c_uint64(label_id), attr.encode(), C.c_uint64(node), _pf(v),
                                            C.c_uint64(v.size)))

    def vector_set_edge(self, type_id, attr, src, dst, edge_id, vec):
        v = _f32(vec)
        _ck(self.L.fh_graph_vector_set_edge(self.h, C.c_uint64(type_id), attr.encode(), C.c_uint64(src), C.c_uint64(dst),
                                            C.c_uint64(edge_id), _pf(v), C.c_uint64(v.size)))

    def vector_unset_node(self, label_id, attr, node):
        return _ck(self.L.fh_graph_vector_unset_node(self.h, C.c_uint64(label_id), attr.encode(), C.c_uint64(node)),
                   allow=(0, 1)) == 0

    def vector_unset_edge(self, type_id, attr, edge_id):
        return _ck(self.L.fh_graph_vector_unset_edge(self.h, C.c_uint64(type_id), attr.encode(), C.c_uint64(edge_id)),
                   allow=(0, 1)) == 0

    def vector_query_nodes(self, label, attr, k, query):
        """CALL db.idx.vector.queryNodes(label, attr, k, query) YIELD node, score -> (nodes, scores float64), ascending."""
        q = _f32(query)
        ids, dist, n = u64p(), C.POINTER(C.c_double)(), C.c_uint64()
        _ck(self.L.fh_vector_query_nodes(self.h, label.encode(), attr.encode(), C.c_int64(k), _pf(q), C.c_uint64(q.size),
                                         C.byref(ids), C.byref(dist), C.byref(n)))
        return _take(ids, n.value), _take(dist, n.value, np.float64)

    def vector_query_edges(self, rel_type, attr, k, query):
        """CALL db.idx.vector.queryRelationships(type, attr, k, query) YIELD relationship, score ->
        (edge ids, scores float64, srcs, dsts), ascending."""
        q = _f32(query)
        ids, dist, srcs, dsts, n = u64p(), C.POINTER(C.c_double)(), u64p(), u64p(), C.c_uint64()
        _ck(self.L.fh_vector_query_edges(self.h, rel_type.encode(), attr.encode(), C.c_int64(k), _pf(q), C.c_uint64(q.size),
                                         C.byref(ids), C.byref(dist), C.byref(srcs), C.byref(dsts), C.byref(n)))
        return _take(ids, n.value), _take(dist, n.value, np.float64), _take(srcs, n.value), _take(dsts, n.value)

    def vector_query_nodes_batch(self, label, attr, k, queries):
        """queryNodes for every row of queries (nq, dim) in one device call -> (offsets uint64[nq + 1], nodes, scores)."""
        q = np.ascontiguousarray(queries, dtype=np.float32)
        assert q.ndim == 2
        nq, qn = q.shape
        off, ids, dist = u64p(), u64p(), C.POINTER(C.c_double)()
        _ck(self.L.fh_vector_query_nodes_batch(self.h, label.encode(), attr.encode(), C.c_int64(k), _pf(q), C.c_uint64(qn),
                                               C.c_uint64(nq), C.byref(off), C.byref(ids), C.byref(dist)))
        offsets = _take(off, nq + 1)
        total = int(offsets[-1])
        return offsets, _take(ids, total), _take(dist, total, np.float64)

    vec_distance = staticmethod(vec_distance)

    def algo_bfs(self, source, max_depth=-1, rel_type=None, want_edges=False):
        has = C.c_int()
        nodes, edges = u64p(), u64p()
        nn, ne = C.c_uint64(), C.c_uint64()
        _ck(self.L.fh_algo_bfs(self.h, C.c_int64(-1 if source is None else source), C.c_int64(max_depth),
                               rel_type.encode() if rel_type is not None else None, 1 if want_edges else 0,
                               C.byref(has), C.byref(nodes), C.byref(nn), C.byref(edges), C.byref(ne)))
        nv, ev = _take(nodes, nn.value).tolist(), _take(edges, ne.value).tolist()
        return (nv, ev) if has.value else None


class Tensor:
    """A Tensor on its own (tensor.rs:184-989), as the reference's unit tests drive it (fh_tn_*)."""
    MULTI_EDGE = 2 ** 64 - 1

    def __init__(self, ctx, nrows=None, ncols=None, _h=None):
        self.ctx, self.L = ctx, ctx.L
        self.h = _h if _h is not None else C.c_void_p()
        if _h is None:
            _ck(self.L.fh_tn_new(ctx.h, C.byref(self.h), C.c_uint64(nrows), C.c_uint64(ncols)))

    def __del__(self):
        try:
            if self.h and self.ctx.h:      # a tensor that outlives its context has nothing left to free
                self.L.fh_tn_free(self.h)
            self.h = C.c_void_p()
        except Exception:
            pass

    def dup(self):
        h = C.c_void_p()
        _ck(self.L.fh_tn_dup(self.h, C.byref(h)))
        return Tensor(self.ctx, _h=h)

    def set_all_from_slices(self, srcs, dsts, ids):
        s, d, i = _u64(srcs), _u64(dsts), _u64(ids)
        _ck(self.L.fh_tn_set_all(self.h, _p(s), _p(d), _p(i), C.c_uint64(len(s))))

    def remove_all(self, rels):
        """rels = [(edge id, src, dst)]; returns the emptied (src, dst) pairs."""
        flat = _u64(np.asarray(list(rels), dtype=np.uint64).reshape(-1))
        es, ed, n = u64p(), u64p(), C.c_uint64()
        _ck(self.L.fh_tn_remove_all(self.h, _p(flat), C.c_uint64(len(flat) // 3), C.byref(es), C.byref(ed), C.byref(n)))
        return list(zip(_take(es, n.value).tolist(), _take(ed, n.value).tolist()))

    def flush(self): _ck(self.L.fh_tn_op(self.h, 0, C.c_uint64(0), C.c_uint64(0)))
    def fold_oversized(self): _ck(self.L.fh_tn_op(self.h, 1, C.c_uint64(0), C.c_uint64(0)))
    def wait(self): _ck(self.L.fh_tn_op(self.h, 2, C.c_uint64(0), C.c_uint64(0)))
    def wait_fwd(self): _ck(self.L.fh_tn_op(self.h, 3, C.c_uint64(0), C.c_uint64(0)))
    def resize(self, nrows, ncols): _ck(self.L.fh_tn_op(self.h, 4, C.c_uint64(nrows), C.c_uint64(ncols)))

    def get(self, src, dst):
        ids, n = u64p(), C.c_uint64()
        _ck(self.L.fh_tn_get(self.h, C.c_uint64(src), C.c_uint64(dst), C.byref(ids), C.byref(n)))
        return _take(ids, n.value).tolist()

    def _probe(self, which, src, dst):
        v = C.c_uint64()
        code = self.L.fh_tn_probe(self.h, which, C.c_uint64(src), C.c_uint64(dst), C.byref(v))
        _ck(code, allow=(0, 1))
        return v.value if code == 0 else None

    def eff_get(self, src, dst): return self._probe(0, src, dst)
    def m_get(self, src, dst): return self._probe(1, src, dst)
    def extract_contains(self, src, dst): return self._probe(2, src, dst) is not None

    def encode(self) -> bytes:
        b, n = C.POINTER(C.c_uint8)(), C.c_uint64()
        _ck(self.L.fh_tn_encode(self.h, C.byref(b), C.byref(n)))
        out = bytes(C.cast(b, C.POINTER(C.c_uint8 * max(n.value, 1))).contents)[:n.value]
        self.L.fh_free(b)
        return out

    @staticmethod
    def decode(ctx, payload: bytes):
        buf = (C.c_uint8 * len(payload)).from_buffer_copy(payload)
        h, used = C.c_void_p(), C.c_uint64()
        _ck(ctx.L.fh_tn_decode(ctx.h, buf, C.c_uint64(len(payload)), C.byref(h), C.byref(used)))
        return Tensor(ctx, _h=h), used.value

    def state(self):
        out = (C.c_uint64 * 8)()
        _ck(self.L.fh_tn_state(self.h, out))
        return dict(zip(("m", "dp", "dm", "multi_pairs", "mt", "me_nvals", "edge_count", "m_pending"), [int(x) for x in out]))


def algo_bfs_multi(graph, gang, source, max_depth=-1, rel_type=None, want_edges=False):
    """algo.BFS partitioned over the contexts of `gang` (host.Context objects, gang[0] = the graph's own)."""
    has = C.c_int()
    nodes, edges = u64p(), u64p()
    nn, ne = C.c_uint64(), C.c_uint64()
    arr = (C.c_void_p * len(gang))(*[c.h for c in gang])
    _ck(graph.L.fh_algo_bfs_multi(graph.h, arr, len(gang), C.c_int64(-1 if source is None else source),
                                  C.c_int64(max_depth), rel_type.encode() if rel_type is not None else None,
                                  1 if want_edges else 0, C.byref(has), C.byref(nodes), C.byref(nn), C.byref(edges),
                                  C.byref(ne)))
    nv, ev = _take(nodes, nn.value).tolist(), _take(edges, ne.value).tolist()
    return (nv, ev) if has.value else None


# ---- v19 matrix payload (Encode<19> / Decode<19> for Matrix<T>) ---------------------------------------------
def container_parse(payload: bytes):
    """CPU-only: {nrows, ncols, nvals, hyper, valued, consumed, p, h, i, x} of a container payload."""
    L = load()
    buf = (C.c_uint8 * len(payload)).from_buffer_copy(payload)
    dims = (C.c_uint64 * 6)()
    p, h, i, x = u64p(), u64p(), u64p(), u64p()
    np_, nh = C.c_uint64(), C.c_uint64()
    _ck(L.fh_container_parse(buf, C.c_uint64(len(payload)), dims, C.byref(p), C.byref(np_), C.byref(h), C.byref(nh),
                             C.byref(i), C.byref(x)))
    nvals, valued = dims[2], bool(dims[4])
    return {"nrows": dims[0], "ncols": dims[1], "nvals": nvals, "hyper": bool(dims[3]), "valued": valued,
            "consumed": dims[5], "p": _take(p, np_.value), "h": _take(h, nh.value), "i": _take(i, nvals),
            "x": _take(x, nvals if valued else 0)}


def matrix_decode(ctx, payload: bytes):
    """Decode<19> for Matrix<T>: payload -> Matrix (arrays go to the device as they are)."""
    buf = (C.c_uint8 * len(payload)).from_buffer_copy(payload)
    h = C.c_void_p()
    used = C.c_uint64()
    _ck(ctx.L.fh_mat_decode(ctx.h, buf, C.c_uint64(len(payload)), C.byref(h), C.byref(used)))
    return Matrix(ctx, _h=h), used.value


def matrix_encode(m) -> bytes:
    """Encode<19> for Matrix<T>."""
    out = C.POINTER(C.c_uint8)()
    n = C.c_uint64()
    _ck(m.L.fh_mat_encode(m.h, C.byref(out), C.byref(n)))
    data = bytes(out[:n.value])
    m.L.fh_free(C.cast(out, C.c_void_p))
    return data


# ---- planner slice (fuse_anonymous_traverse) -------------------------------------------------------------
def _node_txt(n):
    return n["alias"] + "".join(":" + l for l in n.get("labels", [])) + ("*" if n.get("attrs") else "")


def _rel_txt(r):
    flags = ("b" if r.get("bidirectional") else "") + ("v" if r.get("var_len") else "") + ("a" if r.get("attrs") else "")
    return "|".join([r["alias"], _node_txt(r["from"]), _node_txt(r["to"]), ",".join(r.get("types", [])), flags])


def plan_to_text(ops):
    """ops: list of dicts {id, parent, kind: "CT" | "X", ...} (see tests/test_host_cpu.py); children keep list order."""
    lines = []
    for op in ops:
        if op["kind"] == "X":
            lines.append(f"X {op['id']} {op['parent']} {op.get('name', 'Op')} refs={','.join(op.get('refs', []))}")
        else:
            flags = ("e" if op.get("emit") else "") + ("t" if op.get("transposed") else "") + \
                    ("o" if op.get("optional") else "") + ("" if op.get("bind", True) else "n")
            lines.append(f"CT {op['id']} {op['parent']} rel={_rel_txt(op['rel'])} flags={flags} "
                         f"sib={','.join(op.get('siblings', []))} chain={';'.join(_rel_txt(r) for r in op.get('chain', []))}")
    return "\n".join(lines) + "\n"


def _node_from(txt):
    attrs = txt.endswith("*")
    parts = txt.rstrip("*").split(":")
    return {"alias": parts[0], "labels": [p for p in parts[1:] if p], "attrs": attrs}


def _rel_from(txt):
    f = (txt.split("|") + [""] * 5)[:5]
    return {"alias": f[0], "from": _node_from(f[1]), "to": _node_from(f[2]), "types": [t for t in f[3].split(",") if t],
            "bidirectional": "b" in f[4], "var_len": "v" in f[4], "attrs": "a" in f[4]}


def plan_from_text(text):
    ops = []
    for line in text.splitlines():
        tok = line.split()
        if not tok:
            continue
        kv = dict(t.split("=", 1) for t in tok[3:] if "=" in t)
        if tok[0] == "X":
            ops.append({"id": int(tok[1]), "parent": int(tok[2]), "kind": "X", "name": tok[3],
                        "refs": [a for a in kv.get("refs", "").split(",") if a]})
        else:
            fl = kv.get("flags", "")
            ops.append({"id": int(tok[1]), "parent": int(tok[2]), "kind": "CT", "rel": _rel_from(kv["rel"]),
                        "emit": "e" in fl, "transposed": "t" in fl, "optional": "o" in fl, "bind": "n" not in fl,
                        "siblings": [a for a in kv.get("sib", "").split(",") if a],
                        "chain": [_rel_from(r) for r in kv.get("chain", "").split(";") if r]})
    return ops


def plan_fuse(ops, lower_id=-1):
    """fuse_anonymous_traverse on a plan (list of op dicts); returns (ops after the pass, runtime spec of CondTraverse
    node `lower_id` as bytes for Graph.cond_traverse_batch, or None)."""
    L = load()
    out, spec = C.c_char_p(), C.c_char_p()
    L.fh_plan_fuse.argtypes = [C.c_char_p, C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_char_p)]
    _ck(L.fh_plan_fuse(plan_to_text(ops).encode(), lower_id, C.byref(out), C.byref(spec)))
    text, sp = out.value.decode(), spec.value
    return plan_from_text(text), (sp if lower_id >= 0 else None)
