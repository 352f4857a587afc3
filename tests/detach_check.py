"""Plain-Python restatement of the reference's cascade delete, the checker of fgpu_nodes_detach and Graph::delete_nodes_bulk
(tests/test_gpu_nodes_detach.py, tests/test_gpu_delete_nodes_bulk_host.py; pinned by tests/test_detach_cpu.py).

graph.rs:2386-2494 (delete_implicit_edges): per relationship type, per deleted node ASCENDING (a RoaringTreemap iterates in
order, :2405), first the node's outgoing edges — Tensor::iter(node, node, false), ascending dst, the ids of one pair ascending —
(:2407-2413), then its incoming edges — Tensor::iter(node, node, true), ascending src — unless the source is the node itself or
is deleted too (:2417-2426: those were collected from the source's outgoing walk).  An id in explicit_rels is never listed
(:2410, :2422).  graph.rs:1753-1768 (delete_nodes): the deleted nodes' rows leave the node x label matrix.

Everything here is dicts, sets and sorted(); it shares nothing with the device code."""

MULTI = 2**64 - 1


def implicit_edges(edges, deleted, skip_ids=()):
    """edges: iterable of (src, dst, id) of ONE type.  The (id, src, dst) list of graph.rs:2402-2427 for that type."""
    deleted, skip = set(map(int, deleted)), set(map(int, skip_ids))
    out_of, in_of = {}, {}
    for s, d, i in edges:
        out_of.setdefault(int(s), []).append((int(d), int(i)))
        in_of.setdefault(int(d), []).append((int(s), int(i)))
    rels = []
    for node in sorted(deleted):                                         # :2405
        for d, i in sorted(out_of.get(node, [])):                        # :2407-2413
            if i not in skip:
                rels.append((i, node, d))
        for s, i in sorted(in_of.get(node, [])):                         # :2417-2426
            if s != node and s not in deleted and i not in skip:
                rels.append((i, s, node))
    return rels


def delete_nodes(edges_by_type, deleted, skip_ids=(), labels=()):
    """edges_by_type: one (src, dst, id) list per type id; labels: (node, label) pairs.  Returns a dict:
    list       the concatenation over types, ascending type id, of implicit_edges (:2401)
    edges      per type, the sorted edges left once the explicit deletes of skip_ids have run too: neither end deleted
    labels     the sorted label pairs left (:1753-1768)
    adjacency  the pairs some surviving edge connects — the edge-by-edge result
    adjacency_reference  the same plus the (deleted, deleted) pairs, which the reference leaves behind (:2381-2383)"""
    deleted = set(map(int, deleted))
    alive = lambda s, d: int(s) not in deleted and int(d) not in deleted
    lst, left = [], []
    for edges in edges_by_type:
        lst += implicit_edges(edges, deleted, skip_ids)
        left.append(sorted((int(s), int(d), int(i)) for s, d, i in edges if alive(s, d)))
    adj = {(s, d) for es in left for s, d, _ in es}
    both = {(int(s), int(d)) for es in edges_by_type for s, d, _ in es if int(s) in deleted and int(d) in deleted}
    return dict(list=lst, edges=left, labels=sorted((int(n), int(l)) for n, l in labels if int(n) not in deleted),
                adjacency=adj, adjacency_reference=adj | both)


def detach_matrix(entries, nodes, sides):
    """The contract of fgpu_nodes_detach on one matrix.  entries: {(row, col): value}.  Returns (kept, out_list, in_list, stats):
    kept the surviving {(row, col): value}; out_list the (row, col, value) with the row in D (sides bit 0) in ascending (row,
    col); in_list those with the column in D (bit 1) that are not out entries, in ascending (col, row); stats = [distinct
    nodes, out entries, in entries, removed MULTI values, kept, kept] as the call's stats[0..5] with a list and a transpose."""
    D = set(map(int, nodes))
    rows, cols = bool(sides & 1), bool(sides & 2)
    is_out = lambda r, c: rows and r in D
    is_in = lambda r, c: cols and c in D and not is_out(r, c)
    kept = {k: v for k, v in entries.items() if not is_out(*k) and not is_in(*k)}
    out_list = [(r, c, entries[(r, c)]) for r, c in sorted(entries) if is_out(r, c)]
    in_list = [(r, c, entries[(r, c)]) for c, r in sorted((c, r) for r, c in entries if is_in(r, c))]
    multi = sum(1 for _, _, v in out_list + in_list if v == MULTI)
    return kept, out_list, in_list, [len(D), len(out_list), len(in_list), multi, len(kept), len(kept)]
