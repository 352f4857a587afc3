"""Plain-Python restatement of the reference's explicit edge delete, the checker of fgpu_edges_remove and Graph::delete_edges_bulk
(tests/test_gpu_edges_remove.py, tests/test_gpu_delete_edges_bulk_host.py; pinned by tests/test_edges_remove_cpu.py).

tensor.rs:497-629 (Tensor::remove_all, slow path): per touched pair the effective state is read once (:523-543), then every
(id, src, dst) of the batch replays its transition — on a multi-edge pair the id leaves the me row if it is there (:545-552), and a
row left with ONE id demotes: the survivor returns inline, where a later triple of the batch can name it (:563-575); on a
single-edge pair the pair is emptied when the inline id is the named one (:579-582); anything else is skipped (:583-584).  Every
transition applies only where the id is there, so the batch is a SET of removals: its order does not matter and a repeated triple
counts once (here its hit flag is 1 each time; the reference keeps no such flag).  graph.rs:2303-2372 (delete_relationships): the
ids are grouped by type, each group goes through remove_all, and the pairs no tensor holds any more leave the adjacency.

Everything here is dicts, sets and sorted(); it shares nothing with the device code."""

MULTI = 2**64 - 1


def remove_edges(pairs, me_rows, triples):
    """The contract of fgpu_edges_remove on one tensor.  pairs: {(src, dst): inline id or MULTI}; me_rows: {(src, dst): ascending
    ids} — the supplied multi-edge rows (a row whose pair is not MULTI in `pairs` is ignored); triples: (src, dst, id) in batch
    order.  Returns (kept, hit, taken, emptied, stats): kept the {(src, dst): value} left, a demoted pair with its surviving id
    inline; hit one 0 / 1 per triple; taken one 0 / 1 per supplied id, the rows in ascending (src, dst); emptied the sorted pairs
    that left; stats the call's eight counters.  A triple on a MULTI pair without a supplied row raises ValueError."""
    gone = {}                                                            # pair -> set of ids that leave it
    hit, absent, unknown = [], 0, 0
    for s, d, i in triples:
        s, d, i = int(s), int(d), int(i)
        if (s, d) not in pairs:
            absent += 1
            hit.append(0)
            continue
        v = pairs[(s, d)]
        if v == MULTI:
            if (s, d) not in me_rows:
                raise ValueError(f"no multi-edge row supplied for ({s}, {d})")
            here = i in me_rows[(s, d)]
        else:
            here = v == i
        if here:
            gone.setdefault((s, d), set()).add(i)
        else:
            unknown += 1
        hit.append(1 if here else 0)
    kept, emptied, emptied_multi, demoted = dict(pairs), [], 0, 0
    for (s, d), ids in gone.items():
        if pairs[(s, d)] != MULTI:
            del kept[(s, d)]
            emptied.append((s, d))
            continue
        left = [x for x in me_rows[(s, d)] if x not in ids]
        if len(left) == 0:
            del kept[(s, d)]
            emptied.append((s, d))
            emptied_multi += 1
        elif len(left) == 1:
            kept[(s, d)] = left[0]
            demoted += 1
    taken = [1 if x in gone.get(k, ()) and pairs.get(k) == MULTI else 0 for k in sorted(me_rows) for x in me_rows[k]]
    return kept, hit, taken, sorted(emptied), [sum(hit), len(emptied), emptied_multi, demoted, len(kept), len(kept), absent, unknown]


def delete_edges(edges_by_type, batch):
    """edges_by_type: one (src, dst, id) list per type id; batch: (type, src, dst, id) in input order.  Returns a dict:
    list       the removed (id, src, dst): types ascending, input order within a type, stored edges only, a repeated one once
    edges      per type, the sorted edges left
    adjacency  the pairs some surviving edge connects"""
    have = [set((int(s), int(d), int(i)) for s, d, i in es) for es in edges_by_type]
    lst = []
    for t in range(len(edges_by_type)):
        seen = set()
        for tt, s, d, i in batch:
            e = (int(s), int(d), int(i))
            if int(tt) == t and e in have[t] and e not in seen:
                seen.add(e)
                lst.append((e[2], e[0], e[1]))
        have[t] -= seen
    left = [sorted(h) for h in have]
    return dict(list=lst, edges=left, adjacency={(s, d) for es in left for s, d, _ in es})
