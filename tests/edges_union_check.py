"""Plain-Python restatement of the reference's bulk edge insert onto a loaded tensor, the checker of fgpu_edges_union and
Graph::append_edges_bulk (tests/test_gpu_edges_union.py, tests/test_gpu_append_edges_bulk_host.py; pinned by
tests/test_edges_union_cpu.py).

tensor.rs:383-418 (Tensor::set_all_from_slices, the read phase's three arms): the first edge of a batch on a pair reads the
pair's state.  Absent: the id goes inline.  A single edge: the pair is promoted — the stored id and the new one go to the me row
and the entry becomes MULTI_EDGE.  MULTI_EDGE: the id joins the me row.  Every later edge of the batch on the pair joins the row
(:368-378).  Per pair that is a union: a pair only the batch names holds what the batch alone would build; a pair both sides
name holds MULTI_EDGE and the ascending merge of both id lists.  Edge ids are unique in the reference, so an id the pair already
stores is refused here rather than merged into a short row.

Everything here is dicts and sorted(); it shares nothing with the device code."""

MULTI = 2**64 - 1


def _side(name, pairs, rows, key):
    v = pairs[key]
    if v != MULTI:
        return [v]
    if key not in rows:
        raise ValueError(f"no {name} row supplied for {key}")
    return list(rows[key])


def union_edges(pairs, rows, bpairs, brows):
    """The contract of fgpu_edges_union on one tensor.  pairs / bpairs: {(src, dst): inline id or MULTI} of the tensor and of the
    batch; rows / brows: {(src, dst): ascending ids}, the supplied multi-edge rows of either (a row whose pair is not MULTI on its
    side, or an `a` row of a pair the batch does not name, is ignored).  Returns (merged, out_rows, stats): merged the
    {(src, dst): value} of m_out, out_rows {(src, dst): ascending ids} for the colliding pairs only, stats the call's eight
    counters.  A colliding pair that is MULTI on a side without that side's row, and an id on both sides of a colliding pair,
    raise ValueError."""
    merged = dict(pairs)
    out_rows = {}
    new = promoted = extended = 0
    for key in sorted(bpairs):
        if key not in pairs:
            merged[key] = bpairs[key]
            new += 1
            continue
        a, b = _side("a", pairs, rows, key), _side("b", bpairs, brows, key)
        both = sorted(set(a) & set(b))
        if both:
            raise ValueError(f"id {both[0]} is on both sides of {key}")
        if pairs[key] == MULTI:
            extended += 1
        else:
            promoted += 1
        merged[key] = MULTI
        out_rows[key] = sorted(a + b)
    ids = sum(len(r) for r in out_rows.values())
    longest = max((len(r) for r in out_rows.values()), default=0)
    return merged, out_rows, [new, len(out_rows), promoted, extended, ids, longest, len(merged), len(merged)]


def build_edges(edges):
    """What fgpu_edges_build holds for a list of (src, dst, id): ({(src, dst): inline id or MULTI}, {(src, dst): ascending ids})."""
    by = {}
    for s, d, i in edges:
        by.setdefault((int(s), int(d)), []).append(int(i))
    pairs = {k: (v[0] if len(v) == 1 else MULTI) for k, v in by.items()}
    return pairs, {k: sorted(v) for k, v in by.items() if len(v) > 1}
