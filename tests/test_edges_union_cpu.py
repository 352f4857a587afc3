"""tests/edges_union_check.py pinned on expectations written out by hand from tensor.rs:383-418, and held against an
edge-by-edge replay of tensor.rs:360-446 on a folded tensor — the checker of fgpu_edges_union and Graph::append_edges_bulk must
not be whatever the device code happens to compute.  No GPU."""
import os
import random
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from edges_union_check import MULTI, build_edges, union_edges  # noqa: E402

# the 6 x 6 tensor of tests/test_edges_remove_cpu.py: (0, 1), (5, 5) and (3, 2) single, (2, 3) with three edges, (4, 0) and the
# self-loop pair (1, 1) with two
PAIRS = {(0, 1): 10, (2, 3): MULTI, (4, 0): MULTI, (5, 5): 77, (1, 1): MULTI, (3, 2): 31}
ROWS = {(2, 3): [20, 21, 25], (4, 0): [40, 44], (1, 1): [11, 12]}


def run(bpairs, brows=None, pairs=PAIRS, rows=ROWS):
    return union_edges(pairs, rows, bpairs, brows or {})


def test_single_plus_single_promotes():
    """:392-398 — the stored id and the new one go to the row, the entry becomes MULTI_EDGE."""
    merged, out, st = run({(0, 1): 9})
    assert merged == {**PAIRS, (0, 1): MULTI} and out == {(0, 1): [9, 10]}
    #            new collide promoted extended ids longest m_out mt_out
    assert st == [0, 1, 1, 0, 2, 2, 6, 6]


def test_single_plus_run():
    """:392-398 for the batch's first edge on the pair, :368-378 for its others."""
    merged, out, st = run({(5, 5): MULTI}, {(5, 5): [70, 78, 90]})
    assert merged == {**PAIRS, (5, 5): MULTI} and out == {(5, 5): [70, 77, 78, 90]}
    assert st == [0, 1, 1, 0, 4, 4, 6, 6]


def test_run_plus_single():
    """:385-388 — the id joins the row."""
    merged, out, st = run({(2, 3): 22})
    assert merged == PAIRS and out == {(2, 3): [20, 21, 22, 25]}
    assert st == [0, 1, 0, 1, 4, 4, 6, 6]


def test_run_plus_run():
    merged, out, st = run({(4, 0): MULTI}, {(4, 0): [1, 41, 100]})
    assert merged == PAIRS and out == {(4, 0): [1, 40, 41, 44, 100]}
    assert st == [0, 1, 0, 1, 5, 5, 6, 6]


def test_a_new_single_pair_and_a_new_multi_pair():
    """:411-417 — inline; a second edge of the batch on it promotes the pending slot (:370-376).  Neither has an out row: the
    caller holds the batch's row."""
    merged, out, st = run({(0, 0): 5, (3, 3): MULTI}, {(3, 3): [6, 7]})
    assert merged == {**PAIRS, (0, 0): 5, (3, 3): MULTI} and out == {}
    assert st == [2, 0, 0, 0, 0, 0, 8, 8]


def test_an_untouched_pair_keeps_its_value():
    merged, out, st = run({(0, 1): 9, (0, 2): 8})
    assert {k: merged[k] for k in PAIRS if k != (0, 1)} == {k: v for k, v in PAIRS.items() if k != (0, 1)}
    assert merged[(0, 2)] == 8 and st == [1, 1, 1, 0, 2, 2, 7, 7]


def test_the_empty_batch():
    merged, out, st = run({})
    assert merged == PAIRS and out == {} and st == [0, 0, 0, 0, 0, 0, 6, 6]


def test_the_whole_contract_on_6_by_6():
    bpairs = {(0, 1): 9, (5, 5): MULTI, (2, 3): 22, (4, 0): MULTI, (0, 0): 5, (3, 3): MULTI}
    brows = {(5, 5): [70, 78], (4, 0): [41, 100], (3, 3): [6, 7]}
    merged, out, st = run(bpairs, brows)
    assert merged == {(0, 0): 5, (0, 1): MULTI, (1, 1): MULTI, (2, 3): MULTI, (3, 2): 31, (3, 3): MULTI, (4, 0): MULTI, (5, 5): MULTI}
    assert out == {(0, 1): [9, 10], (2, 3): [20, 21, 22, 25], (4, 0): [40, 41, 44, 100], (5, 5): [70, 77, 78]}
    assert st == [2, 4, 2, 2, 13, 4, 8, 8]


def test_ignored_keys():
    """An a row of a pair that is not MULTI in m, an a row of a pair the batch does not name (even one m does not hold), and a b
    row of a pair that is not MULTI in fwd change nothing."""
    rows = {**ROWS, (0, 1): [1, 2], (3, 5): [3, 4]}
    merged, out, st = union_edges(PAIRS, rows, {(0, 1): 9, (2, 3): 22}, {(0, 1): [5, 6], (2, 3): [7, 8], (4, 4): [1, 2]})
    assert merged == {**PAIRS, (0, 1): MULTI} and out == {(0, 1): [9, 10], (2, 3): [20, 21, 22, 25]}
    assert st == [0, 2, 1, 1, 6, 4, 6, 6]
    # ... and a MULTI pair of m the batch does not name needs no row
    merged, out, st = union_edges(PAIRS, {}, {(0, 1): 9}, {})
    assert out == {(0, 1): [9, 10]}


def test_a_missing_row_is_an_error():
    with pytest.raises(ValueError):
        union_edges(PAIRS, {k: v for k, v in ROWS.items() if k != (2, 3)}, {(2, 3): 22}, {})      # no a row
    with pytest.raises(ValueError):
        run({(0, 1): MULTI}, {})                                                                  # no b row
    union_edges(PAIRS, ROWS, {(3, 3): MULTI}, {})         # (a new pair: its row is the caller's, the call never reads it)


@pytest.mark.parametrize("bpairs, brows", [({(0, 1): 10}, {}), ({(0, 1): MULTI}, {(0, 1): [3, 10]}), ({(2, 3): 21}, {}),
                                           ({(2, 3): MULTI}, {(2, 3): [19, 25, 26]})],
                         ids=["inline=inline", "inline-in-b-run", "a-run-id=inline", "run-and-run"])
def test_an_id_on_both_sides_is_an_error(bpairs, brows):
    """The edge is already stored: the reference's ids are unique, and set_all_from_slices would leave a MULTI_EDGE pair with a
    one-id row (me.set of a set id is a no-op)."""
    with pytest.raises(ValueError):
        run(bpairs, brows)


def test_build_edges():
    pairs, rows = build_edges([(2, 3, 9), (0, 1, 5), (2, 3, 4), (2, 3, 6), (1, 1, 2)])
    assert pairs == {(2, 3): MULTI, (0, 1): 5, (1, 1): 2} and rows == {(2, 3): [4, 6, 9]}


def replay(m, me, batch):
    """tensor.rs:360-446 on a folded tensor (dp and dm empty, so `masked` is false, `from_dp` None and cur = m.get): the read
    phase edge by edge, then the write phase's dp entries folded into m.  m: {(s, d): value}, me: {(s, d): set of ids}; both are
    changed in place."""
    pending = {}                                   # pair -> index into w, or None once the pair is known multi-edge
    w = []
    for s, d, i in batch:
        key = (s, d)
        if key in pending:                         # :368-378
            idx = pending[key]
            if idx is not None:
                me.setdefault(key, set()).add(w[idx][1])
                w[idx][1] = MULTI
                pending[key] = None
            me.setdefault(key, set()).add(i)
            continue
        cur = m.get(key)
        if cur == MULTI:                           # :385-388
            me.setdefault(key, set()).add(i)
            pending[key] = None
        elif cur is not None:                      # :392-409
            me.setdefault(key, set()).update((cur, i))
            pending[key] = None
            w.append([key, MULTI])
        else:                                      # :411-417
            pending[key] = len(w)
            w.append([key, i])
    for key, v in w:                               # :428-446, folded
        m[key] = v


def multigraph_edges(rng, n, count, first_id):
    """`count` edges with distinct ascending ids over a small n x n space, so that pairs repeat"""
    return [(rng.randrange(n), rng.randrange(n), first_id + 3 * k) for k in range(count)]


@pytest.mark.parametrize("seed", range(8))
def test_agreement_with_the_edge_by_edge_replay(seed):
    rng = random.Random(seed)
    n = 12 + seed
    loaded = multigraph_edges(rng, n, 150 + 20 * seed, 1000)
    batch = multigraph_edges(rng, n, 120 + 30 * seed, 50_000)
    rng.shuffle(batch)                             # ids arrive in any order
    pairs, rows = build_edges(loaded)
    bpairs, brows = build_edges(batch)
    merged, out, st = union_edges(pairs, rows, bpairs, brows)
    m, me = dict(pairs), {k: set(v) for k, v in rows.items()}
    replay(m, me, batch)
    assert merged == m
    # every pair's ids: inline, the out row of a colliding pair, the batch's row of a new multi-edge pair, or m's own row
    ids = {k: (out[k] if k in out else brows[k] if k in brows and k not in pairs else rows[k]) if v == MULTI else [v]
           for k, v in merged.items()}
    assert ids == {k: sorted(me[k]) if v == MULTI else [v] for k, v in m.items()}
    assert sum(1 for v in merged.values() if v == MULTI) == len(me)
    assert st[1] == len(set(pairs) & set(bpairs)) > 0 and st[2] > 0 and st[3] > 0 and st[0] > 0
    assert st[4] == sum(len(v) for v in out.values()) and st[6] == len(m)
