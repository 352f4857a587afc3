"""CPU: the numpy statement of fgpu_expand_exists' contract (tests/exists_check.py) on hand-built cases, against
oracle.delta_lmxm — the row-level mask above all — and its decision rule (sure / undecided) against that contract."""
import os
import sys

import numpy as np
import pytest

import oracle

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import chain_graph as cg  # noqa: E402
import exists_check as ec  # noqa: E402

U64 = np.uint64


@pytest.mark.parametrize("name", list(ec.mask_cases()))
def test_mask_cases_by_hand(name):
    src, layers, label, want, undecided = ec.mask_cases()[name]
    got = ec.expected(src, layers, ec.MASK_N, label)
    assert np.array_equal(got, want), (name, got)
    # the same rows from oracle.delta_lmxm called here, hop by hop
    valid = src != ec.SKIP
    f = oracle.build_csr(len(src), ec.MASK_N, np.arange(len(src), dtype=U64)[valid], src[valid])
    for m, dp, dm in layers:
        f, _ = oracle.delta_lmxm(f, m, dp, dm)
    rows, cols = f.pairs()
    if label is not None:
        rows = rows[np.isin(cols, label)]
    byhand = np.zeros(len(src), dtype=bool)
    byhand[rows.astype(np.int64)] = True
    assert np.array_equal(byhand, want)
    sure, und = ec.decide(src, layers, ec.MASK_N, label)
    assert np.array_equal(und, undecided), (name, und)
    assert not (sure & ~want).any() and not (want & ~sure & ~und).any()


def test_the_per_edge_rule_differs_on_the_masked_case():
    """(m \\ dm) U dp entry by entry keeps (u1, v): that rule would call row 0 a match."""
    src, layers, _, want, _ = ec.mask_cases()["masked"]
    m, dp, dm = layers[-1]
    per_edge = oracle.merge(m, dp, dm)
    f = cg.reference(src, layers[:-1], ec.MASK_N)[0]
    naive = ec.rows_nonempty(oracle.mxm(f, per_edge)[0])
    assert naive[0] and not want[0]


@pytest.mark.parametrize("cell", ["7 probe, push at 1", "7 probe, small, compacted, push at 1"])
@pytest.mark.parametrize("label", [False, True])
def test_decision_rule_is_sound_on_the_chain_graphs(cell, label):
    g = cg.check(cell)
    lab = cg.label_ids(g.n) if label else None
    want = ec.expected(g.src, g.layers(3), g.n, lab)
    sure, und = ec.decide(g.src, g.layers(3), g.n, lab)
    assert np.array_equal(want, ec.rows_nonempty(g.ref(3, label=label)[0]))
    assert not (sure & ~want).any() and not (want & ~sure & ~und).any()
    assert want.any() and (~want).any()


def test_row_lengths():
    src, layers, _, _, _ = ec.mask_cases()["one hop"]
    assert ec.row_lengths(src, layers[0], ec.MASK_N) == 1 + 1 + 0 + 1      # m rows of u1 and u2, no dp, the dm row of u2
