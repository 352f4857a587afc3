"""The constructed graphs of tests/chain_graph.py without a device: every graph's shape checks (T_h, |F_h|, n, nnz, the rows
that are empty after each hop, their placement) run on construction, and every cell's path is re-derived from the host graph
inequality by inequality (Graph.check_cell)."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import chain_graph as cg  # noqa: E402


@pytest.mark.parametrize("name", sorted(cg.SPECS))
def test_graph_holds_what_it_says(name):
    g = cg.graph(name)
    fig = g.figures()
    print(name, fig)
    assert g.as_built() == cg.FIGURES[name]
    assert 3000 <= g.n <= 20000 and (g.n >= 4096) == (name != "small")
    T = fig["T"]
    assert T[1] >= 3 * T[0] and T[2] >= 6 * T[1]            # T grows hop by hop: integer ratios separate the cells


def test_the_equalities_hold():
    std, std1, full = cg.graph("std"), cg.graph("std-1"), cg.graph("std-full")
    T, F = std.figures()["T"], std.figures()["F"]
    assert std.nnz == 32 * T[1] and std1.nnz == 32 * T[1] - 1
    assert std.n == 8 * F[1] + 1 and full.n == 8 * F[1] and full.figures()["T"] == T and std1.figures()["T"] == T


def test_the_boundaries_are_the_strides():
    for (k, nl), compacts in cg.BOUNDARY_COMPACTS.items():
        g = cg.graph("cb-%d-%d" % (k, nl))
        assert g.figures()["nlive"][1] == nl
        assert compacts == (k >= 128 and cg.bits_stride(nl) < cg.bits_stride(k))
    assert [cg.bits_stride(x) for x in (64, 65, 128, 512, 513, 1024, 2048, 4095, 4096, 4097, 8192)] == \
        [1, 2, 2, 8, 16, 16, 32, 64, 64, 128, 128]


@pytest.mark.parametrize("cell", list(cg.CELLS))
def test_cell_inequalities(cell):
    g = cg.check(cell)
    print(cell, g.figures(), cg.CELLS[cell][2])


def test_a_wrong_path_is_refused():
    """check_cell is not vacuous: the neighbouring ratio, the other entry and the other compaction each fail it."""
    g = cg.graph("std")
    for kw in (dict(ratio=32, leave=1, how="push", pulls=("dense",)), dict(ratio=33, leave=1, how="scatter", zero="lazy", pulls=("sparse", "dense")),
               dict(ratio=33, leave=1, how="push", compact=True, pulls=("dense",)), dict(ratio=33, leave=1, how="push", pulls=("sparse",))):
        with pytest.raises(AssertionError):
            g.check_cell(3, **kw)
