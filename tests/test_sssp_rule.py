"""The oracle's SSSP predecessors on inputs with zero weights and ties: a tree, and
the rule tests/sssp_check.py restates -- checked by a checker that computes neither
through the oracle's own predecessor code.  (The rule "smallest tight in-neighbour"
alone gives cycles here: 1613, 1707 and 1708 of RMAT-11's 1709 vertices from
internal ids 1, V/2 and V-1 never got to the source, none from id 0.)"""
import numpy as np
import pytest

from oracle import graph as og
from oracle import sssp as osssp
from sssp_check import check_sssp, four_vertex, grid, pred_is_tree, rmat_edges


def _check(g, src, dtype=np.float32):
    dist, pred = osssp.sssp(g.num_vertices, g.offsets, g.indices, g.weights, src, dtype=dtype)
    return dist, pred, check_sssp(g.offsets, g.indices, g.weights, src, dist, pred)


def test_four_vertex():
    g = og.create_graph(*four_vertex(), renumber=False)
    dist, pred, rank = _check(g, 0)
    assert dist.tolist() == [0.0, 2.0, 2.0, 1.0]
    assert pred.tolist() == [-1, 3, 3, 0]


@pytest.mark.parametrize("src", [0, 517, 1023])
def test_grid_zero_one(src):
    g = og.create_graph(*grid(32, "01"), renumber=False)
    _, _, rank = _check(g, src)
    assert rank.max() > 1  # chains of equal-distance vertices: the level passes are exercised


@pytest.mark.parametrize("weights", [(0, 2), (1, 3)])
def test_rmat11_integer_weights(weights):
    g = og.create_graph(*rmat_edges(11, weights), renumber=True)
    V = g.num_vertices
    for src in (0, 1, V // 2, V - 1):
        _, _, rank = _check(g, src)
        assert (rank.max() > 0) == (weights[0] == 0)
    _check(g, 1, np.float64)


def test_absorbed_weight():
    """fp32: 2^25 + 1 rounds to 2^25, so the positive weight between a and b is tight
    both ways; the predecessors must still be a tree."""
    big = float(1 << 25)
    s, d, w = [0, 0, 1, 2], [1, 2, 2, 1], [big, big, 1.0, 1.0]
    g = og.create_graph(s, d, w, renumber=False)
    dist, pred, rank = _check(g, 0)
    assert pred.tolist() == [-1, 0, 0]


def test_checker_sees_a_cycle():
    g = og.create_graph(*four_vertex(), renumber=False)
    dist, _ = osssp.sssp(4, g.offsets, g.indices, g.weights, 0)
    bad = np.array([-1, 2, 1, 0])  # every entry a tight in-neighbour
    assert pred_is_tree(bad, 0, dist < np.finfo(np.float32).max).tolist() == [1, 2]
    with pytest.raises(AssertionError, match="not a tree"):
        check_sssp(g.offsets, g.indices, g.weights, 0, dist, bad)
