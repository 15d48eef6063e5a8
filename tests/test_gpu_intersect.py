"""Triangle counting and similarity share one sorted-row intersection (csrc/intersect.hpp); this
checks that its two users agree with each other through the identity

    sum over v in N(u) of |N(u) & N(v)|  =  2 * triangles(u)        for every vertex u

of a simple symmetric graph without self-loops or repeated entries.  The left side comes from
similarity: Sorensen on every stored entry (u, v) as a pair, on a graph with fp64 weights so that
the score is a double, and c = rint(sorensen * (d(u) + d(v)) / 2) with the degrees taken from the
host edge list (the score is 2c / (d(u) + d(v)) rounded once to a double, so the product is within
c * 2^-51 of c, and c <= 4096: far inside rint's half).  The right side comes from
triangle_count.  Both must also equal the
scipy count of test_gpu_triangle_count.py.  Every comparison is integer equality per vertex."""
import functools

import numpy as np
import pytest

from gpu_util import host, make_graph, plc
from test_gpu_triangle_count import symmetrize, truth_plain

pytestmark = pytest.mark.gpu


def clique_and_path():
    """K_70 on ids 0..69 (rows of 69 entries: the wave tier and a staged row) joined by the edge
    69-70 to a path on ids 70..269."""
    a, b = np.meshgrid(np.arange(70), np.arange(70), indexing="ij")
    keep = a < b
    p = np.arange(69, 269)
    return np.r_[a[keep], p], np.r_[b[keep], p + 1]


def rmat12():
    """The suite's R-MAT-12 edge list without its self-loops: V = 4096, hub rows above the
    1024-id stage."""
    from oracle.rmat import rmat
    s, d = rmat(12, 16 << 12, seed=7)
    return s[s != d], d[s != d]


@functools.lru_cache(maxsize=None)
def edges(name):
    """(s, d, degrees, 2 * triangles per vertex), everything indexed by id 0 .. max."""
    s, d = symmetrize(*{"clique_and_path": clique_and_path, "rmat12": rmat12}[name]())
    n = int(s.max()) + 1
    deg = np.bincount(s, minlength=n)
    return s, d, deg, 2 * truth_plain(s, d, n)


@pytest.mark.parametrize("renumber", (True, False))
@pytest.mark.parametrize("name", ("clique_and_path", "rmat12"))
def test_similarity_and_triangle_count_agree(name, renumber):
    s, d, deg, twice = edges(name)
    assert deg.max() >= 64 and (name != "rmat12" or deg.max() > 1024)
    h, g = make_graph(s, d, np.ones(len(s)), renumber=renumber, symmetric=True, wdtype=np.float64)
    for path in (0, 1, 2):
        h.set_option("tc_path", path)
        v, c = (host(x).astype(np.int64) for x in plc().triangle_count(h, g, None, False))
        tri = np.zeros(len(deg), np.int64)
        tri[v] = c
        assert np.array_equal(2 * tri, twice), f"tc_path={path}"
    h.set_option("sim_split_min", 128)
    for path in (0, 1, 2, 3):
        h.set_option("sim_path", path)
        _, _, x = plc().sorensen_coefficients(h, g, s.astype(np.int32), d.astype(np.int32), False, False)
        x = host(x)
        assert x.dtype == np.float64
        c = np.rint(x * (deg[s] + deg[d]) / 2.0).astype(np.int64)
        by_u = np.zeros(len(deg), np.int64)
        np.add.at(by_u, s, c)
        assert np.array_equal(by_u, twice), f"sim_path={path}"
