"""Writes tests/golden/betweenness_email_nx.npz: NetworkX's betweenness and edge betweenness centrality of
email-Eu-core.csv as a directed graph (a NetworkX call on it takes 5 to 9 seconds, too long to repeat in
every test run; the smaller datasets are computed by the tests themselves).

    python scripts/make_betweenness_golden.py

Arrays (float64):
    bc_n<normalized>_e<endpoints>  per vertex, in ascending id order
    ebc_n<normalized>              per distinct (src, dst) pair, in ascending (src, dst) order
plus ``networkx``, the version that computed them.
"""
import os

import networkx as nx
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def main():
    e = np.loadtxt(os.path.join(GOLDEN, "email-Eu-core.csv"), usecols=(0, 1), dtype=np.int64)
    pairs = np.unique(e, axis=0)
    ids = np.unique(pairs)
    G = nx.DiGraph()
    G.add_nodes_from(ids.tolist())
    G.add_edges_from(pairs.tolist())
    out = {"networkx": np.array(nx.__version__)}
    for normalized in (0, 1):
        for endpoints in (0, 1):
            bc = nx.betweenness_centrality(G, normalized=bool(normalized), endpoints=bool(endpoints))
            out[f"bc_n{normalized}_e{endpoints}"] = np.array([bc[int(i)] for i in ids], np.float64)
        ebc = nx.edge_betweenness_centrality(G, normalized=bool(normalized))
        out[f"ebc_n{normalized}"] = np.array([ebc[(int(a), int(b))] for a, b in pairs], np.float64)
    np.savez_compressed(os.path.join(GOLDEN, "betweenness_email_nx.npz"), **out)


if __name__ == "__main__":
    main()
