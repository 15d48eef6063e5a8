#!/usr/bin/env python3
"""Writes tests/golden/k_truss_vectors.json from NetworkX: for each of the five golden datasets and
k = 3, 4, 5, 6, 8 the number of undirected edges of networkx.k_truss(G, k) and the number of rounds a
round-synchronous peel needs (every edge whose support in the remaining graph is below k - 2 goes at
once, supports are then counted afresh with NetworkX; the rounds that remove something are counted),
and the full edge list for karate at k = 4 and 5.  The datasets' self-loops are dropped first, as
networkx.k_truss demands.

    python scripts/make_k_truss_golden.py
"""
import json
import os

import networkx as nx
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
DATASETS = ["karate.csv", "dolphins.csv", "polbooks.csv", "netscience.csv", "email-Eu-core.csv"]
KS = [3, 4, 5, 6, 8]
LISTED = {"karate.csv": [4, 5]}


def load(name):
    data = np.loadtxt(os.path.join(GOLDEN, name), dtype=np.float64, ndmin=2)
    G = nx.Graph()
    G.add_edges_from((int(a), int(b)) for a, b in data[:, :2] if int(a) != int(b))
    return G


def peel_rounds(G, k):
    H, rounds = G.copy(), 0
    while True:
        low = [(u, v) for u, v in H.edges() if len(set(H[u]) & set(H[v])) < k - 2]
        if not low:
            return H, rounds
        H.remove_edges_from(low)
        rounds += 1


def main():
    out = {"comment": "networkx %s; scripts/make_k_truss_golden.py" % nx.__version__, "datasets": {}}
    for name in DATASETS:
        G = load(name)
        facts = {}
        for k in KS:
            T = nx.k_truss(G, k)
            H, rounds = peel_rounds(G, k)
            assert {frozenset(e) for e in T.edges()} == {frozenset(e) for e in H.edges()}
            facts[str(k)] = {"edges": T.number_of_edges(), "rounds": rounds}
            if k in LISTED.get(name, []):
                facts[str(k)]["edge_list"] = sorted([min(u, v), max(u, v)] for u, v in T.edges())
        out["datasets"][name] = facts
        print(name, {k: (f["edges"], f["rounds"]) for k, f in facts.items()})
    with open(os.path.join(GOLDEN, "k_truss_vectors.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
