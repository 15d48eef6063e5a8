#!/usr/bin/env python3
"""Writes tests/golden/ego_vectors.json from NetworkX: for each golden dataset (the five undirected ones
as networkx.Graph, karate-asymmetric as networkx.DiGraph), four seeds (the smallest id, the id a third of
the way up, the largest id and the vertex of the largest out-degree) and radius 0 .. 3, the number of
vertices and of edges of networkx.ego_graph(G, seed, radius=r) -- NetworkX's edge count: an undirected
edge or a self-loop once -- and the full sorted edge list for three karate cases.

    python scripts/make_ego_golden.py
"""
import json
import os

import networkx as nx
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
DATASETS = {"karate.csv": False, "dolphins.csv": False, "polbooks.csv": False, "netscience.csv": False,
            "email-Eu-core.csv": False, "karate-asymmetric.csv": True}
RADII = [0, 1, 2, 3]
LISTED = {("karate.csv", 0, 1), ("karate.csv", 33, 1), ("karate-asymmetric.csv", 1, 1)}


def load(name, directed):
    data = np.loadtxt(os.path.join(GOLDEN, name), dtype=np.float64, ndmin=2)
    G = nx.DiGraph() if directed else nx.Graph()
    G.add_edges_from((int(a), int(b)) for a, b in data[:, :2])
    return G


def seeds_of(G):
    nodes = sorted(G.nodes())
    deg = G.out_degree if G.is_directed() else G.degree
    hub = max(nodes, key=lambda n: (deg(n), -n))
    return sorted({nodes[0], nodes[len(nodes) // 3], nodes[-1], hub})


def main():
    out = {"comment": "networkx %s; scripts/make_ego_golden.py" % nx.__version__, "datasets": {}}
    for name, directed in DATASETS.items():
        G = load(name, directed)
        facts = {}
        for seed in seeds_of(G):
            for r in RADII:
                E = nx.ego_graph(G, seed, radius=r)
                f = {"vertices": E.number_of_nodes(), "edges": E.number_of_edges()}
                if (name, seed, r) in LISTED:
                    f["edge_list"] = sorted([u, v] if directed else [min(u, v), max(u, v)] for u, v in E.edges())
                facts["%d/%d" % (seed, r)] = f
        out["datasets"][name] = facts
        print(name, {k: (f["vertices"], f["edges"]) for k, f in facts.items()})
    with open(os.path.join(GOLDEN, "ego_vectors.json"), "w") as f:
        json.dump(out, f, indent=None, sort_keys=True, separators=(",", ":"))
        f.write("\n")


if __name__ == "__main__":
    main()
