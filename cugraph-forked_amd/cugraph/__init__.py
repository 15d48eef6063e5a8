"""cugraph-compatible Python API over the MI355X libcugraph_c (hot path only).

Mirrors the reference's ``python/cugraph/cugraph`` surface for PageRank, BFS,
SSSP and Louvain: ``Graph`` / ``DiGraph`` with ``from_cudf_edgelist`` semantics
(structure/graph_classes.py:95-171, graph_implementation/simpleGraph.py:110-244:
symmetrise when undirected, drop duplicate edges keeping the minimum weight,
renumber in libcugraph_c), and the algorithm wrappers with their argument names,
defaults, result columns and NetworkX-graph handling.  cudf is not available in
this image: edge lists are pandas DataFrames (or dicts of numpy arrays / torch
tensors) and results come back as pandas DataFrames.
"""
from .structure import DiGraph, Graph, from_edgelist, from_pandas_edgelist
from .algorithms import (batched_ego_graphs, betweenness_centrality, bfs, connected_components, core_number,
                         edge_betweenness_centrality, ego_graph, eigenvector_centrality, hits, jaccard,
                         jaccard_coefficient, k_core, k_truss, katz_centrality, ktruss_subgraph, louvain, overlap,
                         overlap_coefficient,
                         pagerank, random_walks, shortest_path, shortest_path_length, sorensen, sorensen_coefficient,
                         sssp, strongly_connected_components, subgraph, triangle_count, uniform_neighbor_sample,
                         weakly_connected_components)
from . import generators
from . import dask  # noqa: F401  (multi-GPU, one process per GPU)

__all__ = ["Graph", "DiGraph", "from_edgelist", "from_pandas_edgelist", "pagerank", "bfs", "sssp",
           "shortest_path", "shortest_path_length", "louvain", "katz_centrality", "eigenvector_centrality", "hits",
           "betweenness_centrality", "edge_betweenness_centrality",
           "weakly_connected_components", "strongly_connected_components", "connected_components",
           "triangle_count", "core_number", "k_core", "ktruss_subgraph", "k_truss", "subgraph", "ego_graph",
           "batched_ego_graphs", "jaccard", "sorensen", "overlap", "jaccard_coefficient",
           "sorensen_coefficient", "overlap_coefficient", "uniform_neighbor_sample", "random_walks", "generators",
           "dask"]
