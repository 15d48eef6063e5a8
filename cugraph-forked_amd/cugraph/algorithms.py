"""cugraph algorithm wrappers (reference link_analysis/pagerank.py:61-244,
traversal/bfs.py:127-262, traversal/sssp.py:132-260, community/louvain.py:23-101).

Same names, argument order, defaults, result columns and error types; the
inputs may also be NetworkX graphs (results then use the NetworkX node labels, as
the reference's ``ensure_cugraph_obj_for_nx`` / ``df_score_to_dictionary``)."""
from __future__ import annotations

import warnings

import numpy as np

from .structure import DiGraph, Graph


def _plc():
    import pylibcugraph
    return pylibcugraph


def _is_nx(G):
    try:
        import networkx as nx
    except ImportError:
        return False
    return isinstance(G, nx.Graph)


class _NxView:
    """A NetworkX graph as a cugraph Graph over integer labels 0..n-1."""

    def __init__(self, nxG, weight="weight", store_transposed=False):
        import pandas as pd
        self.nodes = list(nxG.nodes())
        index = {n: i for i, n in enumerate(self.nodes)}
        rows = [(index[u], index[v], float(d.get(weight, 1.0)) if weight else 1.0)
                for u, v, d in nxG.edges(data=True)]
        arr = np.array(rows, dtype=np.float64).reshape(-1, 3)
        df = pd.DataFrame({"src": arr[:, 0].astype(np.int64), "dst": arr[:, 1].astype(np.int64), "w": arr[:, 2]})
        weighted = any("weight" in d for _, _, d in nxG.edges(data=True)) and weight is not None
        self.G = DiGraph() if nxG.is_directed() else Graph()
        self.G.from_pandas_edgelist(df, "src", "dst", "w" if weighted else None, renumber=True,
                                    store_transposed=store_transposed)
        self.index = index

    def label(self, ids):
        return [self.nodes[int(i)] if int(i) >= 0 else -1 for i in ids]

    def ids(self, labels):
        if np.isscalar(labels) or not hasattr(labels, "__len__"):
            labels = [labels]
        try:
            return [self.index[x] for x in labels]
        except KeyError:
            raise ValueError("A provided vertex was not valid") from None


def _frame_col(df, name):
    import torch
    c = df[name]
    if isinstance(c, torch.Tensor):
        return c
    if hasattr(c, "to_numpy"):
        c = c.to_numpy()
    return torch.as_tensor(np.asarray(c))


def _cuda_like(t, dtype):
    return t.to(dtype).cuda()


def _vertex_dtype(G):
    return G.edgelist["src"].dtype


def pagerank(G, alpha=0.85, personalization=None, precomputed_vertex_out_weight=None, max_iter=100, tol=1.0e-5,
             nstart=None, weight=None, dangling=None):
    """link_analysis/pagerank.py:61-244.  Returns DataFrame ['vertex', 'pagerank']
    (dict {node: score} for a NetworkX input)."""
    import pandas as pd
    import torch
    nxv = None
    if _is_nx(G):
        nxv = _NxView(G, weight or "weight", store_transposed=True)
        G = nxv.G
    if G.store_transposed is False:
        warnings.warn("Pagerank expects the 'store_transposed' flag to be set to 'True' for optimal performance "
                      "during the graph creation", UserWarning)
    p = _plc()
    vt = _vertex_dtype(G)
    wt = torch.float32 if G.edgelist["weights"] is None else G.edgelist["weights"].dtype

    def pair(df, vcol, xcol):
        if df is None:
            return None, None
        if nxv is not None:
            v = torch.as_tensor(nxv.ids(list(df[vcol])), dtype=torch.int64)
        else:
            v = _frame_col(df, vcol)
        return _cuda_like(v, vt), _cuda_like(_frame_col(df, xcol), wt)

    gv, gx = pair(nstart, "vertex", "values")
    ov, ox = pair(precomputed_vertex_out_weight, "vertex", "sums")
    h = p.ResourceHandle()
    if personalization is not None:
        pv, px = pair(personalization, "vertex", "values")
        vertex, values = p.personalized_pagerank(h, G._plc_graph, ov, ox, gv, gx, pv, px, alpha, tol, max_iter, False)
    else:
        vertex, values = p.pagerank(h, G._plc_graph, ov, ox, gv, gx, alpha, tol, max_iter, False)
    df = pd.DataFrame({"vertex": vertex.cpu().numpy(), "pagerank": values.cpu().numpy()})
    if nxv is not None:
        return dict(zip(nxv.label(df["vertex"]), df["pagerank"]))
    return df


def _starts(G, start, i_start, directed, nxv):
    if start is not None and i_start is not None:
        raise TypeError("cannot specify both 'start' and 'i_start'")
    if start is None and i_start is None:
        raise TypeError("must specify 'start' or 'i_start', but not both")
    if directed is not None:
        raise TypeError("'directed' cannot be specified for a Graph-type input")
    start = start if start is not None else i_start
    if nxv is not None:
        return nxv.ids(start)
    if hasattr(start, "columns"):
        start = start[start.columns[0]]
    if hasattr(start, "to_numpy"):
        start = start.to_numpy()
    s = np.atleast_1d(np.asarray(start)).astype(np.int64)
    for x in s:
        if not G.has_node(int(x)):
            raise ValueError("A provided vertex was not valid")
    return s.tolist()


def bfs(G, start=None, depth_limit=None, i_start=None, directed=None, return_predecessors=True):
    """traversal/bfs.py:127-262.  Returns DataFrame ['vertex', 'distance', 'predecessor']."""
    import pandas as pd
    import torch
    nxv = None
    if _is_nx(G):
        nxv = _NxView(G)
        G = nxv.G
    starts = _starts(G, start, i_start, directed, nxv)
    p = _plc()
    src = torch.as_tensor(starts, dtype=_vertex_dtype(G)).cuda()
    dist, pred, vertex = p.bfs(p.ResourceHandle(), G._plc_graph, src, False,
                               depth_limit if depth_limit is not None else -1, return_predecessors, False)
    df = pd.DataFrame({"vertex": vertex.cpu().numpy(), "distance": dist.cpu().numpy(),
                       "predecessor": (pred.cpu().numpy() if return_predecessors
                                       else np.full(vertex.numel(), -1, dtype=vertex.cpu().numpy().dtype))})
    if nxv is not None:
        df["vertex"] = nxv.label(df["vertex"])
        df["predecessor"] = nxv.label(df["predecessor"])
    return df


def sssp(G, source=None, method=None, directed=None, return_predecessors=None, unweighted=None, overwrite=None,
         indices=None, cutoff=None, edge_attr="weight"):
    """traversal/sssp.py:132-260.  Returns DataFrame ['distance', 'vertex', 'predecessor'];
    unweighted graphs use weight 1.0 (simpleGraph.py:840-843)."""
    import pandas as pd
    if source is None and indices is None:
        raise TypeError("must specify 'source' or 'indices', but not both")
    if source is not None and indices is not None:
        raise TypeError("must specify 'source' or 'indices', but not both")
    source = source if source is not None else indices
    nxv = None
    if _is_nx(G):
        nxv = _NxView(G, edge_attr)
        G = nxv.G
        source = nxv.ids(source)[0]
    elif not G.has_node(int(source)):
        raise ValueError("Starting vertex should be between 0 to number of vertices")
    if cutoff is None:
        cutoff = np.inf
    p = _plc()
    vertex, dist, pred = p.sssp(p.ResourceHandle(), G._weighted_plc_graph(), int(source), float(cutoff), True, False)
    df = pd.DataFrame({"distance": dist.cpu().numpy(), "vertex": vertex.cpu().numpy(),
                       "predecessor": pred.cpu().numpy()})
    if nxv is not None:
        df["vertex"] = nxv.label(df["vertex"])
        df["predecessor"] = nxv.label(df["predecessor"])
    return df


def shortest_path(G, source=None, method=None, directed=None, return_predecessors=None, unweighted=None,
                  overwrite=None, indices=None):
    """Alias of sssp (traversal/sssp.py)."""
    return sssp(G, source, method, directed, return_predecessors, unweighted, overwrite, indices)


def shortest_path_length(G, source, target=None):
    """traversal/sssp.py shortest_path_length: DataFrame ['vertex', 'distance'] or one distance."""
    df = sssp(G, source)
    if target is not None:
        hit = df.loc[df["vertex"] == target]
        if hit.empty:
            raise ValueError("Graph does not contain target vertex")
        return hit.iloc[0]["distance"]
    return df[["vertex", "distance"]].reset_index(drop=True)


def louvain(G, max_iter=100, resolution=1.0):
    """community/louvain.py:23-101.  Returns (DataFrame ['vertex', 'partition'], modularity)."""
    import pandas as pd
    nxv = None
    if _is_nx(G):
        nxv = _NxView(G)
        G = nxv.G
    if G.is_directed():
        raise ValueError("input graph must be undirected")
    p = _plc()
    vertex, part, q = p.louvain(p.ResourceHandle(), G._weighted_plc_graph(), max_iter, resolution, False)
    df = pd.DataFrame({"vertex": vertex.cpu().numpy(), "partition": part.cpu().numpy()})
    if nxv is not None:
        return dict(zip(nxv.label(df["vertex"]), df["partition"])), q
    return df, q


def _is_matrix(G):
    if isinstance(G, np.ndarray):
        return True
    try:
        import scipy.sparse as sp
    except ImportError:
        return False
    return sp.issparse(G)


def _ensure_args(api_name, G, directed, connection, return_labels):
    """components/connectivity.py:26-64: defaults and argument errors, before any GPU call."""
    if isinstance(G, Graph) or _is_nx(G):
        exc_value = "'%s' cannot be specified for a Graph-type input"
        if directed is not None:
            raise TypeError(exc_value % "directed")
        if return_labels is not None:
            raise TypeError(exc_value % "return_labels")
        directed = True
        return_labels = True
    else:
        directed = True if directed is None else directed
        return_labels = True if return_labels is None else return_labels
    want = {"strongly_connected_components": "strong", "weakly_connected_components": "weak"}.get(api_name)
    if want is None:
        raise RuntimeError(f"invalid API name specified (internal): {api_name}")
    if connection is not None and connection != want:
        raise TypeError(f"'connection' must be '{want}' for {api_name}()")
    return directed, want, return_labels


def _matrix_graph(M, directed):
    """A SciPy sparse matrix or a 2-D numpy array as a Graph over its row indices
    (renumber=False), and its number of rows."""
    import pandas as pd
    if isinstance(M, np.ndarray):
        if M.ndim != 2:
            raise TypeError("a numpy input must be a 2-D adjacency matrix")
        s, d = np.nonzero(M)
    else:
        coo = M.tocoo()
        s, d = coo.row, coo.col
    if M.shape[0] != M.shape[1]:
        raise ValueError("the adjacency matrix must be square")
    G = DiGraph() if directed else Graph()
    if len(s):
        G.from_pandas_edgelist(pd.DataFrame({"src": np.asarray(s, np.int64), "dst": np.asarray(d, np.int64)}),
                               "src", "dst", None, renumber=False)
    return G, int(M.shape[0])


def _components(api_name, G, directed, connection, return_labels):
    import pandas as pd
    directed, connection, return_labels = _ensure_args(api_name, G, directed, connection, return_labels)
    if not (isinstance(G, Graph) or _is_nx(G) or _is_matrix(G)):
        raise TypeError(f"input type {type(G)} is not a supported type.")
    p = _plc()
    run = p.weakly_connected_components if connection == "weak" else p.strongly_connected_components
    nxv = rows = None
    if _is_nx(G):
        nxv = _NxView(G)
        G = nxv.G
    elif _is_matrix(G):
        G, rows = _matrix_graph(G, directed)
    if G.edgelist is None:  # a matrix without entries
        if connection == "strong":
            raise NotImplementedError("SCC Not currently implemented")
        vertex = labels = np.zeros(0, np.int64)
    else:
        if connection == "weak" and G.is_directed():
            G = G.to_undirected()  # weak connectivity ignores the direction
        v, lab = run(p.ResourceHandle(), G._plc_graph, False)
        vertex, labels = v.cpu().numpy(), lab.cpu().numpy()
    if rows is not None:
        # rows without entries (trailing ones past the graph's last id too) are singletons
        out = np.arange(rows, dtype=labels.dtype if len(labels) else np.int32)
        out[vertex] = labels
        n_components = int(len(np.unique(out)))
        return (n_components, out) if return_labels else n_components
    df = pd.DataFrame({"labels": labels, "vertex": vertex})
    if nxv is not None:
        return dict(zip(nxv.label(df["vertex"]), df["labels"]))
    return df


def weakly_connected_components(G, directed=None, connection=None, return_labels=None):
    """components/connectivity.py:101-192.  Graph: DataFrame ['labels', 'vertex'];
    NetworkX graph: dict {node: label}; SciPy sparse matrix / 2-D numpy array:
    (n_components, labels by row index), or n_components with return_labels=False.
    The label of a vertex is the smallest internal id of its component (the smallest
    row index for a matrix)."""
    return _components("weakly_connected_components", G, directed, connection, return_labels)


def strongly_connected_components(G, directed=None, connection=None, return_labels=None):
    """components/connectivity.py:195-287.  Checks its arguments, then raises
    NotImplementedError as the reference's C API does."""
    return _components("strongly_connected_components", G, directed, connection, return_labels)


def connected_components(G, directed=None, connection="weak", return_labels=None):
    """components/connectivity.py:290-375."""
    if connection == "weak":
        return weakly_connected_components(G, directed, connection, return_labels)
    if connection == "strong":
        return strongly_connected_components(G, directed, connection, return_labels)
    raise ValueError(f"invalid connection type: {connection}, must be either 'strong' or 'weak'")


def triangle_count(G, start_list=None):
    """community/triangle_count.py:22-99.  Returns DataFrame ['vertex', 'counts']: the
    number of triangles every vertex (or every vertex of ``start_list``: an int, a list
    or a Series, in the given order) belongs to.  Undirected graphs only."""
    import pandas as pd
    import torch
    nxv = None
    if _is_nx(G):
        nxv = _NxView(G)
        G = nxv.G
    if G.is_directed():
        raise ValueError("input graph must be undirected")
    start = None
    if start_list is not None:
        if isinstance(start_list, (int, np.integer)) and not isinstance(start_list, bool):
            start_list = [start_list]
        if isinstance(start_list, list):
            start_list = pd.Series(nxv.ids(start_list) if nxv is not None else start_list, dtype=np.int64)
        elif nxv is not None and isinstance(start_list, pd.Series):
            start_list = pd.Series(nxv.ids(list(start_list)), dtype=np.int64)
        if not isinstance(start_list, pd.Series):
            raise TypeError(f"'start_list' must be either a list or a cudf.Series,"
                            f"got: {getattr(start_list, 'dtype', type(start_list))}")
        start = torch.as_tensor(start_list.to_numpy()).to(_vertex_dtype(G)).cuda()
    p = _plc()
    vertex, counts = p.triangle_count(p.ResourceHandle(), G._plc_graph, start, False)
    df = pd.DataFrame({"vertex": vertex.cpu().numpy(), "counts": counts.cpu().numpy()})
    if nxv is not None:
        df["vertex"] = nxv.label(df["vertex"])
    return df


def core_number(G, degree_type=None):
    """cores/core_number.py:25-101.  Returns DataFrame ['vertex', 'core_number'] (dict
    {node: core number} for a NetworkX input): the numbers ``networkx.core_number`` gives for
    the graph without its self-loops.  As in the reference ``degree_type`` is ignored with a
    warning.  Undirected graphs only."""
    import pandas as pd
    if degree_type is not None:
        warnings.warn("The 'degree_type' parameter is ignored in this release.", Warning)
    if G.is_directed():
        raise ValueError("input graph must be undirected")
    nxv = None
    if _is_nx(G):
        nxv = _NxView(G)
        G = nxv.G
    p = _plc()
    vertex, numbers = p.core_number(p.ResourceHandle(), G._plc_graph, None, False)
    df = pd.DataFrame({"vertex": vertex.cpu().numpy(), "core_number": numbers.cpu().numpy()})
    if nxv is not None:
        return dict(zip(nxv.label(df["vertex"]), df["core_number"]))
    return df


def k_core(G, k=None, core_number=None):
    """cores/k_core.py:39-129.  The k-core of G as a Graph of G's type (a NetworkX graph for a
    NetworkX input), with G's weights if it has them.  ``k`` None: the main core.
    ``core_number``: a precomputed DataFrame with columns 'vertex' and 'values'; None computes
    the core numbers.  A k above the largest core number gives a graph without edges."""
    import pandas as pd
    import torch
    if G.is_directed():
        raise ValueError("G must be an undirected Graph instance")
    nxv = None
    if _is_nx(G):
        nxv = _NxView(G)
        G = nxv.G
    out = type(G)()
    p = _plc()
    h = p.ResourceHandle()
    if core_number is not None:
        ids = _frame_col(core_number, "vertex")
        if nxv is not None:
            ids = torch.as_tensor(nxv.ids(list(ids.tolist())))
        # the C entry takes the numbers in the graph's edge type (capi_core.cpp: the vertex type below 2^31 - 1 edges)
        et = torch.int64 if G.edgelist["src"].numel() >= 2**31 - 1 else _vertex_dtype(G)
        given = (_cuda_like(ids, _vertex_dtype(G)), _cuda_like(_frame_col(core_number, "values"), et))
    else:
        given = p.core_number(h, G._plc_graph, None, False)
    if k is None:
        k = int(given[1].max().item()) if given[1].numel() else 0
    if not isinstance(k, (int, np.integer)) or isinstance(k, bool) or k < 0:
        raise ValueError(f"'k' must be a non-negative integer or None, got: {k}")
    src, dst, w = p.k_core(h, G._plc_graph, int(k), None, given, False)
    src, dst = src.cpu().numpy(), dst.cpu().numpy()
    w = None if w is None else w.cpu().numpy()
    if nxv is not None:
        import networkx as nx
        res = nx.Graph()
        labels_s, labels_d = nxv.label(src), nxv.label(dst)
        if w is None:
            res.add_edges_from(zip(labels_s, labels_d))
        else:
            res.add_weighted_edges_from(zip(labels_s, labels_d, w.tolist()))
        return res
    if len(src):
        cols = {"src": src, "dst": dst}
        if w is not None:
            cols["weights"] = w
        out.from_pandas_edgelist(pd.DataFrame(cols), "src", "dst", "weights" if w is not None else None,
                                 renumber=G._renumber, store_transposed=G.store_transposed)
    return out


def ktruss_subgraph(G, k, use_weights=True):
    """community/ktruss_subgraph.py:91-188.  The k-truss of G as a Graph of G's type: the maximal
    subgraph in which every edge lies in at least ``k - 2`` triangles of the subgraph (the
    reference's convention and ``networkx.k_truss``'s), so ``k <= 2`` keeps every edge.  Computed on
    the underlying simple graph.  G's weights are carried unless ``use_weights`` is False.  A k that
    leaves no edge gives a graph without edges.  Undirected graphs only; unlike the reference there
    is no CUDA-version check."""
    import pandas as pd
    if G.is_directed():
        raise ValueError("input graph must be undirected")
    if not isinstance(k, (int, np.integer)) or isinstance(k, bool) or k < 0:
        raise ValueError(f"'k' must be a non-negative integer, got: {k}")
    out = type(G)()
    p = _plc()
    src, dst, w, _ = p.k_truss_subgraph(p.ResourceHandle(), G._plc_graph, int(k), False)
    src, dst = src.cpu().numpy(), dst.cpu().numpy()
    w = None if (w is None or not use_weights) else w.cpu().numpy()
    if len(src):
        cols = {"src": src, "dst": dst}
        if w is not None:
            cols["weights"] = w
        out.from_pandas_edgelist(pd.DataFrame(cols), "src", "dst", "weights" if w is not None else None,
                                 renumber=G._renumber, store_transposed=G.store_transposed)
    return out


def k_truss(G, k):
    """community/ktruss_subgraph.py:30-88, the NetworkX-facing twin of ``ktruss_subgraph``: a
    NetworkX graph gives ``networkx.k_truss(G, k)`` as an ``nx.Graph`` with the original labels (and
    weights where G has them), a cugraph Graph gives ``ktruss_subgraph(G, k)``."""
    if G.is_directed():
        raise ValueError("input graph must be undirected")
    if not isinstance(k, (int, np.integer)) or isinstance(k, bool) or k < 0:
        raise ValueError(f"'k' must be a non-negative integer, got: {k}")
    if not _is_nx(G):
        return ktruss_subgraph(G, k)
    import networkx as nx
    nxv = _NxView(G)
    p = _plc()
    src, dst, w, _ = p.k_truss_subgraph(p.ResourceHandle(), nxv.G._plc_graph, int(k), False)
    labels_s, labels_d = nxv.label(src.cpu().numpy()), nxv.label(dst.cpu().numpy())
    res = nx.Graph()
    if w is None:
        res.add_edges_from(zip(labels_s, labels_d))
    else:
        res.add_weighted_edges_from(zip(labels_s, labels_d, w.cpu().numpy().tolist()))
    return res


def _check_radius(radius, center, undirected, distance):
    """The argument checks of ego_graph / batched_ego_graphs, before any GPU call."""
    if not isinstance(radius, (int, np.integer)) or isinstance(radius, bool) or radius < 0:
        raise ValueError(f"'radius' must be a non-negative integer, got: {radius}")
    if center is not True:
        raise NotImplementedError("center=False is not supported")
    if undirected is not False:
        raise NotImplementedError("undirected=True is not supported")
    if distance is not None:
        raise NotImplementedError("distance is not supported: distances are counted in hops")


def _vertex_list(G, nxv, vertices, what):
    """``vertices`` (a scalar, a list, an array, a Series or a one-column frame) as an int64 numpy
    array of G's ids; NetworkX labels go through the view's index."""
    if hasattr(vertices, "columns"):
        if len(vertices.columns) != 1:
            raise ValueError("multi-column vertex ids are not supported by this build")
        vertices = vertices[vertices.columns[0]]
    if hasattr(vertices, "to_numpy"):
        vertices = vertices.to_numpy()
    if isinstance(vertices, np.ndarray):
        vertices = vertices.tolist()
    elif hasattr(vertices, "cpu") and hasattr(vertices, "numpy"):
        vertices = vertices.cpu().numpy().tolist()
    elif np.isscalar(vertices) or not hasattr(vertices, "__len__"):
        vertices = [vertices]
    vertices = list(vertices)
    if nxv is not None:
        vertices = nxv.ids(vertices)
    for v in vertices:
        if not isinstance(v, (int, np.integer)) or isinstance(v, bool):
            raise ValueError(f"'{what}' must hold integer vertex ids, got: {v!r}")
    return np.asarray(vertices, dtype=np.int64)


def _subgraph_input(G, api):
    """(NetworkX view or None, Graph) with the distributed graph refused."""
    nxv = None
    if _is_nx(G):
        nxv = _NxView(G)
        G = nxv.G
    if G.is_distributed():
        raise NotImplementedError(f"{api} of a distributed graph is not implemented in this build")
    return nxv, G


def _extract(G, ids, offsets, radius):
    """The four host arrays (src, dst, weights or None, offsets) of the induced subgraphs
    (``offsets`` given) or the ego nets (``radius`` given) of ``ids``."""
    import torch
    if G.edgelist is None or G._plc_graph is None:
        if len(ids):
            raise ValueError("A provided vertex was not valid")
        n = 1 if offsets is None else len(offsets)
        return np.zeros(0, np.int64), np.zeros(0, np.int64), None, np.zeros(n, np.int64)
    p = _plc()
    dev = torch.as_tensor(ids).to(_vertex_dtype(G)).cuda()
    if offsets is not None:
        out = p.induced_subgraph(p.ResourceHandle(), G._plc_graph, dev, torch.as_tensor(offsets).cuda(), False)
    else:
        out = p.ego_graph(p.ResourceHandle(), G._plc_graph, dev, int(radius), False)
    src, dst, w, off = out
    return src.cpu().numpy(), dst.cpu().numpy(), (None if w is None else w.cpu().numpy()), off.cpu().numpy()


def _edges_to_graph(G, nxv, nx_directed, src, dst, w):
    """One extracted edge list as a Graph of G's type, or as a NetworkX graph with the view's labels."""
    import pandas as pd
    if nxv is not None:
        import networkx as nx
        res = nx.DiGraph() if nx_directed else nx.Graph()
        labels_s, labels_d = nxv.label(src), nxv.label(dst)
        if w is None:
            res.add_edges_from(zip(labels_s, labels_d))
        else:
            res.add_weighted_edges_from(zip(labels_s, labels_d, w.tolist()))
        return res
    out = type(G)(directed=G.is_directed()) if type(G) is Graph else type(G)()
    if len(src):
        cols = {"src": src, "dst": dst}
        if w is not None:
            cols["weights"] = w
        out.from_pandas_edgelist(pd.DataFrame(cols), "src", "dst", "weights" if w is not None else None,
                                 renumber=G._renumber, store_transposed=G.store_transposed)
    return out


def subgraph(G, vertices):
    """community/subgraph_extraction.py:22-87.  The subgraph of G induced by ``vertices`` (a list, an
    array or a Series, in any order) as a Graph of G's type (a NetworkX graph for a NetworkX input),
    with G's weights if it has them, built with G's ``renumber`` / ``store_transposed``.  Every stored
    edge with both ends in the set is kept, self-loops included.  An empty set, or one without edges
    inside, gives a graph without edges; a vertex G does not know, or one given twice, is a ValueError."""
    nx_directed = _is_nx(G) and G.is_directed()
    nxv, G = _subgraph_input(G, "subgraph")
    ids = _vertex_list(G, nxv, vertices, "vertices")
    src, dst, w, _ = _extract(G, ids, np.asarray([0, len(ids)], np.int64), None)
    return _edges_to_graph(G, nxv, nx_directed, src, dst, w)


def ego_graph(G, n, radius=1, center=True, undirected=False, distance=None):
    """community/egonet.py:47-113.  The subgraph induced by every vertex within ``radius`` hops of ``n``
    (over out-edges for a directed graph), ``n`` included, as a Graph of G's type or a NetworkX graph
    for a NetworkX input; weights are carried.  ``center=False``, ``undirected=True`` and a
    ``distance`` key, which the reference documents as unsupported and ignores, raise
    NotImplementedError here."""
    _check_radius(radius, center, undirected, distance)
    nx_directed = _is_nx(G) and G.is_directed()
    nxv, G = _subgraph_input(G, "ego_graph")
    ids = _vertex_list(G, nxv, n, "n")[:1]
    if len(ids) != 1:
        raise ValueError("'n' must be one vertex")
    src, dst, w, _ = _extract(G, ids, None, radius)
    return _edges_to_graph(G, nxv, nx_directed, src, dst, w)


def batched_ego_graphs(G, seeds, radius=1, center=True, undirected=False, distance=None):
    """community/egonet.py:116-177.  The ego nets of every seed at once.  Returns (DataFrame with
    'src', 'dst' and, for a weighted graph, 'weight'; Series of len(seeds) + 1 offsets): the edges of
    seed i's ego net are the rows [offsets[i], offsets[i + 1]).  For a NetworkX input the frame holds
    the NetworkX labels and the offsets are a list, as in the reference.  A seed may repeat; no seeds
    give an empty frame and the offsets [0].  The unsupported keywords raise as in ``ego_graph``."""
    import pandas as pd
    _check_radius(radius, center, undirected, distance)
    nxv, G = _subgraph_input(G, "batched_ego_graphs")
    ids = _vertex_list(G, nxv, seeds, "seeds")
    src, dst, w, off = _extract(G, ids, None, radius)
    if nxv is not None:
        src, dst = nxv.label(src), nxv.label(dst)
    cols = {"src": src, "dst": dst}
    if w is not None:
        cols["weight"] = w
    df = pd.DataFrame(cols)
    if nxv is not None:
        return df, off.tolist()
    return df, pd.Series(off)


def _similarity(G, vertex_pair, measure):
    """link_prediction/jaccard.py:21-134 and its siblings, for one of 'jaccard', 'sorensen',
    'overlap'."""
    import pandas as pd
    import torch
    if G.is_directed():
        raise ValueError("Input must be an undirected Graph.")
    if vertex_pair is not None and not isinstance(vertex_pair, pd.DataFrame):
        raise ValueError("vertex_pair must be a cudf dataframe")
    vt = _vertex_dtype(G)
    if vertex_pair is None:  # the stored edges, both directions
        e = G.edgelist
        first, second = e["src"].cpu().numpy(), e["dst"].cpu().numpy()
        order = np.lexsort((second, first))
        first, second = first[order], second[order]
    else:
        if vertex_pair.shape[1] < 2:
            raise ValueError("vertex_pair must have two columns")
        first, second = vertex_pair.iloc[:, 0].to_numpy(), vertex_pair.iloc[:, 1].to_numpy()
    p = _plc()
    a = torch.as_tensor(np.ascontiguousarray(first)).to(vt).cuda()
    b = torch.as_tensor(np.ascontiguousarray(second)).to(vt).cuda()
    f = getattr(p, measure + "_coefficients")
    a, b, score = f(p.ResourceHandle(), G._plc_graph, a, b, False, False)
    return pd.DataFrame({"source": a.cpu().numpy(), "destination": b.cpu().numpy(),
                         measure + "_coeff": score.cpu().numpy()})


def _similarity_coefficient(G, ebunch, measure):
    import pandas as pd
    nxv = None
    if _is_nx(G):
        if G.is_directed():
            raise ValueError("Input must be an undirected Graph.")
        nxv = _NxView(G)
        G = nxv.G
    pairs = None
    if ebunch is not None:
        if isinstance(ebunch, pd.DataFrame):
            pairs = ebunch
        else:
            ebunch = list(ebunch)
            us, vs = [u for u, _ in ebunch], [v for _, v in ebunch]
            if nxv is not None:
                us, vs = nxv.ids(us), nxv.ids(vs)
            pairs = pd.DataFrame({"first": np.asarray(us, dtype=np.int64), "second": np.asarray(vs, dtype=np.int64)})
    df = _similarity(G, pairs, measure)
    if nxv is not None:  # utilities/utils.py df_edge_score_to_dictionary
        return dict(zip(zip(nxv.label(df["source"]), nxv.label(df["destination"])),
                        df[measure + "_coeff"].tolist()))
    return df


def jaccard(input_graph, vertex_pair=None):
    """link_prediction/jaccard.py:21-134.  Returns DataFrame ['source', 'destination',
    'jaccard_coeff'], one row per pair in the order given: |N(u) & N(v)| / |N(u) | N(v)|, where
    N(x) is the set of distinct neighbours in x's stored row (a self-loop makes x its own
    neighbour).  ``vertex_pair`` is a DataFrame whose first two columns are the pairs; None means
    the graph's stored edges, both directions, sorted by (source, destination).  Scores are exact:
    the integer sizes in float64, rounded once to the graph's weight dtype (float32 without
    weights); a zero denominator scores 0.  Undirected graphs only."""
    return _similarity(input_graph, vertex_pair, "jaccard")


def sorensen(input_graph, vertex_pair=None):
    """link_prediction/sorensen.py.  As ``jaccard`` with column 'sorensen_coeff':
    2 |N(u) & N(v)| / (|N(u)| + |N(v)|)."""
    return _similarity(input_graph, vertex_pair, "sorensen")


def overlap(input_graph, vertex_pair=None):
    """link_prediction/overlap.py.  As ``jaccard`` with column 'overlap_coeff':
    |N(u) & N(v)| / min(|N(u)|, |N(v)|)."""
    return _similarity(input_graph, vertex_pair, "overlap")


def jaccard_coefficient(G, ebunch=None):
    """link_prediction/jaccard.py:137-190.  ``jaccard`` that also takes a NetworkX graph:
    ``ebunch`` is then a list of node pairs (None: every edge, both directions) and the result a
    dict {(u, v): score} in node labels.  For a Graph, ``ebunch`` may be a list of id pairs or a
    DataFrame and the result is ``jaccard``'s DataFrame."""
    return _similarity_coefficient(G, ebunch, "jaccard")


def sorensen_coefficient(G, ebunch=None):
    """link_prediction/sorensen.py.  See ``jaccard_coefficient``."""
    return _similarity_coefficient(G, ebunch, "sorensen")


def overlap_coefficient(G, ebunch=None):
    """link_prediction/overlap.py.  See ``jaccard_coefficient``."""
    return _similarity_coefficient(G, ebunch, "overlap")


def uniform_neighbor_sample(G, start_list, fanout_vals, with_replacement=True, is_edge_ids=False):
    """sampling/uniform_neighbor_sample.py:23-120.  Returns DataFrame ['sources', 'destinations',
    'indices']: the distinct edges drawn when every vertex of ``start_list`` (an int, a list or a Series;
    duplicates are sampled separately) picks ``fanout_vals[0]`` of its out-edges, their destinations pick
    ``fanout_vals[1]`` each, and so on; a fan-out <= 0 takes every out-edge.  'indices' is the edge's
    weight (1.0 for a graph without weights), cast back to int32 / int64 when the graph's edge list
    carried such values (edge ids).  ``is_edge_ids`` is accepted and unused, as in the reference.  The
    sample is the same on every call (pylibcugraph.uniform_neighbor_sample)."""
    import pandas as pd
    import torch
    if isinstance(start_list, (int, np.integer)) and not isinstance(start_list, bool):
        start_list = [start_list]
    if isinstance(fanout_vals, list):
        fanout_vals = np.asarray(fanout_vals, dtype="int32")
    else:
        raise TypeError(f"fanout_vals must be a list, got: {type(fanout_vals)}")
    if hasattr(start_list, "to_numpy"):
        start_list = start_list.to_numpy()
    start = torch.as_tensor(np.atleast_1d(np.asarray(start_list))).to(_vertex_dtype(G)).cuda()
    p = _plc()
    sources, destinations, indices = p.uniform_neighbor_sample(p.ResourceHandle(), G._plc_graph, start, fanout_vals,
                                                               bool(with_replacement), False)
    indices = indices.cpu().numpy()
    weight_t = getattr(G, "_weight_dtype", None)
    if weight_t in (np.dtype(np.int32), np.dtype(np.int64)):
        indices = indices.astype(weight_t)
    return pd.DataFrame({"sources": sources.cpu().numpy(), "destinations": destinations.cpu().numpy(),
                         "indices": indices})


def random_walks(G, start_vertices, max_depth=None, use_padding=False):
    """sampling/random_walks.py:19-104.  Uniform random walks of at most ``max_depth`` vertices from every
    vertex of ``start_vertices`` (an int, a list or a Series).  Returns (vertex_paths, edge_weight_paths,
    sizes) as pandas Series; sizes[i] is the number of vertices of walk i, which stops early at a vertex
    without out-edges.  ``use_padding=True``: every walk takes max_depth vertex entries (-1 after its end)
    and max_depth - 1 weight entries (0 after its end); otherwise the walks are coalesced, walk i taking
    sizes[i] vertices and sizes[i] - 1 weights.  A graph without weights gives weights of 1."""
    import pandas as pd
    import torch
    if max_depth is None:
        raise TypeError("must specify a 'max_depth'")
    nxv = None
    if _is_nx(G):
        nxv = _NxView(G)
        G = nxv.G
    if isinstance(start_vertices, (int, np.integer)) and not isinstance(start_vertices, bool):
        start_vertices = [start_vertices]
    if hasattr(start_vertices, "to_numpy"):
        start_vertices = start_vertices.to_numpy()
    if nxv is not None:
        start_vertices = nxv.ids(list(start_vertices))
    if int(max_depth) < 1:
        raise ValueError(f"'max_depth' must be a positive integer, got: {max_depth}")
    length = int(max_depth) - 1  # max_depth counts vertices, the C entry counts edges
    start = torch.as_tensor(np.atleast_1d(np.asarray(start_vertices))).to(_vertex_dtype(G)).cuda()
    p = _plc()
    paths, weights, _ = p.uniform_random_walks(p.ResourceHandle(), G._plc_graph, start, length)
    n = start.numel()
    paths = paths.cpu().numpy().reshape(n, length + 1)
    sizes = (paths >= 0).sum(axis=1).astype(np.int64)
    steps = np.arange(length)[None, :] < (sizes - 1)[:, None]
    weights = steps.astype(np.float32) if weights is None else weights.cpu().numpy().reshape(n, length)
    if use_padding:
        vertex_paths, edge_weight_paths = paths.reshape(-1), weights.reshape(-1)
    else:
        vertex_paths, edge_weight_paths = paths[paths >= 0], weights[steps]
    if nxv is not None:
        vertex_paths = np.asarray(nxv.label(vertex_paths), dtype=object)
    return pd.Series(vertex_paths), pd.Series(edge_weight_paths), pd.Series(sizes)


def _max_degree(G):
    import torch
    e = G.edgelist
    ids = torch.cat([e["src"], e["dst"]]) if G.is_directed() else e["src"]
    return int(torch.bincount(ids.to(torch.int64)).max().item()) if ids.numel() else 0


def katz_centrality(G, alpha=None, beta=1.0, max_iter=100, tol=1.0e-6, nstart=None, normalized=True):
    """centrality/katz_centrality.py:24-170.  Returns DataFrame ['vertex', 'katz_centrality']
    (dict for a NetworkX input).  As the reference, ``nstart`` is passed as the betas."""
    import pandas as pd
    import torch
    nxv = None
    if _is_nx(G):
        nxv = _NxView(G, store_transposed=True)
        G = nxv.G
    if alpha is None:
        alpha = 1.0 / _max_degree(G)
    if alpha <= 0.0:
        raise ValueError(f"'alpha' must be a positive float or None, got: {alpha}")
    if not isinstance(beta, float) or beta <= 0.0:
        raise ValueError(f"'beta' must be a positive float or None, got: {beta}")
    if not isinstance(max_iter, int) or max_iter <= 0:
        raise ValueError(f"'max_iter' must be a positive integer, got: {max_iter}")
    if not isinstance(tol, float) or tol <= 0.0:
        raise ValueError(f"'tol' must be a positive float, got: {tol}")
    betas = None
    if nstart is not None:
        wt = torch.float32 if G.edgelist["weights"] is None else G.edgelist["weights"].dtype
        betas = _cuda_like(_frame_col(nstart, "values"), wt)
    p = _plc()
    vertex, values = p.katz_centrality(p.ResourceHandle(), G._plc_graph, betas, alpha, beta, tol, max_iter, False)
    df = pd.DataFrame({"vertex": vertex.cpu().numpy(), "katz_centrality": values.cpu().numpy()})
    if nxv is not None:
        return dict(zip(nxv.label(df["vertex"]), df["katz_centrality"]))
    return df


def eigenvector_centrality(G, max_iter=100, tol=1.0e-6):
    """centrality/eigenvector_centrality.py.  Returns DataFrame ['vertex', 'eigenvector_centrality']."""
    import pandas as pd
    nxv = None
    if _is_nx(G):
        nxv = _NxView(G, store_transposed=True)
        G = nxv.G
    p = _plc()
    vertex, values = p.eigenvector_centrality(p.ResourceHandle(), G._plc_graph, tol, max_iter, False)
    df = pd.DataFrame({"vertex": vertex.cpu().numpy(), "eigenvector_centrality": values.cpu().numpy()})
    if nxv is not None:
        return dict(zip(nxv.label(df["vertex"]), df["eigenvector_centrality"]))
    return df


def _betweenness_setup(G, k, weight, result_dtype, what):
    """The checks of centrality/betweenness_centrality.py:120-131 and its ``_initialize_vertices``:
    returns (NetworkX view or None, Graph, k for pylibcugraph)."""
    if weight is not None:
        raise NotImplementedError(f"weighted implementation of {what} centrality not currently supported")
    if result_dtype not in [np.float32, np.float64]:
        raise TypeError("result type can only be np.float32 or np.float64")
    nxv = None
    if _is_nx(G):
        nxv = _NxView(G)
        G = nxv.G
    if k is not None and not (isinstance(k, (int, np.integer)) and not isinstance(k, bool)):
        # a list of identifiers (any sequence): the sources themselves
        ids = nxv.ids(list(k)) if nxv is not None else list(np.asarray(k).tolist())
        if any(not isinstance(i, (int, np.integer)) for i in ids):
            raise ValueError("A provided vertex was not valid")
        k = ids
    return nxv, G, k


def betweenness_centrality(G, k=None, normalized=True, weight=None, endpoints=False, seed=None,
                           result_dtype=np.float64):
    """centrality/betweenness_centrality.py:26-144.  Returns DataFrame ['vertex', 'betweenness_centrality']
    (dict {node: score} for a NetworkX input).  ``k``: None (every vertex is a source), an int (that many
    sources drawn with ``random.Random(seed)`` from the vertices' positions) or a list of vertex
    identifiers.  Weights of G are ignored; ``weight`` is not supported, ``endpoints`` is."""
    import pandas as pd
    nxv, G, k = _betweenness_setup(G, k, weight, result_dtype, "betweenness")
    p = _plc()
    vertex, values = p.betweenness_centrality(p.ResourceHandle(), G._plc_graph, k, seed, normalized, endpoints, False)
    df = pd.DataFrame({"vertex": vertex.cpu().numpy(),
                       "betweenness_centrality": values.cpu().numpy().astype(result_dtype)})
    if nxv is not None:
        return dict(zip(nxv.label(df["vertex"]), df["betweenness_centrality"]))
    return df


def edge_betweenness_centrality(G, k=None, normalized=True, weight=None, seed=None, result_dtype=np.float64):
    """centrality/betweenness_centrality.py:147-276.  Returns DataFrame ['src', 'dst',
    'betweenness_centrality'] (dict {(u, v): score} for a NetworkX input).  For an undirected graph the
    two directions of an edge are folded as the reference does (:260-271): swapped so that src < dst and
    summed, one row per edge.  ``k`` as in ``betweenness_centrality``."""
    import pandas as pd
    nxv, G, k = _betweenness_setup(G, k, weight, result_dtype, "edge betweenness")
    p = _plc()
    src, dst, values = p.edge_betweenness_centrality(p.ResourceHandle(), G._plc_graph, k, seed, normalized, False)
    df = pd.DataFrame({"src": src.cpu().numpy(), "dst": dst.cpu().numpy(),
                       "betweenness_centrality": values.cpu().numpy()})
    if not G.is_directed():
        lower = (df["src"] >= df["dst"]).to_numpy()
        s, d = df["src"].to_numpy().copy(), df["dst"].to_numpy().copy()
        s[lower], d[lower] = df["dst"].to_numpy()[lower], df["src"].to_numpy()[lower]
        df["src"], df["dst"] = s, d
        df = df.groupby(by=["src", "dst"]).sum().reset_index()
    df["betweenness_centrality"] = df["betweenness_centrality"].to_numpy().astype(result_dtype)
    if nxv is not None:
        return {(a, b): x for a, b, x in zip(nxv.label(df["src"]), nxv.label(df["dst"]), df["betweenness_centrality"])}
    return df


def hits(G, max_iter=100, tol=1.0e-5, nstart=None, normalized=True):
    """link_analysis/hits.py:26-120.  Returns DataFrame ['vertex', 'hubs', 'authorities']
    ((hubs dict, authorities dict) for a NetworkX input)."""
    import pandas as pd
    import torch
    nxv = None
    if _is_nx(G):
        nxv = _NxView(G, store_transposed=True)
        G = nxv.G
    if G.store_transposed is False:
        warnings.warn("HITS expects the 'store_transposed' flag to be set to 'True' for optimal performance during "
                      "the graph creation", UserWarning)
    gv = gx = None
    if nstart is not None:
        wt = torch.float32 if G.edgelist["weights"] is None else G.edgelist["weights"].dtype
        v = (torch.as_tensor(nxv.ids(list(nstart["vertex"]))) if nxv is not None else _frame_col(nstart, "vertex"))
        gv, gx = _cuda_like(v, _vertex_dtype(G)), _cuda_like(_frame_col(nstart, "values"), wt)
    p = _plc()
    vertex, hubs_, auth = p.hits(p.ResourceHandle(), G._plc_graph, tol, max_iter, gv, gx, normalized, False)
    df = pd.DataFrame({"vertex": vertex.cpu().numpy(), "hubs": hubs_.cpu().numpy(),
                       "authorities": auth.cpu().numpy()})
    if nxv is not None:
        lab = nxv.label(df["vertex"])
        return dict(zip(lab, df["hubs"])), dict(zip(lab, df["authorities"]))
    return df
