"""pylibcugraph-compatible Python surface over the MI355X libcugraph_c.

Mirrors the reference's Cython shim (``python/pylibcugraph/pylibcugraph``) for the
hot path: ``ResourceHandle`` (resource_handle.pyx:25-46), ``GraphProperties``
(graph_properties.pyx:17-35), ``SGGraph``/``MGGraph`` (graphs.pyx:60-330),
``pagerank`` (pagerank.pyx:57-224), ``personalized_pagerank``
(personalized_pagerank.pyx), ``bfs`` (bfs.pyx:59-200), ``sssp`` (sssp.pyx:52-178),
``louvain`` (louvain.pyx:58-149), ``weakly_connected_components``
(weakly_connected_components.pyx, components/_connectivity.pyx:132-220), ``triangle_count``
(triangle_count.pyx:57-60), ``core_number`` (core_number.pyx:58-140), ``k_core`` (the C
entry of core_algorithms.h), ``k_truss_subgraph`` (the signature of later pylibcugraph releases;
22.10 reaches its legacy k-truss from cugraph only), ``induced_subgraph`` / ``ego_graph`` (likewise the
signatures of later releases), ``jaccard_coefficients`` / ``sorensen_coefficients`` /
``overlap_coefficients`` (jaccard_coefficients.pyx:58-150 and its siblings) and
``get_two_hop_neighbors`` (the C entry of graph_functions.h), ``uniform_neighbor_sample``
(uniform_neighbor_sample.pyx), ``uniform_random_walks`` / ``biased_random_walks`` (uniform_random_walks.pyx) and
the ``node2vec`` stub, ``betweenness_centrality`` / ``edge_betweenness_centrality`` (the signatures of
later pylibcugraph releases; 22.10 has none) -- same argument names, order, return tuples and
exception types.  Arrays come back as GPU torch tensors (the reference returns
cupy arrays).
"""
from __future__ import annotations

import ctypes

from . import _lib
from ._arrays import (_NP_TO_C, DeviceArray, DeviceView, copy_view_to_tensor, copy_views_to_tensors, optional_view,
                      to_device_tensor, views_to_tensors_owned, vptr)

from . import generators  # noqa: E402,F401  (MI355X build extensions)
from . import comms  # noqa: E402,F401  (multi-GPU communicator contexts)

__all__ = ["trim_device_cache", "ResourceHandle", "GraphProperties", "SGGraph", "MGGraph", "pagerank",
           "personalized_pagerank", "katz_centrality", "eigenvector_centrality", "betweenness_centrality",
           "edge_betweenness_centrality", "hits", "bfs", "sssp",
           "louvain", "weakly_connected_components", "strongly_connected_components", "triangle_count",
           "core_number", "k_core", "k_truss_subgraph", "induced_subgraph", "ego_graph", "jaccard_coefficients",
           "sorensen_coefficients",
           "overlap_coefficients",
           "get_two_hop_neighbors", "uniform_neighbor_sample", "uniform_random_walks", "biased_random_walks",
           "node2vec", "version"]


def allocator_stats():
    """libcugraph_c's caching allocator counters: dict of driver allocations, their
    bytes and seconds, out-of-memory trims and the bytes cached now."""
    out = (ctypes.c_double * 5)()
    _lib.lib.cugraph_amd_allocator_stats(out)
    return {"mallocs": int(out[0]), "malloc_bytes": int(out[1]), "malloc_s": out[2], "oom_trims": int(out[3]),
            "cached_bytes": int(out[4])}


def trim_device_cache():
    """Return libcugraph_c's cached HBM blocks to the driver (ext.h
    cugraph_amd_trim_device_cache); call it beside torch.cuda.empty_cache().
    Returns the bytes released."""
    return int(_lib.lib.cugraph_amd_trim_device_cache())


def version():
    return _lib.lib.cugraph_amd_version().decode()


class ResourceHandle:
    """resource_handle.pyx:25-46.  ``handle`` may be a communicator pointer
    (``cugraph.dask.comms``) for multi-GPU use, else None."""

    def __init__(self, handle=None):
        p = None if handle is None else ctypes.c_void_p(int(handle))
        self.c_resource_handle_ptr = _lib.lib.cugraph_create_resource_handle(p)
        if not self.c_resource_handle_ptr:
            raise RuntimeError("cugraph_create_resource_handle failed")

    @property
    def ptr(self):
        return self.c_resource_handle_ptr

    def get_rank(self):
        return _lib.lib.cugraph_resource_handle_get_rank(self.c_resource_handle_ptr)

    # measurement hooks (include/cugraph_amd/ext.h)
    def set_profiling(self, enable=True):
        _lib.lib.cugraph_amd_set_profiling(self.c_resource_handle_ptr, 1 if enable else 0)

    def set_option(self, name, value):
        """Measurement / A-B switch of the kernels (cugraph_amd_set_option); ``None``
        or "defaults" restores the production settings."""
        if name is None:
            name, value = "defaults", 0
        _lib.call("cugraph_amd_set_option", self.c_resource_handle_ptr, name.encode(), float(value))

    def last_iterations(self):
        return _lib.lib.cugraph_amd_last_iterations(self.c_resource_handle_ptr)

    def last_hot_kernel_ms(self):
        return _lib.lib.cugraph_amd_last_hot_kernel_ms(self.c_resource_handle_ptr)

    def last_hot_kernel_launches(self):
        return _lib.lib.cugraph_amd_last_hot_kernel_launches(self.c_resource_handle_ptr)

    def last_bfs_levels(self):
        return _lib.lib.cugraph_amd_last_bfs_levels(self.c_resource_handle_ptr)

    def last_bfs_bottom_up_steps(self):
        return _lib.lib.cugraph_amd_last_bfs_bottom_up_steps(self.c_resource_handle_ptr)

    def last_louvain_levels(self):
        return _lib.lib.cugraph_amd_last_louvain_levels(self.c_resource_handle_ptr)

    def last_louvain_sweep_bytes(self):
        """Multi-GPU Louvain: average bytes this rank sent per local-move sweep."""
        return _lib.lib.cugraph_amd_last_louvain_sweep_bytes(self.c_resource_handle_ptr)

    def last_louvain_partition(self):
        """Multi-GPU Louvain: (level-0 edges, level-0 ghosts) of this rank's 1D share."""
        e, g = ctypes.c_int64(), ctypes.c_int64()
        _lib.lib.cugraph_amd_last_louvain_partition(self.c_resource_handle_ptr, ctypes.byref(e), ctypes.byref(g))
        return e.value, g.value

    def last_pagerank_schedule(self):
        """Push schedule of the last single-GPU PageRank call: (packed 16-bit stream
        entries, 0 for the other entry formats; vertices whose x~ the layout map moves,
        0 when the schedule has no map)."""
        n, m = ctypes.c_int64(), ctypes.c_int64()
        _lib.lib.cugraph_amd_last_pagerank_schedule(self.c_resource_handle_ptr, ctypes.byref(n), ctypes.byref(m))
        return n.value, m.value

    def last_pagerank_runs(self):
        """Run rows of the last single-GPU PageRank call's push schedule: (rows of 64
        entries of one source, the entries they hold); (0, 0) without run rows."""
        n, m = ctypes.c_int64(), ctypes.c_int64()
        _lib.lib.cugraph_amd_last_pagerank_runs(self.c_resource_handle_ptr, ctypes.byref(n), ctypes.byref(m))
        return n.value, m.value

    def last_pagerank_dense(self):
        """Dense wave segments of the last single-GPU PageRank call's push schedule:
        (512-entry segments of the packed stream flagged dense, all its segments);
        (0, 0) without a packed stream."""
        n, m = ctypes.c_int64(), ctypes.c_int64()
        _lib.lib.cugraph_amd_last_pagerank_dense(self.c_resource_handle_ptr, ctypes.byref(n), ctypes.byref(m))
        return n.value, m.value

    def measure_copy_bandwidth(self, nbytes=4 << 30, reps=10):
        """HBM ceiling: 16-B-per-lane copy kernel on this handle's stream, GB/s (read + write)."""
        r = _lib.lib.cugraph_amd_measure_copy_bandwidth(self.c_resource_handle_ptr, int(nbytes), int(reps))
        if r < 0:
            raise RuntimeError("cugraph_amd_measure_copy_bandwidth failed")
        return r

    def __del__(self, _sd=_lib.SHUTDOWN, _free=_lib.lib.cugraph_free_resource_handle):
        p = getattr(self, "c_resource_handle_ptr", None)
        if p and not _sd[0]:
            _free(p)
            self.c_resource_handle_ptr = None


class GraphProperties:
    """graph_properties.pyx:17-35."""

    def __init__(self, is_symmetric=False, is_multigraph=False):
        self.is_symmetric = bool(is_symmetric)
        self.is_multigraph = bool(is_multigraph)

    def _c(self):
        return _lib.GraphPropertiesStruct(int(self.is_symmetric), int(self.is_multigraph))

    def __getnewargs_ex__(self):
        return ((), {"is_symmetric": self.is_symmetric, "is_multigraph": self.is_multigraph})


class _GPUGraph:
    c_graph_ptr = None

    def number_of_vertices(self):
        return _lib.lib.cugraph_amd_graph_get_number_of_vertices(self.c_graph_ptr)

    def number_of_edges(self):
        return _lib.lib.cugraph_amd_graph_get_number_of_edges(self.c_graph_ptr)

    def adjacency(self, resource_handle, transposed=False):
        """(offsets, indices, weights|None) in internal ids (MI355X build extension)."""
        o, i, w = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
        _lib.call("cugraph_amd_graph_get_adjacency", resource_handle.ptr, self.c_graph_ptr,
                  1 if transposed else 0, ctypes.byref(o), ctypes.byref(i), ctypes.byref(w))
        h = resource_handle.ptr
        out = (DeviceArray(o.value).to_tensor(h), DeviceArray(i.value).to_tensor(h),
               DeviceArray(w.value).to_tensor(h) if w.value else None)
        return out

    def out_weight_sums(self, resource_handle):
        """Per-vertex out-weight sums in internal order (weight dtype; out-degrees when
        unweighted), as PageRank computes them (MI355X build extension)."""
        a = ctypes.c_void_p()
        _lib.call("cugraph_amd_graph_get_out_weight_sums", resource_handle.ptr, self.c_graph_ptr, ctypes.byref(a))
        return DeviceArray(a.value).to_tensor(resource_handle.ptr)


def _check_bool(name, v):
    if not isinstance(v, (int, bool)):
        raise TypeError(f"expected int or bool for {name}, got {type(v)}")


class SGGraph(_GPUGraph):
    """graphs.pyx:60-240."""

    def __init__(self, resource_handle, graph_properties, src_array, dst_array, weight_array,
                 store_transposed=False, renumber=False, do_expensive_check=False,
                 edge_id_array=None, edge_type_array=None):
        _check_bool("store_transposed", store_transposed)
        _check_bool("renumber", renumber)
        _check_bool("do_expensive_check", do_expensive_check)
        if edge_id_array is not None or edge_type_array is not None:
            raise NotImplementedError("edge ids / edge types are not supported by this build")
        src = DeviceView(src_array)
        dst = DeviceView(dst_array)
        if dst.c_type != src.c_type:
            dst = DeviceView(dst.tensor.to(src.tensor.dtype))
        wgt = optional_view(weight_array)
        props = graph_properties._c()
        g = ctypes.c_void_p()
        _lib.call("cugraph_sg_graph_create", resource_handle.ptr, ctypes.byref(props), src.ptr, dst.ptr,
                  vptr(wgt), None, None, int(bool(store_transposed)), int(bool(renumber)),
                  int(bool(do_expensive_check)), ctypes.byref(g))
        self.c_graph_ptr = g.value
        self._mg = False
        self._vertex_dtype = src.tensor.dtype

    def __del__(self, _sd=_lib.SHUTDOWN, _free=_lib.lib.cugraph_sg_graph_free):
        if getattr(self, "c_graph_ptr", None) and not _sd[0]:
            _free(self.c_graph_ptr)
            self.c_graph_ptr = None


class MGGraph(_GPUGraph):
    """graphs.pyx:247-330: collective over the communicator in the handle."""

    def __init__(self, resource_handle, graph_properties, src_array, dst_array, weight_array,
                 store_transposed=False, num_edges=-1, do_expensive_check=False,
                 edge_id_array=None, edge_type_array=None):
        _check_bool("store_transposed", store_transposed)
        src = DeviceView(src_array)
        dst = DeviceView(dst_array, src.tensor.dtype)
        wgt = optional_view(weight_array)
        if num_edges < 0:
            raise ValueError("num_edges (global edge count) is required for MGGraph")
        props = graph_properties._c()
        g = ctypes.c_void_p()
        _lib.call("cugraph_mg_graph_create", resource_handle.ptr, ctypes.byref(props), src.ptr, dst.ptr,
                  vptr(wgt), None, None, int(bool(store_transposed)), int(num_edges),
                  int(bool(do_expensive_check)), ctypes.byref(g))
        self.c_graph_ptr = g.value
        self._mg = True
        self._vertex_dtype = src.tensor.dtype

    def __del__(self, _sd=_lib.SHUTDOWN, _free=_lib.lib.cugraph_mg_graph_free):
        if getattr(self, "c_graph_ptr", None) and not _sd[0]:
            _free(self.c_graph_ptr)
            self.c_graph_ptr = None


def _centrality(api, resource_handle, graph, *views_and_scalars):
    res = ctypes.c_void_p()
    _lib.call(api, resource_handle.ptr, graph.c_graph_ptr, *views_and_scalars, ctypes.byref(res))
    v, x = views_to_tensors_owned(resource_handle.ptr, [_lib.lib.cugraph_centrality_result_get_vertices(res),
                                                        _lib.lib.cugraph_centrality_result_get_values(res)],
                                  res, _lib.lib.cugraph_centrality_result_free)
    return v, x


def pagerank(resource_handle, graph, precomputed_vertex_out_weight_vertices,
             precomputed_vertex_out_weight_sums, initial_guess_vertices, initial_guess_values,
             alpha, epsilon, max_iterations, do_expensive_check):
    """pagerank.pyx:57-224.  Returns (vertices, pageranks)."""
    a = optional_view(precomputed_vertex_out_weight_vertices)
    b = optional_view(precomputed_vertex_out_weight_sums)
    c = optional_view(initial_guess_vertices)
    d = optional_view(initial_guess_values)
    return _centrality("cugraph_pagerank", resource_handle, graph, vptr(a), vptr(b), vptr(c), vptr(d),
                       float(alpha), float(epsilon), int(max_iterations), int(bool(do_expensive_check)))


def personalized_pagerank(resource_handle, graph, precomputed_vertex_out_weight_vertices,
                          precomputed_vertex_out_weight_sums, initial_guess_vertices,
                          initial_guess_values, personalization_vertices, personalization_values,
                          alpha, epsilon, max_iterations, do_expensive_check):
    """personalized_pagerank.pyx.  Returns (vertices, pageranks)."""
    a = optional_view(precomputed_vertex_out_weight_vertices)
    b = optional_view(precomputed_vertex_out_weight_sums)
    c = optional_view(initial_guess_vertices)
    d = optional_view(initial_guess_values)
    e = optional_view(personalization_vertices)
    f = optional_view(personalization_values)
    return _centrality("cugraph_personalized_pagerank", resource_handle, graph, vptr(a), vptr(b), vptr(c),
                       vptr(d), vptr(e), vptr(f), float(alpha), float(epsilon), int(max_iterations),
                       int(bool(do_expensive_check)))


def _paths(resource_handle, res):
    v, d, p = views_to_tensors_owned(resource_handle.ptr, [_lib.lib.cugraph_paths_result_get_vertices(res),
                                                           _lib.lib.cugraph_paths_result_get_distances(res),
                                                           _lib.lib.cugraph_paths_result_get_predecessors(res)],
                                     res, _lib.lib.cugraph_paths_result_free)
    return v, d, p


def katz_centrality(resource_handle, graph, betas, alpha, beta, epsilon, max_iterations, do_expensive_check):
    """katz_centrality.pyx:57-155.  betas (optional) indexed by external vertex id.
    Returns (vertices, values)."""
    b = optional_view(betas)
    return _centrality("cugraph_katz_centrality", resource_handle, graph, vptr(b), float(alpha), float(beta),
                       float(epsilon), int(max_iterations), int(bool(do_expensive_check)))


def eigenvector_centrality(resource_handle, graph, epsilon, max_iterations, do_expensive_check):
    """eigenvector_centrality.pyx:57-136.  Returns (vertices, values)."""
    return _centrality("cugraph_eigenvector_centrality", resource_handle, graph, float(epsilon),
                       int(max_iterations), int(bool(do_expensive_check)))


def _betweenness_sources(resource_handle, graph, k, random_state):
    """The source list of a betweenness call as a view of the graph's vertex type, or None for every
    vertex.  An int draws ``random.Random(random_state).sample(range(n), k)``: positions in the
    order of the result's ``vertices`` (the reference samples indices, not identifiers,
    betweenness_centrality.py:298-309)."""
    if k is None:
        return None
    import random
    import numpy as np
    if isinstance(k, (int, np.integer)) and not isinstance(k, bool):
        n = graph.number_of_vertices()
        if k < 0 or k > n:
            raise ValueError(f"'k' must be in [0, {n}], got: {k}")
        picks = random.Random(random_state).sample(range(n), int(k))
        # the ids at those positions: a call without sources returns the number map and does no work
        empty = DeviceView(to_device_tensor(np.empty(0, np.int64)).to(graph._vertex_dtype))
        vertices, _ = _centrality("cugraph_betweenness_centrality", resource_handle, graph, empty.ptr, 0, 0, 0)
        ids = vertices[to_device_tensor(np.asarray(picks, np.int64))]
        return DeviceView(ids.contiguous())
    if isinstance(k, (list, tuple)):  # plain Python ids have no type of their own: the graph's
        return DeviceView(to_device_tensor(np.asarray(k, np.int64)), graph._vertex_dtype)
    return DeviceView(k)  # an array keeps its type; another one than the graph's is refused by the C entry


def betweenness_centrality(resource_handle, graph, k, random_state, normalized, include_endpoints,
                           do_expensive_check):
    """The C entry cugraph_betweenness_centrality with the signature later pylibcugraph releases give it.
    ``k``: None (every vertex is a source), an int (that many sources, drawn with
    ``random.Random(random_state)``) or an array of vertex ids of the graph's vertex type (every entry a
    source).  Returns (vertices, values); the values are float64."""
    src = _betweenness_sources(resource_handle, graph, k, random_state)
    return _centrality("cugraph_betweenness_centrality", resource_handle, graph, vptr(src), int(bool(normalized)),
                       int(bool(include_endpoints)), int(bool(do_expensive_check)))


def edge_betweenness_centrality(resource_handle, graph, k, random_state, normalized, do_expensive_check):
    """The C entry cugraph_edge_betweenness_centrality; ``k`` as in ``betweenness_centrality``.  Returns
    (src, dst, values): one entry per stored edge in the order of the graph's out-edge rows (both
    directions of an edge of a symmetric graph), float64 values."""
    src = _betweenness_sources(resource_handle, graph, k, random_state)
    res = ctypes.c_void_p()
    _lib.call("cugraph_edge_betweenness_centrality", resource_handle.ptr, graph.c_graph_ptr, vptr(src),
              int(bool(normalized)), int(bool(do_expensive_check)), ctypes.byref(res))
    s, d, x = views_to_tensors_owned(resource_handle.ptr,
                                     [_lib.lib.cugraph_edge_centrality_result_get_src_vertices(res),
                                      _lib.lib.cugraph_edge_centrality_result_get_dst_vertices(res),
                                      _lib.lib.cugraph_edge_centrality_result_get_values(res)],
                                     res, _lib.lib.cugraph_edge_centrality_result_free)
    return s, d, x


def hits(resource_handle, graph, tol, max_iter, initial_hubs_guess_vertices, initial_hubs_guess_values,
         normalized, do_expensive_check):
    """hits.pyx:58-193.  Returns (vertices, hubs, authorities)."""
    gv = optional_view(initial_hubs_guess_vertices)
    gs = optional_view(initial_hubs_guess_values)
    res = ctypes.c_void_p()
    _lib.call("cugraph_hits", resource_handle.ptr, graph.c_graph_ptr, float(tol), int(max_iter), vptr(gv), vptr(gs),
              int(bool(normalized)), int(bool(do_expensive_check)), ctypes.byref(res))
    h = resource_handle.ptr
    try:
        v = copy_view_to_tensor(h, _lib.lib.cugraph_hits_result_get_vertices(res))
        hb = copy_view_to_tensor(h, _lib.lib.cugraph_hits_result_get_hubs(res))
        au = copy_view_to_tensor(h, _lib.lib.cugraph_hits_result_get_authorities(res))
        resource_handle._last_hits = (_lib.lib.cugraph_hits_result_get_hub_score_differences(res),
                                      _lib.lib.cugraph_hits_result_get_number_of_iterations(res))
    finally:
        _lib.lib.cugraph_hits_result_free(res)
    return v, hb, au


def bfs(handle, graph, sources, direction_optimizing, depth_limit, compute_predecessors,
        do_expensive_check):
    """bfs.pyx:59-200.  depth_limit <= 0 means unlimited (bfs.pyx:148-149).
    Returns (distances, predecessors, vertices)."""
    # the library renumbers sources in place (bfs.cpp:96-114): hand it a private copy
    src = DeviceView(to_device_tensor(sources).clone())
    if depth_limit is None or depth_limit <= 0:
        depth_limit = 2 ** 31 - 2
    res = ctypes.c_void_p()
    _lib.call("cugraph_bfs", handle.ptr, graph.c_graph_ptr, src.ptr, int(bool(direction_optimizing)),
              int(depth_limit), int(bool(compute_predecessors)), int(bool(do_expensive_check)),
              ctypes.byref(res))
    v, d, p = _paths(handle, res)
    return d, p, v


def bfs_paths(resource_handle, graph, sources, destinations, depth_limit=0):
    """BFS (predecessors on) followed by ``cugraph_extract_paths`` on its result
    (reference traversal/extract_bfs_paths_impl.cuh; the reference declares the C
    entry in _cugraph_c/algorithms.pxd without a Python wrapper).  Returns
    (paths [len(destinations) x max_path_length] tensor, max_path_length)."""
    src = DeviceView(to_device_tensor(sources).clone())
    dst = DeviceView(to_device_tensor(destinations), src.tensor.dtype)
    if depth_limit is None or depth_limit <= 0:
        depth_limit = 2 ** 31 - 2
    res = ctypes.c_void_p()
    _lib.call("cugraph_bfs", resource_handle.ptr, graph.c_graph_ptr, src.ptr, 0, int(depth_limit), 1, 0,
              ctypes.byref(res))
    ep = ctypes.c_void_p()
    try:
        _lib.call("cugraph_extract_paths", resource_handle.ptr, graph.c_graph_ptr, src.ptr, res, dst.ptr,
                  ctypes.byref(ep))
    finally:
        _lib.lib.cugraph_paths_result_free(res)
    try:
        L = _lib.lib.cugraph_extract_paths_result_get_max_path_length(ep)
        paths = copy_view_to_tensor(resource_handle.ptr, _lib.lib.cugraph_extract_paths_result_get_paths(ep))
    finally:
        _lib.lib.cugraph_extract_paths_result_free(ep)
    return paths.reshape(-1, L) if L else paths, L


def sssp(resource_handle, graph, source, cutoff, compute_predecessors, do_expensive_check):
    """sssp.pyx:52-178.  Returns (vertices, distances, predecessors)."""
    res = ctypes.c_void_p()
    _lib.call("cugraph_sssp", resource_handle.ptr, graph.c_graph_ptr, int(source), float(cutoff),
              int(bool(compute_predecessors)), int(bool(do_expensive_check)), ctypes.byref(res))
    return _paths(resource_handle, res)


def louvain(resource_handle, graph, max_level, resolution, do_expensive_check):
    """louvain.pyx:58-149.  Returns (vertices, clusters, modularity)."""
    res = ctypes.c_void_p()
    _lib.call("cugraph_louvain", resource_handle.ptr, graph.c_graph_ptr, int(max_level), float(resolution),
              int(bool(do_expensive_check)), ctypes.byref(res))
    h = resource_handle.ptr
    try:
        v = copy_view_to_tensor(h, _lib.lib.cugraph_heirarchical_clustering_result_get_vertices(res))
        c = copy_view_to_tensor(h, _lib.lib.cugraph_heirarchical_clustering_result_get_clusters(res))
        q = _lib.lib.cugraph_heirarchical_clustering_result_get_modularity(res)
    finally:
        _lib.lib.cugraph_heirarchical_clustering_result_free(res)
    return v, c, q


def louvain_dendrogram(resource_handle, graph, max_level, resolution, do_expensive_check=False):
    """Extension (the reference C++ ``cugraph::louvain`` returns the Dendrogram,
    louvain_impl.cuh:280-301).  Returns (vertices, clusters, modularity, levels):
    ``levels[i]`` is this rank's slice of dendrogram level i (its level-i vertices
    in global-id order; values are level-(i+1) ids)."""
    res = ctypes.c_void_p()
    _lib.call("cugraph_louvain", resource_handle.ptr, graph.c_graph_ptr, int(max_level), float(resolution),
              int(bool(do_expensive_check)), ctypes.byref(res))
    h = resource_handle.ptr
    try:
        v = copy_view_to_tensor(h, _lib.lib.cugraph_heirarchical_clustering_result_get_vertices(res))
        c = copy_view_to_tensor(h, _lib.lib.cugraph_heirarchical_clustering_result_get_clusters(res))
        q = _lib.lib.cugraph_heirarchical_clustering_result_get_modularity(res)
        n = _lib.lib.cugraph_amd_heirarchical_clustering_result_get_num_levels(res)
        levels = [copy_view_to_tensor(h, _lib.lib.cugraph_amd_heirarchical_clustering_result_get_level(res, i))
                  for i in range(n)]
    finally:
        _lib.lib.cugraph_heirarchical_clustering_result_free(res)
    return v, c, q, levels


def _labeling(api, resource_handle, graph, do_expensive_check):
    res = ctypes.c_void_p()
    _lib.call(api, resource_handle.ptr, graph.c_graph_ptr, int(bool(do_expensive_check)), ctypes.byref(res))
    v, lab = views_to_tensors_owned(resource_handle.ptr, [_lib.lib.cugraph_labeling_result_get_vertices(res),
                                                          _lib.lib.cugraph_labeling_result_get_labels(res)],
                                    res, _lib.lib.cugraph_labeling_result_free)
    return v, lab


def _legacy_wcc(offsets, indices, weights, num_verts, num_edges, labels):
    """components/_connectivity.pyx:132-220: CSR in, ``labels`` (int32, length num_verts)
    filled in place.  The CSR must hold both directions of every edge."""
    import numpy as np
    import torch
    if num_verts is None or num_edges is None or labels is None:
        raise TypeError("the CSR form needs offsets, indices, weights, num_verts, num_edges and labels")
    num_verts, num_edges = int(num_verts), int(num_edges)
    off = to_device_tensor(offsets).to(torch.int64)
    idx = to_device_tensor(indices)
    if off.numel() != num_verts + 1 or idx.numel() < num_edges:
        raise ValueError("offsets / indices do not match num_verts / num_edges")
    is_np = isinstance(labels, np.ndarray)
    if not is_np and not isinstance(labels, torch.Tensor):
        raise TypeError("labels must be a torch tensor or a numpy array")
    if (labels.dtype != (np.int32 if is_np else torch.int32)) or len(labels) != num_verts:
        raise ValueError("labels must be int32 of length num_verts")
    idx = idx[:num_edges].to(torch.int32)
    src = torch.repeat_interleave(torch.arange(num_verts, dtype=torch.int32, device=idx.device), off[1:] - off[:-1])
    out = torch.arange(num_verts, dtype=torch.int32, device=idx.device)  # ids without edges: their own index
    if num_edges:
        h = ResourceHandle()
        g = SGGraph(h, GraphProperties(is_symmetric=True), src, idx, None, store_transposed=False, renumber=False)
        _, lab = _labeling("cugraph_weakly_connected_components", h, g, False)
        out[:lab.numel()] = lab
    if is_np:
        labels[:] = out.cpu().numpy()
    else:
        labels.copy_(out.to(labels.device))
    return labels


def weakly_connected_components(resource_handle, graph=None, do_expensive_check=False, *legacy):
    """weakly_connected_components.pyx.  Returns (vertices, labels): the label of a
    vertex is the smallest internal id of its component, so label L names
    ``vertices[L]`` (and is the smallest vertex id itself when the graph was built
    with renumber=False).

    The 22.10 CSR form ``weakly_connected_components(offsets, indices, weights,
    num_verts, num_edges, labels)`` is taken when the first argument is not a
    ResourceHandle; it fills ``labels`` in place."""
    if not isinstance(resource_handle, ResourceHandle):
        if len(legacy) > 3:
            raise TypeError("too many arguments")
        args = (resource_handle, graph, do_expensive_check) + legacy + (None,) * (3 - len(legacy))
        return _legacy_wcc(*args)
    if legacy:
        raise TypeError("weakly_connected_components(resource_handle, graph, do_expensive_check)")
    return _labeling("cugraph_weakly_connected_components", resource_handle, graph, do_expensive_check)


def strongly_connected_components(resource_handle, graph=None, do_expensive_check=False, *legacy):
    """Raises NotImplementedError through the C call, as the reference's C API does
    (c_api/strongly_connected_components.cpp:69)."""
    if not isinstance(resource_handle, ResourceHandle):
        raise NotImplementedError("strongly connected components is not implemented")
    return _labeling("cugraph_strongly_connected_components", resource_handle, graph, do_expensive_check)


def triangle_count(resource_handle, graph, start_list, do_expensive_check):
    """triangle_count.pyx:57-60.  Returns (vertices, counts): every vertex's number of
    triangles, counts in the graph's edge type.  ``start_list`` (None: every vertex)
    holds vertex ids of the graph's vertex type; they come back as ``vertices`` in the
    given order, duplicates kept.  An id that is not in the graph counts 0, or raises
    ValueError with ``do_expensive_check``."""
    start = optional_view(start_list)
    res = ctypes.c_void_p()
    _lib.call("cugraph_triangle_count", resource_handle.ptr, graph.c_graph_ptr, vptr(start),
              int(bool(do_expensive_check)), ctypes.byref(res))
    v, c = views_to_tensors_owned(resource_handle.ptr, [_lib.lib.cugraph_triangle_count_result_get_vertices(res),
                                                        _lib.lib.cugraph_triangle_count_result_get_counts(res)],
                                  res, _lib.lib.cugraph_triangle_count_result_free)
    return v, c


_DEGREE_TYPES = {"incoming": 0, "outgoing": 1, "bidirectional": 2}  # cugraph_k_core_degree_type_t


def _core_number(resource_handle, graph, degree_type_id, do_expensive_check):
    """cugraph_core_number with the C enum value given as it is (0 in, 1 out, 2 in + out)."""
    res = ctypes.c_void_p()
    _lib.call("cugraph_core_number", resource_handle.ptr, graph.c_graph_ptr, int(degree_type_id),
              int(bool(do_expensive_check)), ctypes.byref(res))
    v, c = views_to_tensors_owned(resource_handle.ptr, [_lib.lib.cugraph_core_result_get_vertices(res),
                                                        _lib.lib.cugraph_core_result_get_core_numbers(res)],
                                  res, _lib.lib.cugraph_core_result_free)
    return v, c


def core_number(resource_handle, graph, degree_type, do_expensive_check):
    """core_number.pyx:58-140.  Returns (vertices, core_numbers): every vertex's core number
    in the underlying simple graph (self-loops and repeated entries do not count), in the
    graph's edge type; the numbers NetworkX's ``core_number`` gives.  As in the reference a
    ``degree_type`` other than None is ignored with a warning.  The graph must be symmetric;
    with ``do_expensive_check`` a graph that has self-loops raises ValueError."""
    if degree_type is not None:
        import warnings
        warnings.warn("The 'degree_type' parameter is ignored in this release.", Warning)
    return _core_number(resource_handle, graph, _DEGREE_TYPES["incoming"], do_expensive_check)


def k_core(resource_handle, graph, k, degree_type, core_result, do_expensive_check):
    """C entry cugraph_k_core (core_algorithms.h; the reference snapshot has no binding for it
    and its C++ k_core is unimplemented).  Returns (src, dst, weights or None): the stored
    edges, both directions, whose endpoints both have a core number of at least ``k``, without
    self-loops and repeats.  ``core_result`` is None (the core numbers are computed inside
    with ``degree_type``: None / "incoming" / "outgoing" the ordinary ones, "bidirectional"
    twice those) or a pair (vertices, core_numbers) in the graph's vertex and edge types;
    vertices it does not list count as core 0, and an id that is not in the graph is skipped,
    or raises ValueError with ``do_expensive_check``."""
    if degree_type is not None and degree_type not in _DEGREE_TYPES:
        raise ValueError(f"'degree_type' must be one of {sorted(_DEGREE_TYPES)} or None, got: {degree_type}")
    if int(k) < 0:
        raise ValueError(f"'k' must be non-negative, got: {k}")
    h = resource_handle.ptr
    given = ctypes.c_void_p()
    views = None
    if core_result is not None:
        vertices, numbers = core_result
        views = (DeviceView(vertices), DeviceView(numbers))
        _lib.call("cugraph_core_result_create", h, views[0].ptr, views[1].ptr, ctypes.byref(given))
    res = ctypes.c_void_p()
    try:
        _lib.call("cugraph_k_core", h, graph.c_graph_ptr, int(k), _DEGREE_TYPES[degree_type or "incoming"], given,
                  int(bool(do_expensive_check)), ctypes.byref(res))
    finally:
        if given:
            _lib.lib.cugraph_core_result_free(given)
    ptrs = [_lib.lib.cugraph_k_core_result_get_src_vertices(res), _lib.lib.cugraph_k_core_result_get_dst_vertices(res)]
    w = _lib.lib.cugraph_k_core_result_get_weights(res)
    if w:
        ptrs.append(w)
    out = views_to_tensors_owned(h, ptrs, res, _lib.lib.cugraph_k_core_result_free)
    return out[0], out[1], (out[2] if w else None)


def k_truss_subgraph(resource_handle, graph, k, do_expensive_check):
    """C entry cugraph_k_truss_subgraph (community_algorithms.h; the name and return tuple of later
    pylibcugraph releases).  Returns (sources, destinations, edge_weights or None, subgraph_offsets):
    the stored edges, both directions of each, of the k-truss -- the maximal subgraph in which every
    edge lies in at least ``k - 2`` triangles of the subgraph, ``networkx.k_truss``'s convention --
    in the order of the graph's rows.  ``k <= 2`` gives every edge of the underlying simple graph;
    self-loops and repeated entries neither count nor come back.  ``subgraph_offsets`` is the int64
    pair [0, number of edges].  The graph must be symmetric (ValueError otherwise)."""
    if isinstance(k, bool) or int(k) != k or int(k) < 0:
        raise ValueError(f"'k' must be a non-negative integer, got: {k}")
    h = resource_handle.ptr
    res = ctypes.c_void_p()
    _lib.call("cugraph_k_truss_subgraph", h, graph.c_graph_ptr, int(k), int(bool(do_expensive_check)),
              ctypes.byref(res))
    ptrs = [_lib.lib.cugraph_induced_subgraph_get_sources(res), _lib.lib.cugraph_induced_subgraph_get_destinations(res),
            _lib.lib.cugraph_induced_subgraph_get_subgraph_offsets(res)]
    w = _lib.lib.cugraph_induced_subgraph_get_edge_weights(res)
    if w:
        ptrs.append(w)
    out = views_to_tensors_owned(h, ptrs, res, _lib.lib.cugraph_induced_subgraph_result_free)
    return out[0], out[1], (out[3] if w else None), out[2]


def _subgraph_result(h, res):
    ptrs = [_lib.lib.cugraph_induced_subgraph_get_sources(res), _lib.lib.cugraph_induced_subgraph_get_destinations(res),
            _lib.lib.cugraph_induced_subgraph_get_subgraph_offsets(res)]
    w = _lib.lib.cugraph_induced_subgraph_get_edge_weights(res)
    if w:
        ptrs.append(w)
    out = views_to_tensors_owned(h, ptrs, res, _lib.lib.cugraph_induced_subgraph_result_free)
    return out[0], out[1], (out[3] if w else None), out[2]


def induced_subgraph(resource_handle, graph, subgraph_vertices, subgraph_offsets, do_expensive_check):
    """C entry cugraph_extract_induced_subgraph (graph_functions.h; the name, argument order and return
    tuple of later pylibcugraph releases).  ``subgraph_vertices``: the vertex sets back to back, in the
    graph's vertex type and in any order inside a set; ``subgraph_offsets``: int64, sets + 1 entries, set
    ``i`` is ``subgraph_vertices[subgraph_offsets[i]:subgraph_offsets[i + 1]]``.  Returns (sources,
    destinations, edge_weights or None, subgraph_offsets): for every set the stored edges with both ends
    in it (loops and every copy of a repeated edge included), sets in the order given, edges by ascending
    internal source id and then stored order; the int64 offsets give each set's range.  ValueError: bad
    offsets, an id the graph does not know, a vertex repeated inside a set."""
    import torch
    h = resource_handle.ptr
    verts = DeviceView(subgraph_vertices)
    offs = DeviceView(subgraph_offsets, torch.int64)
    res = ctypes.c_void_p()
    _lib.call("cugraph_extract_induced_subgraph", h, graph.c_graph_ptr, offs.ptr, verts.ptr,
              int(bool(do_expensive_check)), ctypes.byref(res))
    return _subgraph_result(h, res)


def ego_graph(resource_handle, graph, source_vertices, radius, do_expensive_check):
    """C entry cugraph_extract_ego (community_algorithms.h; the name, argument order and return tuple of
    later pylibcugraph releases).  Returns (sources, destinations, edge_weights or None, subgraph_offsets)
    as ``induced_subgraph`` does, subgraph ``i`` induced by every vertex within ``radius`` hops over
    out-edges of ``source_vertices[i]``, the source included.  A source may repeat; no sources give no
    edges and the offsets [0].  ValueError: an id the graph does not know, a radius that is not a
    non-negative integer."""
    if isinstance(radius, bool) or int(radius) != radius or int(radius) < 0:
        raise ValueError(f"'radius' must be a non-negative integer, got: {radius}")
    h = resource_handle.ptr
    src = DeviceView(source_vertices)
    res = ctypes.c_void_p()
    _lib.call("cugraph_extract_ego", h, graph.c_graph_ptr, src.ptr, int(radius), int(bool(do_expensive_check)),
              ctypes.byref(res))
    return _subgraph_result(h, res)


def _similarity(api, resource_handle, graph, first, second, use_weight, do_expensive_check):
    h = resource_handle.ptr
    a, b = DeviceView(first), DeviceView(second)
    pairs = ctypes.c_void_p()
    _lib.call("cugraph_create_vertex_pairs", h, graph.c_graph_ptr, a.ptr, b.ptr, ctypes.byref(pairs))
    res = ctypes.c_void_p()
    try:
        _lib.call(api, h, graph.c_graph_ptr, pairs, int(bool(use_weight)), int(bool(do_expensive_check)),
                  ctypes.byref(res))
    finally:
        _lib.lib.cugraph_vertex_pairs_free(pairs)
    (score,) = views_to_tensors_owned(h, [_lib.lib.cugraph_similarity_result_get_similarity(res)], res,
                                      _lib.lib.cugraph_similarity_result_free)
    return a.tensor, b.tensor, score


def jaccard_coefficients(resource_handle, graph, first, second, use_weight, do_expensive_check):
    """jaccard_coefficients.pyx:58-150.  Returns (first, second, coefficients): for pair i =
    (first[i], second[i]), |N(u) & N(v)| / |N(u) | N(v)|, where N(x) is the set of distinct ids in
    x's stored row (a self-loop makes x a member, a repeated entry counts once).  Computed from the
    integers in double and rounded once to the graph's weight type (float32 without weights); a zero
    denominator scores 0.  ``first`` and ``second`` hold external ids in the graph's vertex type, in
    any order, repeats and (u, u) allowed; an id that is not in the graph scores 0, or raises
    ValueError with ``do_expensive_check``.  The graph must be symmetric; ``use_weight=True`` raises
    NotImplementedError."""
    return _similarity("cugraph_jaccard_coefficients", resource_handle, graph, first, second, use_weight,
                       do_expensive_check)


def sorensen_coefficients(resource_handle, graph, first, second, use_weight, do_expensive_check):
    """sorensen_coefficients.pyx.  As ``jaccard_coefficients`` with the score
    2 |N(u) & N(v)| / (|N(u)| + |N(v)|)."""
    return _similarity("cugraph_sorensen_coefficients", resource_handle, graph, first, second, use_weight,
                       do_expensive_check)


def overlap_coefficients(resource_handle, graph, first, second, use_weight, do_expensive_check):
    """overlap_coefficients.pyx.  As ``jaccard_coefficients`` with the score
    |N(u) & N(v)| / min(|N(u)|, |N(v)|)."""
    return _similarity("cugraph_overlap_coefficients", resource_handle, graph, first, second, use_weight,
                       do_expensive_check)


def get_two_hop_neighbors(resource_handle, graph, start_vertices=None):
    """C entry cugraph_two_hop_neighbors (graph_functions.h).  Returns (first, second): every
    ordered pair (u, v), u != v, with a walk u -> w -> v over the out-edges, each pair once, in
    external ids; pairs that are also adjacent are included.  ``start_vertices``: None for every
    vertex, or the ids u is restricted to (repeats do not repeat pairs; an id that is not in the
    graph raises ValueError).  The order is unspecified but the same from call to call."""
    h = resource_handle.ptr
    start = optional_view(start_vertices)
    res = ctypes.c_void_p()
    _lib.call("cugraph_two_hop_neighbors", h, graph.c_graph_ptr, vptr(start), ctypes.byref(res))
    first, second = views_to_tensors_owned(h, [_lib.lib.cugraph_vertex_pairs_get_first(res),
                                               _lib.lib.cugraph_vertex_pairs_get_second(res)],
                                           res, _lib.lib.cugraph_vertex_pairs_free)
    return first, second


def uniform_neighbor_sample(resource_handle, input_graph, start_list, h_fan_out, with_replacement,
                            do_expensive_check, return_counts=False):
    """uniform_neighbor_sample.pyx:60-170.  Returns (sources, destinations, indices): the distinct edges
    drawn over all hops, in no particular order; ``indices`` has the graph's weight type and carries each
    edge's weight bit for bit (ones for a graph without weights).  ``start_list`` holds external ids in the
    graph's vertex type, duplicates being slots of their own; ``h_fan_out`` is a non-empty host array of
    int32, one fan-out per hop, a value <= 0 taking every out-edge.  The sample is a pure function of the
    handle option ``sample_seed`` (default 0), the call's arguments and the graph
    (include/cugraph_c/sampling_algorithms.h).  ``return_counts=True`` (MI355X build extension) appends how
    often each edge was drawn."""
    import numpy as np
    h = resource_handle.ptr
    start = DeviceView(start_list)
    fan = np.ascontiguousarray(h_fan_out)
    if fan.dtype not in _NP_TO_C:
        raise TypeError(f"unsupported fan-out dtype {fan.dtype}")
    fview = _lib.lib.cugraph_type_erased_host_array_view_create(fan.ctypes.data_as(ctypes.c_void_p), fan.size,
                                                               _NP_TO_C[fan.dtype])
    res = ctypes.c_void_p()
    try:
        _lib.call("cugraph_uniform_neighbor_sample", h, input_graph.c_graph_ptr, start.ptr, fview,
                  int(bool(with_replacement)), int(bool(do_expensive_check)), ctypes.byref(res))
    finally:
        _lib.lib.cugraph_type_erased_host_array_view_free(fview)
    ptrs = [_lib.lib.cugraph_sample_result_get_sources(res), _lib.lib.cugraph_sample_result_get_destinations(res),
            _lib.lib.cugraph_sample_result_get_index(res)]
    if return_counts:
        ptrs.append(_lib.lib.cugraph_amd_sample_result_get_counts(res))
    return tuple(views_to_tensors_owned(h, ptrs, res, _lib.lib.cugraph_sample_result_free))


def _random_walks(api, resource_handle, input_graph, start_vertices, max_length):
    h = resource_handle.ptr
    start = DeviceView(start_vertices)
    res = ctypes.c_void_p()
    _lib.call(api, h, input_graph.c_graph_ptr, start.ptr, int(max_length), ctypes.byref(res))
    length = int(_lib.lib.cugraph_random_walk_result_get_max_path_length(res))
    ptrs = [_lib.lib.cugraph_random_walk_result_get_paths(res)]
    w = _lib.lib.cugraph_random_walk_result_get_weights(res)
    if w:
        ptrs.append(w)
    out = views_to_tensors_owned(h, ptrs, res, _lib.lib.cugraph_random_walk_result_free)
    return out[0], (out[1] if w else None), length


def uniform_random_walks(resource_handle, input_graph, start_vertices, max_length):
    """uniform_random_walks.pyx:50-120.  Returns (paths, weights, max_length): ``paths`` is
    [len(start_vertices) x (max_length + 1)] flattened row by row, external ids, each row starting with its
    start vertex; ``weights`` is [len(start_vertices) x max_length] in the graph's weight type, None for a
    graph without weights.  After a vertex without out-edges a row holds -1 and its weights 0.  Every step
    picks an out-edge uniformly; the walks are a pure function of the handle option ``sample_seed``, the
    start list and the graph."""
    return _random_walks("cugraph_uniform_random_walks", resource_handle, input_graph, start_vertices, max_length)


def biased_random_walks(resource_handle, input_graph, start_vertices, max_length):
    """C entry cugraph_biased_random_walks.  As ``uniform_random_walks`` with every step picking an out-edge
    with probability weight / sum of the row's weights; a row whose weights sum to 0 ends the walk.  The
    graph must have weights and none may be negative (ValueError)."""
    return _random_walks("cugraph_biased_random_walks", resource_handle, input_graph, start_vertices, max_length)


def node2vec(resource_handle, graph, seed_array, max_depth, compress_result, p, q):
    """node2vec.pyx:55-140.  Raises NotImplementedError through the C call: the node2vec biases are not
    implemented in this build."""
    start = DeviceView(seed_array)
    res = ctypes.c_void_p()
    _lib.call("cugraph_node2vec", resource_handle.ptr, graph.c_graph_ptr, start.ptr, int(max_depth),
              int(bool(compress_result)), float(p), float(q), ctypes.byref(res))
    raise NotImplementedError("node2vec is not implemented in this build")
