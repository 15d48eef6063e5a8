/*
 * libcugraph_c community entry points on the hot path -- MI355X build.
 * ABI-compatible with the reference cpp/include/cugraph_c/community_algorithms.h:35-136.
 */
#pragma once
#include <cugraph_c/error.h>
#include <cugraph_c/graph.h>
#include <cugraph_c/graph_functions.h>
#include <cugraph_c/resource_handle.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct { int32_t align_; } cugraph_triangle_count_result_t;

/*
 * reference community_algorithms.h:54-59 (implementation c_api/triangle_count.cpp,
 * algorithm community/triangle_count_impl.cuh).  Every vertex's number of triangles in the
 * underlying simple graph: self-loops and edge weights are ignored.  The graph must be
 * symmetric and not flagged multigraph.  start (may be NULL: every vertex) holds vertex ids
 * of the graph's vertex type; the result then lists them in the given order, duplicates
 * kept.  With do_expensive_check an id that is not in the graph is CUGRAPH_INVALID_INPUT,
 * without it such an id counts 0.  A count that does not fit a 32-bit edge type is
 * CUGRAPH_UNSUPPORTED_TYPE_COMBINATION, never a wrapped number.  Single GPU only.
 */
cugraph_error_code_t cugraph_triangle_count(const cugraph_resource_handle_t* handle,
                                            cugraph_graph_t* graph,
                                            const cugraph_type_erased_device_array_view_t* start,
                                            bool_t do_expensive_check,
                                            cugraph_triangle_count_result_t** result,
                                            cugraph_error_t** error);

/* reference community_algorithms.h:64 -- the graph's vertex ids, or the start ids */
cugraph_type_erased_device_array_view_t* cugraph_triangle_count_result_get_vertices(
  cugraph_triangle_count_result_t* result);

/* reference community_algorithms.h:70 -- counts[i] belongs to vertices[i]; edge type */
cugraph_type_erased_device_array_view_t* cugraph_triangle_count_result_get_counts(
  cugraph_triangle_count_result_t* result);

/* reference community_algorithms.h:78 */
void cugraph_triangle_count_result_free(cugraph_triangle_count_result_t* result);

/* [sic] "heirarchical", as in the reference ABI */
typedef struct { int32_t align_; } cugraph_heirarchical_clustering_result_t;

/*
 * reference community_algorithms.h:105-111 (implementation c_api/louvain.cpp:152,
 * algorithm community/louvain_impl.cuh:46-301).
 */
cugraph_error_code_t cugraph_louvain(const cugraph_resource_handle_t* handle,
                                     cugraph_graph_t* graph,
                                     size_t max_level,
                                     double resolution,
                                     bool_t do_expensive_check,
                                     cugraph_heirarchical_clustering_result_t** result,
                                     cugraph_error_t** error);

/* reference community_algorithms.h:116 */
cugraph_type_erased_device_array_view_t* cugraph_heirarchical_clustering_result_get_vertices(
  cugraph_heirarchical_clustering_result_t* result);

/* reference community_algorithms.h:122 */
cugraph_type_erased_device_array_view_t* cugraph_heirarchical_clustering_result_get_clusters(
  cugraph_heirarchical_clustering_result_t* result);

/* reference community_algorithms.h:128 */
double cugraph_heirarchical_clustering_result_get_modularity(
  cugraph_heirarchical_clustering_result_t* result);

/* reference community_algorithms.h:136 */
void cugraph_heirarchical_clustering_result_free(cugraph_heirarchical_clustering_result_t* result);

/*
 * k-truss subgraph (the name and signature of later cuGraph releases; the 22.10 reference reaches
 * community/legacy/ktruss.cu from Python only).  Kernels: csrc/k_truss.hip.
 *
 * The k-truss is the maximal subgraph in which every edge lies in at least k - 2 triangles of the
 * subgraph (the reference's convention, and networkx.k_truss's); k <= 2 returns every edge.  The
 * algorithm runs on the underlying simple graph: self-loops and repeated row entries neither form nor
 * count triangles and are not emitted; a repeated entry is represented by its first stored copy, weight
 * included.
 *
 * The result (graph_functions.h) holds the surviving stored edges, both directions of each, in external
 * ids and in the order of the graph's out-edge rows: the same from call to call and under every value of
 * the handle option kt_path.  Weights are carried bit for bit when the graph has them, otherwise the
 * weights view is NULL.  The result is a pure function of the graph and k.
 *
 * CUGRAPH_INVALID_INPUT: graph NULL, or a graph that is not symmetric.  CUGRAPH_NOT_IMPLEMENTED: a
 * multi-GPU graph.  *result is NULL on error.  do_expensive_check adds nothing: a missing reverse edge
 * is found while the edge ids are built and is CUGRAPH_INVALID_INPUT either way.
 */
cugraph_error_code_t cugraph_k_truss_subgraph(const cugraph_resource_handle_t* handle,
                                              cugraph_graph_t* graph,
                                              size_t k,
                                              bool_t do_expensive_check,
                                              cugraph_induced_subgraph_result_t** result,
                                              cugraph_error_t** error);

/*
 * Ego nets (the name and signature of later cuGraph releases; the 22.10 reference reaches
 * community/legacy/egonet.cu from Python only).  Kernels: csrc/subgraph.hip.
 *
 * Subgraph i is the subgraph induced (cugraph_extract_induced_subgraph, graph_functions.h: the same edges,
 * order and offsets) by every vertex reachable from source_vertices[i] over out-edges in at most radius
 * hops, the source included.  radius 0 gives the source's self-loops and nothing else; a radius above the
 * eccentricity gives the whole reachable set.  source_vertices holds external ids in the graph's vertex
 * type; a source may appear more than once and each occurrence gets its own, identical, subgraph.  An
 * empty source_vertices gives an empty result whose offsets are {0} (the reference refuses it).
 *
 * The sets of all sources grow together, a hop at a time, in batches of at most the handle option
 * ego_budget candidate keys; the result is the same bytes from call to call and under every value of
 * ego_budget, sg_path and sg_split_min.
 *
 * CUGRAPH_INVALID_INPUT: graph or source_vertices NULL, a type mismatch, an id the graph does not know
 * (with or without do_expensive_check).  CUGRAPH_NOT_IMPLEMENTED: a multi-GPU graph, or sources x vertices
 * above 64 bits.  *result is NULL on error.
 */
cugraph_error_code_t cugraph_extract_ego(const cugraph_resource_handle_t* handle,
                                         cugraph_graph_t* graph,
                                         const cugraph_type_erased_device_array_view_t* source_vertices,
                                         size_t radius,
                                         bool_t do_expensive_check,
                                         cugraph_induced_subgraph_result_t** result,
                                         cugraph_error_t** error);

#ifdef __cplusplus
}
#endif
