/*
 * libcugraph_c vertex pairs and two-hop neighbours -- MI355X build.
 * ABI-compatible with the reference cpp/include/cugraph_c/graph_functions.h:27-100
 * (implementation c_api/graph_functions.cpp, whose two-hop body the reference snapshot leaves
 * unimplemented; algorithm traversal/two_hop_neighbors.cu).  Kernels: csrc/two_hop.hip.
 */
#pragma once
#include <cugraph_c/array.h>
#include <cugraph_c/error.h>
#include <cugraph_c/graph.h>
#include <cugraph_c/resource_handle.h>

#ifdef __cplusplus
extern "C" {
#endif

/* reference graph_functions.h:30-32 -- two arrays of vertex ids of one length, pair i = (first[i], second[i]) */
typedef struct { int32_t align_; } cugraph_vertex_pairs_t;

/*
 * reference graph_functions.h:49-55.  Both views are copied, so the caller's arrays may go once the
 * call returns.  The ids are external ids in the graph's vertex type, in any order; repeated pairs
 * and pairs (u, u) are allowed, and an id that is not in the graph is accepted here (the similarity
 * calls treat it as a vertex without neighbours).
 * CUGRAPH_INVALID_INPUT: "vertex type of graph and first must match" / "... second ..." when a view's
 * type differs from the graph's vertex type, and when the two views differ in length.
 */
cugraph_error_code_t cugraph_create_vertex_pairs(const cugraph_resource_handle_t* handle,
                                                 cugraph_graph_t* graph,
                                                 const cugraph_type_erased_device_array_view_t* first,
                                                 const cugraph_type_erased_device_array_view_t* second,
                                                 cugraph_vertex_pairs_t** vertex_pairs,
                                                 cugraph_error_t** error);

/* reference graph_functions.h:63 -- external ids, vertex type */
cugraph_type_erased_device_array_view_t* cugraph_vertex_pairs_get_first(cugraph_vertex_pairs_t* vertex_pairs);

/* reference graph_functions.h:72 */
cugraph_type_erased_device_array_view_t* cugraph_vertex_pairs_get_second(cugraph_vertex_pairs_t* vertex_pairs);

/* reference graph_functions.h:80 */
void cugraph_vertex_pairs_free(cugraph_vertex_pairs_t* vertex_pairs);

/*
 * reference graph_functions.h:95-100.  Every ordered pair (u, v), u != v, for which the graph has
 * a walk u -> w -> v over its out-edges, each pair once, in external ids.  A pair whose vertices
 * are also adjacent is included (as in traversal/two_hop_neighbors.cu).  Works on any single-GPU
 * graph, directed or not; a multi-GPU graph gives CUGRAPH_NOT_IMPLEMENTED.
 *
 * start_vertices: NULL for every vertex, or a list that restricts u (vertex type, external ids);
 * repeating an id in it does not repeat pairs, and an id that is not in the graph is
 * CUGRAPH_INVALID_INPUT.
 *
 * The order of the result is not specified, but it is the same from call to call (and for every
 * value of the handle option two_hop_budget, which bounds the temporary memory: source rows are
 * expanded in batches of at most that many walks).
 */
cugraph_error_code_t cugraph_two_hop_neighbors(const cugraph_resource_handle_t* handle,
                                               const cugraph_graph_t* graph,
                                               const cugraph_type_erased_device_array_view_t* start_vertices,
                                               cugraph_vertex_pairs_t** result,
                                               cugraph_error_t** error);

/*
 * An extracted subgraph as an edge list (the type and getters of later cuGraph releases' graph_functions.h;
 * the 22.10 reference has none).  cugraph_k_truss_subgraph (community_algorithms.h) returns one.
 */
typedef struct { int32_t align_; } cugraph_induced_subgraph_result_t;

/* external ids, vertex type */
cugraph_type_erased_device_array_view_t* cugraph_induced_subgraph_get_sources(
  cugraph_induced_subgraph_result_t* induced_subgraph);

/* external ids, vertex type */
cugraph_type_erased_device_array_view_t* cugraph_induced_subgraph_get_destinations(
  cugraph_induced_subgraph_result_t* induced_subgraph);

/* weight type, edge i's weight; NULL when the graph has no weights */
cugraph_type_erased_device_array_view_t* cugraph_induced_subgraph_get_edge_weights(
  cugraph_induced_subgraph_result_t* induced_subgraph);

/*
 * Number of subgraphs + 1 size_t values: subgraph i is the range [offsets[i], offsets[i + 1]) of the three
 * arrays ({0, number of edges} for the one subgraph of k-truss).  data_type_id_t of this ABI has no SIZE_T,
 * so the view's type id is INT64 (the same 8 bytes).
 */
cugraph_type_erased_device_array_view_t* cugraph_induced_subgraph_get_subgraph_offsets(
  cugraph_induced_subgraph_result_t* induced_subgraph);

void cugraph_induced_subgraph_result_free(cugraph_induced_subgraph_result_t* induced_subgraph);

/*
 * The subgraphs induced by vertex sets (the name and signature of later cuGraph releases; the 22.10
 * reference has no C entry, its C++ is structure/induced_subgraph_impl.cuh).  Kernels: csrc/subgraph.hip.
 *
 * subgraph_offsets: INT64, number of subgraphs + 1 entries (at least 1); it starts at 0, does not decrease
 * and ends at the size of subgraph_vertices.  subgraph_vertices: external ids in the graph's vertex type;
 * set i is the range [subgraph_offsets[i], subgraph_offsets[i + 1]).  The vertices of a set may come in any
 * order (the reference wants them sorted; the entry sorts each set by internal id itself) and a set may be
 * empty.
 *
 * Subgraph i holds every stored edge (u, v) of the out-edge orientation with u and v both in set i, with
 * its weight when the graph has weights: a self-loop of a member is such an edge, a repeated edge of a
 * multigraph comes back as often as it is stored, and both directions of an undirected edge come back.
 * Subgraphs appear in the order given; inside one, edges ascend by the internal id of the source and keep
 * the stored row order within a source.  The result is the same bytes from call to call and under every
 * value of the handle options sg_path and sg_split_min.
 *
 * CUGRAPH_INVALID_INPUT: graph or a view NULL, offsets that break the rules above, a type mismatch, an id
 * the graph does not know, a vertex repeated inside one set -- with or without do_expensive_check, which
 * adds nothing.  CUGRAPH_NOT_IMPLEMENTED: a multi-GPU graph, or subgraphs x vertices above 64 bits.
 * *result is NULL on error.
 */
cugraph_error_code_t cugraph_extract_induced_subgraph(
  const cugraph_resource_handle_t* handle,
  cugraph_graph_t* graph,
  const cugraph_type_erased_device_array_view_t* subgraph_offsets,
  const cugraph_type_erased_device_array_view_t* subgraph_vertices,
  bool_t do_expensive_check,
  cugraph_induced_subgraph_result_t** result,
  cugraph_error_t** error);

#ifdef __cplusplus
}
#endif
