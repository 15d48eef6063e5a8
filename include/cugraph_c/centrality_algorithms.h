/*
 * libcugraph_c centrality entry points on the hot path -- MI355X build.
 * ABI-compatible with the reference cpp/include/cugraph_c/centrality_algorithms.h:36-171.
 */
#pragma once
#include <cugraph_c/array.h>
#include <cugraph_c/error.h>
#include <cugraph_c/graph.h>
#include <cugraph_c/resource_handle.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct { int32_t align_; } cugraph_centrality_result_t;

/* reference centrality_algorithms.h:46 -- external vertex ids (the number map) */
cugraph_type_erased_device_array_view_t* cugraph_centrality_result_get_vertices(
  cugraph_centrality_result_t* result);

/* reference centrality_algorithms.h:55 */
cugraph_type_erased_device_array_view_t* cugraph_centrality_result_get_values(
  cugraph_centrality_result_t* result);

/* reference centrality_algorithms.h:63 */
void cugraph_centrality_result_free(cugraph_centrality_result_t* result);

/*
 * reference centrality_algorithms.h:102-114 (implementation c_api/pagerank.cpp:244-304,
 * algorithm link_analysis/pagerank_impl.cuh:48-293).  Converges when the L1
 * difference of two consecutive iterates is < epsilon (plain epsilon, as the
 * reference implementation does); otherwise CUGRAPH_UNKNOWN_ERROR
 * ("PageRank failed to converge.") after max_iterations.
 */
cugraph_error_code_t cugraph_pagerank(
  const cugraph_resource_handle_t* handle,
  cugraph_graph_t* graph,
  const cugraph_type_erased_device_array_view_t* precomputed_vertex_out_weight_vertices,
  const cugraph_type_erased_device_array_view_t* precomputed_vertex_out_weight_sums,
  const cugraph_type_erased_device_array_view_t* initial_guess_vertices,
  const cugraph_type_erased_device_array_view_t* initial_guess_values,
  double alpha,
  double epsilon,
  size_t max_iterations,
  bool_t do_expensive_check,
  cugraph_centrality_result_t** result,
  cugraph_error_t** error);

/* reference centrality_algorithms.h:157-171 */
cugraph_error_code_t cugraph_personalized_pagerank(
  const cugraph_resource_handle_t* handle,
  cugraph_graph_t* graph,
  const cugraph_type_erased_device_array_view_t* precomputed_vertex_out_weight_vertices,
  const cugraph_type_erased_device_array_view_t* precomputed_vertex_out_weight_sums,
  const cugraph_type_erased_device_array_view_t* initial_guess_vertices,
  const cugraph_type_erased_device_array_view_t* initial_guess_values,
  const cugraph_type_erased_device_array_view_t* personalization_vertices,
  const cugraph_type_erased_device_array_view_t* personalization_values,
  double alpha,
  double epsilon,
  size_t max_iterations,
  bool_t do_expensive_check,
  cugraph_centrality_result_t** result,
  cugraph_error_t** error);

/*
 * Eigenvector centrality, reference centrality_algorithms.h:191-197
 * (centrality/eigenvector_centrality_impl.cuh): power method, L2 normalised,
 * stop when the L1 change < |V| * epsilon, else CUGRAPH_UNKNOWN_ERROR.
 */
cugraph_error_code_t cugraph_eigenvector_centrality(const cugraph_resource_handle_t* handle,
                                                    cugraph_graph_t* graph,
                                                    double epsilon,
                                                    size_t max_iterations,
                                                    bool_t do_expensive_check,
                                                    cugraph_centrality_result_t** result,
                                                    cugraph_error_t** error);

/*
 * Katz centrality, reference centrality_algorithms.h:224-233 (c_api/katz.cpp):
 * betas (optional) are indexed by external vertex id; results are L2 normalised.
 */
cugraph_error_code_t cugraph_katz_centrality(const cugraph_resource_handle_t* handle,
                                             cugraph_graph_t* graph,
                                             const cugraph_type_erased_device_array_view_t* betas,
                                             double alpha,
                                             double beta,
                                             double epsilon,
                                             size_t max_iterations,
                                             bool_t do_expensive_check,
                                             cugraph_centrality_result_t** result,
                                             cugraph_error_t** error);

/*
 * Betweenness centrality and edge betweenness centrality.  The 22.10 snapshot of the reference declares
 * neither in its C API (its Python layer reaches centrality/betweenness_centrality.cu through Cython); the
 * names and the argument order are the ones later cuGraph releases give these calls, the scores and their
 * scaling are the 22.10 implementation's (betweenness_centrality.cu:368-452).
 *
 * Brandes' algorithm on the unweighted graph (weights are ignored).  vertex_list holds the sources as
 * external ids of the graph's vertex type, every entry a source (a repeated id counts again); NULL means
 * every vertex.  With n vertices and k sources (k = n for NULL):
 *   vertex scores: normalized and n > 2: divided by (n - 1)(n - 2), or n(n - 1) with include_endpoints;
 *                  not normalized and the graph symmetric: divided by 2;
 *                  then, if k > 0, n > 2 and (normalized or symmetric): multiplied by n / k;
 *   edge scores:   normalized and n > 1: divided by n(n - 1); not normalized and symmetric: divided by 2.
 * Parallel edges count as distinct paths, self-loops contribute nothing.
 *
 * The values are always FLOAT64, whatever the graph's weight type: the scores are computed in double and
 * narrowing them is the caller's choice.  The vertex result is a cugraph_centrality_result_t (vertices: the
 * number map).  The edge result has one entry per stored edge, in the order of the graph's out-edge rows,
 * with external ids; a symmetric graph reports both directions of an edge.
 *
 * Errors: CUGRAPH_NOT_IMPLEMENTED for a multi-GPU graph; CUGRAPH_INVALID_INPUT for a vertex_list of
 * another type than the graph's vertices or one that holds an id the graph does not have (checked with or
 * without do_expensive_check).
 */
typedef struct {
  int32_t align_;
} cugraph_edge_centrality_result_t;

cugraph_error_code_t cugraph_betweenness_centrality(
  const cugraph_resource_handle_t* handle,
  cugraph_graph_t* graph,
  const cugraph_type_erased_device_array_view_t* vertex_list,
  bool_t normalized,
  bool_t include_endpoints,
  bool_t do_expensive_check,
  cugraph_centrality_result_t** result,
  cugraph_error_t** error);

cugraph_error_code_t cugraph_edge_betweenness_centrality(
  const cugraph_resource_handle_t* handle,
  cugraph_graph_t* graph,
  const cugraph_type_erased_device_array_view_t* vertex_list,
  bool_t normalized,
  bool_t do_expensive_check,
  cugraph_edge_centrality_result_t** result,
  cugraph_error_t** error);

cugraph_type_erased_device_array_view_t* cugraph_edge_centrality_result_get_src_vertices(
  cugraph_edge_centrality_result_t* result);
cugraph_type_erased_device_array_view_t* cugraph_edge_centrality_result_get_dst_vertices(
  cugraph_edge_centrality_result_t* result);
cugraph_type_erased_device_array_view_t* cugraph_edge_centrality_result_get_values(
  cugraph_edge_centrality_result_t* result);
void cugraph_edge_centrality_result_free(cugraph_edge_centrality_result_t* result);

/* HITS result, reference centrality_algorithms.h:238-290 */
typedef struct {
  int32_t align_;
} cugraph_hits_result_t;

cugraph_type_erased_device_array_view_t* cugraph_hits_result_get_vertices(cugraph_hits_result_t* result);
cugraph_type_erased_device_array_view_t* cugraph_hits_result_get_hubs(cugraph_hits_result_t* result);
cugraph_type_erased_device_array_view_t* cugraph_hits_result_get_authorities(cugraph_hits_result_t* result);
double cugraph_hits_result_get_hub_score_differences(cugraph_hits_result_t* result);
size_t cugraph_hits_result_get_number_of_iterations(cugraph_hits_result_t* result);
void cugraph_hits_result_free(cugraph_hits_result_t* result);

/* HITS, reference centrality_algorithms.h:322-332 (link_analysis/hits_impl.cuh) */
cugraph_error_code_t cugraph_hits(
  const cugraph_resource_handle_t* handle,
  cugraph_graph_t* graph,
  double epsilon,
  size_t max_iterations,
  const cugraph_type_erased_device_array_view_t* initial_hubs_guess_vertices,
  const cugraph_type_erased_device_array_view_t* initial_hubs_guess_values,
  bool_t normalize,
  bool_t do_expensive_check,
  cugraph_hits_result_t** result,
  cugraph_error_t** error);

#ifdef __cplusplus
}
#endif
