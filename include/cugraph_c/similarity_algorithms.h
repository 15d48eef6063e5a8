/*
 * libcugraph_c link prediction: Jaccard, Sorensen and overlap similarity -- MI355X build.
 * ABI-compatible with the reference cpp/include/cugraph_c/similarity_algorithms.h:29-131
 * (implementation c_api/similarity.cpp, whose body the reference snapshot leaves unimplemented;
 * algorithm link_prediction/similarity_impl.cuh and legacy/jaccard.cu).  Kernels:
 * csrc/similarity.hip.
 *
 * What the three calls compute, for pair i = (u, v) of vertex_pairs:
 *   N(x)  the set of distinct ids in x's stored row.  A self-loop makes x a member of N(x)
 *         (as networkx.jaccard_coefficient does); a repeated entry counts once.
 *   d(x) = |N(x)|,  c = |N(u) & N(v)|
 *   Jaccard  c / (d(u) + d(v) - c)
 *   Sorensen 2c / (d(u) + d(v))
 *   overlap  c / min(d(u), d(v))
 * A zero denominator scores 0, not NaN.  The score is computed from the integers in double and
 * rounded once to the graph's weight type (FLOAT32 for a graph without weights), so results are
 * exact and identical on every run.  Output i belongs to pair i; pairs may come in any order, be
 * repeated or be (u, u).  An id that is not in the graph counts as a vertex without neighbours
 * and scores 0; with do_expensive_check it is CUGRAPH_INVALID_INPUT ("invalid vertex IDs").
 *
 * The graph must be symmetric and not flagged multigraph (CUGRAPH_INVALID_INPUT otherwise) and
 * single-GPU (CUGRAPH_NOT_IMPLEMENTED otherwise).  use_weight = TRUE gives
 * CUGRAPH_NOT_IMPLEMENTED, "weighted similarity computations are not supported in this release";
 * a weighted graph with use_weight = FALSE is scored by its structure alone.
 * Handle options sim_path and sim_split_min (cugraph_amd/ext.h) change the timing only.
 */
#pragma once
#include <cugraph_c/array.h>
#include <cugraph_c/error.h>
#include <cugraph_c/graph.h>
#include <cugraph_c/graph_functions.h>
#include <cugraph_c/resource_handle.h>

#ifdef __cplusplus
extern "C" {
#endif

/* reference similarity_algorithms.h:32-34 -- one score per pair */
typedef struct { int32_t align_; } cugraph_similarity_result_t;

/* reference similarity_algorithms.h:42 -- weight type, similarity[i] belongs to pair i */
cugraph_type_erased_device_array_view_t* cugraph_similarity_result_get_similarity(
  cugraph_similarity_result_t* result);

/* reference similarity_algorithms.h:50 */
void cugraph_similarity_result_free(cugraph_similarity_result_t* result);

/* reference similarity_algorithms.h:71-77 */
cugraph_error_code_t cugraph_jaccard_coefficients(const cugraph_resource_handle_t* handle,
                                                  cugraph_graph_t* graph,
                                                  const cugraph_vertex_pairs_t* vertex_pairs,
                                                  bool_t use_weight,
                                                  bool_t do_expensive_check,
                                                  cugraph_similarity_result_t** result,
                                                  cugraph_error_t** error);

/* reference similarity_algorithms.h:98-104 */
cugraph_error_code_t cugraph_sorensen_coefficients(const cugraph_resource_handle_t* handle,
                                                   cugraph_graph_t* graph,
                                                   const cugraph_vertex_pairs_t* vertex_pairs,
                                                   bool_t use_weight,
                                                   bool_t do_expensive_check,
                                                   cugraph_similarity_result_t** result,
                                                   cugraph_error_t** error);

/* reference similarity_algorithms.h:125-131 */
cugraph_error_code_t cugraph_overlap_coefficients(const cugraph_resource_handle_t* handle,
                                                  cugraph_graph_t* graph,
                                                  const cugraph_vertex_pairs_t* vertex_pairs,
                                                  bool_t use_weight,
                                                  bool_t do_expensive_check,
                                                  cugraph_similarity_result_t** result,
                                                  cugraph_error_t** error);

#ifdef __cplusplus
}
#endif
