/*
 * libcugraph_c sampling: uniform neighbour sampling and random walks -- MI355X build.
 * ABI-compatible with the reference cpp/include/cugraph_c/sampling_algorithms.h:35-293
 * (implementation c_api/uniform_neighbor_sampling.cpp, c_api/random_walks.cpp; algorithms
 * sampling/uniform_neighbor_sampling_impl.hpp, sampling/random_walks_impl.cuh).  Kernels:
 * csrc/sampling.hip, csrc/random_walks.hip; single GPU (CUGRAPH_NOT_IMPLEMENTED otherwise).
 *
 * Every random choice is a pure function, defined in csrc/sample.hpp with sm = splitmix64 and
 * all arithmetic mod 2^64:
 *   draw(seed, stream, i, j) = sm(sm(sm(seed * 0x9E3779B97F4A7C15 ^ stream) ^ i) ^ j)
 *   index(r, n) = high 64 bits of r * n,   unit(r) = (r >> 11) * 2^-53
 * seed is the handle option sample_seed (cugraph_amd/ext.h; default 0 -- the reference's C API
 * passes seed 0 as well), so the same call gives the same result on every run, and
 * tests/sampling_ref.py reproduces it exactly on the CPU.
 *
 * Neighbour sample.  start holds external vertex ids (graph's vertex type; an id the graph lacks
 * is CUGRAPH_INVALID_INPUT); every entry, duplicates too, is slot i = its position of hop 0's
 * frontier.  fan_out is a non-empty host array of INT32, one entry K per hop.  A slot whose vertex
 * has d out-edges picks, in this order:
 *   d == 0                         nothing
 *   K <= 0                         all d edges in stored row order (ascending destination)
 *   with replacement               K edges; pick j is row position index(draw(seed, hop, i, j), d)
 *   without replacement, d <= K    all d edges in row order
 *   without replacement, d > K     Floyd's sampler: for t = 0 .. K-1, m = d - K + t,
 *                                  r = index(draw(seed, hop, i, t), m + 1); pick t is r unless an
 *                                  earlier pick of the slot is r, then m
 * The picks of a hop, slot after slot, are the slots of the next hop's frontier (their
 * destinations, duplicates kept).  The result is the set of distinct (source, destination, weight)
 * triples over all hops, in no order a caller may rely on: get_sources / get_destinations are
 * external ids, get_index has the graph's weight type and carries the edge's weight bit for bit
 * (ones, FLOAT32, for a graph without weights), and cugraph_amd_sample_result_get_counts
 * (cugraph_amd/ext.h) tells how often each triple was drawn.  get_start_labels and get_counts
 * return NULL for such a result: the reference never sets them on this path.
 *
 * Random walks.  Walk i starts at start_vertices[i]; step s from a vertex with d out-edges takes
 *   uniform   row position index(draw(seed, s, i, 0), d)
 *   biased    the first row position p with cum[p] > unit(draw(seed, s, i, 0)) * cum[d - 1], cum
 *             being the row's running sum of weights in double: probability weight / row total.
 *             Needs a weighted graph without negative weights (CUGRAPH_INVALID_INPUT); a row
 *             whose weights sum to 0 ends the walk like a vertex without out-edges.
 * get_paths is [n x (max_length + 1)] of vertex type, row major, external ids, column 0 the
 * start; get_weights is [n x max_length] of weight type, NULL for a graph without weights.  After
 * a vertex without out-edges the rest of the row is -1 and its weights 0.  get_path_sizes is NULL.
 * The node2vec calls return CUGRAPH_NOT_IMPLEMENTED.
 */
#pragma once
#include <cugraph_c/array.h>
#include <cugraph_c/error.h>
#include <cugraph_c/graph.h>
#include <cugraph_c/resource_handle.h>

#ifdef __cplusplus
extern "C" {
#endif

/* reference sampling_algorithms.h:35-37 */
typedef struct { int32_t align_; } cugraph_random_walk_result_t;

/* reference sampling_algorithms.h:52-58 */
cugraph_error_code_t cugraph_uniform_random_walks(const cugraph_resource_handle_t* handle,
                                                  cugraph_graph_t* graph,
                                                  const cugraph_type_erased_device_array_view_t* start_vertices,
                                                  size_t max_length,
                                                  cugraph_random_walk_result_t** result,
                                                  cugraph_error_t** error);

/* reference sampling_algorithms.h:73-79 */
cugraph_error_code_t cugraph_biased_random_walks(const cugraph_resource_handle_t* handle,
                                                 cugraph_graph_t* graph,
                                                 const cugraph_type_erased_device_array_view_t* start_vertices,
                                                 size_t max_length,
                                                 cugraph_random_walk_result_t** result,
                                                 cugraph_error_t** error);

/* reference sampling_algorithms.h:98-106 -- CUGRAPH_NOT_IMPLEMENTED */
cugraph_error_code_t cugraph_node2vec_random_walks(const cugraph_resource_handle_t* handle,
                                                   cugraph_graph_t* graph,
                                                   const cugraph_type_erased_device_array_view_t* start_vertices,
                                                   size_t max_length,
                                                   double p,
                                                   double q,
                                                   cugraph_random_walk_result_t** result,
                                                   cugraph_error_t** error);

/* reference sampling_algorithms.h:126-134 (deprecated there) -- CUGRAPH_NOT_IMPLEMENTED */
cugraph_error_code_t cugraph_node2vec(const cugraph_resource_handle_t* handle,
                                      cugraph_graph_t* graph,
                                      const cugraph_type_erased_device_array_view_t* sources,
                                      size_t max_depth,
                                      bool_t compress_result,
                                      double p,
                                      double q,
                                      cugraph_random_walk_result_t** result,
                                      cugraph_error_t** error);

/* reference sampling_algorithms.h:142 -- the max_length of the call */
size_t cugraph_random_walk_result_get_max_path_length(cugraph_random_walk_result_t* result);

/* reference sampling_algorithms.h:153 */
cugraph_type_erased_device_array_view_t* cugraph_random_walk_result_get_paths(
  cugraph_random_walk_result_t* result);

/* reference sampling_algorithms.h:162 -- NULL for a graph without weights */
cugraph_type_erased_device_array_view_t* cugraph_random_walk_result_get_weights(
  cugraph_random_walk_result_t* result);

/* reference sampling_algorithms.h:172 -- always NULL here */
cugraph_type_erased_device_array_view_t* cugraph_random_walk_result_get_path_sizes(
  cugraph_random_walk_result_t* result);

/* reference sampling_algorithms.h:180 */
void cugraph_random_walk_result_free(cugraph_random_walk_result_t* result);

/* reference sampling_algorithms.h:185-187 */
typedef struct { int32_t align_; } cugraph_sample_result_t;

/* reference sampling_algorithms.h:207-215 */
cugraph_error_code_t cugraph_uniform_neighbor_sample(const cugraph_resource_handle_t* handle,
                                                     cugraph_graph_t* graph,
                                                     const cugraph_type_erased_device_array_view_t* start,
                                                     const cugraph_type_erased_host_array_view_t* fan_out,
                                                     bool_t with_replacement,
                                                     bool_t do_expensive_check,
                                                     cugraph_sample_result_t** result,
                                                     cugraph_error_t** error);

/* reference sampling_algorithms.h:223 */
cugraph_type_erased_device_array_view_t* cugraph_sample_result_get_sources(const cugraph_sample_result_t* result);

/* reference sampling_algorithms.h:232 */
cugraph_type_erased_device_array_view_t* cugraph_sample_result_get_destinations(
  const cugraph_sample_result_t* result);

/* reference sampling_algorithms.h:242 -- always NULL here */
cugraph_type_erased_device_array_view_t* cugraph_sample_result_get_start_labels(
  const cugraph_sample_result_t* result);

/* reference sampling_algorithms.h:251 -- weight type, the edges' weight bits */
cugraph_type_erased_device_array_view_t* cugraph_sample_result_get_index(const cugraph_sample_result_t* result);

/* reference sampling_algorithms.h:261 -- NULL for the result of a sample call; for a result of
 * cugraph_test_sample_result_create a host copy of the counts it was given */
cugraph_type_erased_host_array_view_t* cugraph_sample_result_get_counts(const cugraph_sample_result_t* result);

/* reference sampling_algorithms.h:269 */
void cugraph_sample_result_free(cugraph_sample_result_t* result);

/* reference sampling_algorithms.h:286-293 -- testing aid: a result holding copies of four arrays */
cugraph_error_code_t cugraph_test_sample_result_create(const cugraph_resource_handle_t* handle,
                                                       const cugraph_type_erased_device_array_view_t* srcs,
                                                       const cugraph_type_erased_device_array_view_t* dsts,
                                                       const cugraph_type_erased_device_array_view_t* weights,
                                                       const cugraph_type_erased_device_array_view_t* counts,
                                                       cugraph_sample_result_t** result,
                                                       cugraph_error_t** error);

#ifdef __cplusplus
}
#endif
