/*
 * libcugraph_c core number / k-core entry points -- MI355X build.
 * ABI-compatible with the reference cpp/include/cugraph_c/core_algorithms.h:31-174
 * (implementation c_api/core_number.cpp, c_api/k_core.cpp, c_api/core_result.cpp; algorithm
 * cores/core_number_impl.cuh).  Kernels: csrc/core_number.hip.
 */
#pragma once
#include <cugraph_c/array.h>
#include <cugraph_c/error.h>
#include <cugraph_c/graph.h>
#include <cugraph_c/resource_handle.h>

#ifdef __cplusplus
extern "C" {
#endif

/* reference core_algorithms.h:31-33 -- vertex ids and their core numbers */
typedef struct { int32_t align_; } cugraph_core_result_t;

/* reference core_algorithms.h:38-40 -- the edges of a k-core */
typedef struct { int32_t align_; } cugraph_k_core_result_t;

/*
 * reference core_algorithms.h:124-128.  The graphs these calls accept are symmetric, so IN
 * and OUT give the same, ordinary core number; INOUT counts every neighbour twice and gives
 * exactly twice that (core_number_impl.cuh:110-122).
 */
typedef enum {
  K_CORE_DEGREE_TYPE_IN    = 0,
  K_CORE_DEGREE_TYPE_OUT   = 1,
  K_CORE_DEGREE_TYPE_INOUT = 2
} cugraph_k_core_degree_type_t;

/*
 * reference core_algorithms.h:53-58 (c_api/core_result.cpp): a core result from two arrays the
 * caller already has, e.g. kept from an earlier cugraph_core_number.  Both views are copied;
 * they must have the same length.  vertices holds external ids in any order.
 */
cugraph_error_code_t cugraph_core_result_create(const cugraph_resource_handle_t* handle,
                                                cugraph_type_erased_device_array_view_t* vertices,
                                                cugraph_type_erased_device_array_view_t* core_numbers,
                                                cugraph_core_result_t** core_result,
                                                cugraph_error_t** error);

/* reference core_algorithms.h:66 */
cugraph_type_erased_device_array_view_t* cugraph_core_result_get_vertices(cugraph_core_result_t* result);

/* reference core_algorithms.h:75 -- core_numbers[i] belongs to vertices[i]; edge type */
cugraph_type_erased_device_array_view_t* cugraph_core_result_get_core_numbers(cugraph_core_result_t* result);

/* reference core_algorithms.h:83 */
void cugraph_core_result_free(cugraph_core_result_t* result);

/* reference core_algorithms.h:91 -- external ids, vertex type */
cugraph_type_erased_device_array_view_t* cugraph_k_core_result_get_src_vertices(cugraph_k_core_result_t* result);

/* reference core_algorithms.h:100 */
cugraph_type_erased_device_array_view_t* cugraph_k_core_result_get_dst_vertices(cugraph_k_core_result_t* result);

/* reference core_algorithms.h:111 -- NULL for an unweighted graph */
cugraph_type_erased_device_array_view_t* cugraph_k_core_result_get_weights(cugraph_k_core_result_t* result);

/* reference core_algorithms.h:119 */
void cugraph_k_core_result_free(cugraph_k_core_result_t* result);

/*
 * reference core_algorithms.h:143-148.  Every vertex's core number in the underlying simple
 * graph: self-loop entries do not count and a neighbour stored several times counts once.  The
 * graph must be symmetric and not flagged multigraph (CUGRAPH_INVALID_INPUT otherwise); with
 * do_expensive_check a graph that has self-loops is CUGRAPH_INVALID_INPUT as well.  vertices is
 * a copy of the graph's vertex ids (ids without edges included, core number 0), core_numbers is
 * in the graph's edge type.  The numbers are the same on every run.  Single GPU only.
 */
cugraph_error_code_t cugraph_core_number(const cugraph_resource_handle_t* handle,
                                         cugraph_graph_t* graph,
                                         cugraph_k_core_degree_type_t degree_type,
                                         bool_t do_expensive_check,
                                         cugraph_core_result_t** result,
                                         cugraph_error_t** error);

/*
 * reference core_algorithms.h:167-174.  (The reference snapshot's cugraph::k_core fails with
 * "Not implemented"; this build implements what this header documents.)  The stored entries
 * (src, dst, weight) whose two endpoints both have a core number of at least k, both directions,
 * external ids, ordered by internal row and ascending within it.  Self-loop entries are never
 * returned and a neighbour stored several times is returned once.  core_result == NULL: the
 * core numbers are computed inside with degree_type; otherwise degree_type is ignored, k is
 * compared with the numbers as given, a graph vertex the result does not list counts as core 0,
 * and a listed id that is not in the graph is CUGRAPH_INVALID_INPUT with do_expensive_check and
 * skipped without it.
 */
cugraph_error_code_t cugraph_k_core(const cugraph_resource_handle_t* handle,
                                    cugraph_graph_t* graph,
                                    size_t k,
                                    cugraph_k_core_degree_type_t degree_type,
                                    const cugraph_core_result_t* core_result,
                                    bool_t do_expensive_check,
                                    cugraph_k_core_result_t** result,
                                    cugraph_error_t** error);

#ifdef __cplusplus
}
#endif
