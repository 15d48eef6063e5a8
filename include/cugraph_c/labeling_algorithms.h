/*
 * libcugraph_c labeling entry points -- MI355X build.
 * ABI-compatible with the reference cpp/include/cugraph_c/labeling_algorithms.h:35-102.
 */
#pragma once
#include <cugraph_c/array.h>
#include <cugraph_c/error.h>
#include <cugraph_c/graph.h>
#include <cugraph_c/resource_handle.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct { int32_t align_; } cugraph_labeling_result_t;

/* reference labeling_algorithms.h:45 -- the graph's vertex ids (its number map) */
cugraph_type_erased_device_array_view_t* cugraph_labeling_result_get_vertices(
  cugraph_labeling_result_t* result);

/* reference labeling_algorithms.h:54 -- labels[i] belongs to vertices[i]; vertex type */
cugraph_type_erased_device_array_view_t* cugraph_labeling_result_get_labels(
  cugraph_labeling_result_t* result);

/* reference labeling_algorithms.h:62 */
void cugraph_labeling_result_free(cugraph_labeling_result_t* result);

/*
 * reference labeling_algorithms.h:78-82 (implementation c_api/weakly_connected_components.cpp,
 * components/weakly_connected_components_impl.cuh).  The graph must be symmetric.
 * The reference leaves the label values arbitrary; this build fixes them: the label of
 * a vertex is the smallest internal id of its component, so label L names the vertex at
 * position L of the result's vertices, and the labels are the same bits on every run.
 * A vertex without edges is its own component.  Single GPU only.
 */
cugraph_error_code_t cugraph_weakly_connected_components(const cugraph_resource_handle_t* handle,
                                                         cugraph_graph_t* graph,
                                                         bool_t do_expensive_check,
                                                         cugraph_labeling_result_t** result,
                                                         cugraph_error_t** error);

/*
 * reference labeling_algorithms.h:98-102.  Checks its arguments and returns
 * CUGRAPH_NOT_IMPLEMENTED, as the reference does (c_api/strongly_connected_components.cpp:69).
 */
cugraph_error_code_t cugraph_strongly_connected_components(const cugraph_resource_handle_t* handle,
                                                           cugraph_graph_t* graph,
                                                           bool_t do_expensive_check,
                                                           cugraph_labeling_result_t** result,
                                                           cugraph_error_t** error);

#ifdef __cplusplus
}
#endif
