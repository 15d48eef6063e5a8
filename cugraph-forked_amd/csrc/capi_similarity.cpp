// libcugraph_c link prediction entry points (MI355X build): vertex pairs, two-hop neighbours and
// the Jaccard / Sorensen / overlap coefficients with their result object.
//
// Argument checks and messages follow cpp/src/c_api/graph_functions.cpp:60-100 and
// c_api/similarity.cpp:60-150; the reference snapshot stops at CUGRAPH_FAIL("Not implemented")
// in both, so what is computed is what the headers, similarity_impl.cuh and the legacy kernels
// specify (include/cugraph_c/similarity_algorithms.h, graph_functions.h).
#include "capi.hpp"

using namespace cgx;

namespace cgx {
void run_similarity(handle_t& h, graph_t& g, array_view_t const& first, array_view_t const& second, int measure,
                    bool expensive, similarity_result_t& res);
void run_two_hop(handle_t& h, graph_t& g, array_view_t const* start, vertex_pairs_t& res);
}  // namespace cgx

namespace {

std::unique_ptr<device_array_t> copy_of(array_view_t const& v, hipStream_t s)
{
  auto a = std::make_unique<device_array_t>(v.size, v.type, s);
  if (v.size) HIP_CHECK(hipMemcpyAsync(a->buf.data(), v.data, v.size * dtype_size(v.type), hipMemcpyDefault, s));
  return a;
}

// measure: 0 Jaccard, 1 Sorensen, 2 overlap (similarity.hip k_sim_finish)
cugraph_error_code_t similarity(char const* name, int measure, const cugraph_resource_handle_t* handle,
                                cugraph_graph_t* graph, const cugraph_vertex_pairs_t* vertex_pairs, bool_t use_weight,
                                bool_t do_expensive_check, cugraph_similarity_result_t** result,
                                cugraph_error_t** error)
{
  *result = nullptr;
  *error  = nullptr;
  return guarded(error, [&] {
    std::string const n(name);
    CGX_EXPECTS(handle != nullptr, CUGRAPH_INVALID_HANDLE, "invalid resource handle");
    CGX_INPUT(graph != nullptr, "Invalid input argument: graph is NULL");
    CGX_INPUT(vertex_pairs != nullptr, "Invalid input argument: vertex_pairs is NULL");
    auto& g = *G(graph);
    CGX_EXPECTS(!g.multi_gpu, CUGRAPH_NOT_IMPLEMENTED, "multi-GPU " + n + " is not implemented in this build");
    CGX_EXPECTS(use_weight != TRUE, CUGRAPH_NOT_IMPLEMENTED,
                "weighted similarity computations are not supported in this release");
    CGX_INPUT(g.symmetric, "Invalid input arguments: " + n + " currently supports undirected graphs only.");
    CGX_INPUT(!g.multigraph, "Invalid input arguments: " + n + " currently does not support multi-graphs.");
    auto const& vp = *reinterpret_cast<vertex_pairs_t const*>(vertex_pairs);
    CGX_INPUT(vp.first->type == g.vertex_type && vp.second->type == g.vertex_type,
              "Invalid input arguments: vertex type of graph and vertex_pairs must match");
    auto res = std::make_unique<similarity_result_t>();
    run_similarity(*H(handle), g, vp.first->view(), vp.second->view(), measure, do_expensive_check == TRUE, *res);
    HIP_CHECK(hipStreamSynchronize(H(handle)->stream));
    *result = reinterpret_cast<cugraph_similarity_result_t*>(res.release());
  });
}

}  // namespace

// ============================================================== vertex pairs
extern "C" cugraph_error_code_t cugraph_create_vertex_pairs(const cugraph_resource_handle_t* handle,
                                                            cugraph_graph_t* graph,
                                                            const cugraph_type_erased_device_array_view_t* first,
                                                            const cugraph_type_erased_device_array_view_t* second,
                                                            cugraph_vertex_pairs_t** vertex_pairs,
                                                            cugraph_error_t** error)
{
  *vertex_pairs = nullptr;
  *error        = nullptr;
  return guarded(error, [&] {
    CGX_EXPECTS(handle != nullptr, CUGRAPH_INVALID_HANDLE, "invalid resource handle");
    CGX_INPUT(graph != nullptr, "Invalid input argument: graph is NULL");
    CGX_INPUT(first != nullptr && second != nullptr, "Invalid input argument: a vertex pair array is NULL");
    auto& g = *G(graph);
    // c_api/graph_functions.cpp:75-82
    CGX_INPUT(AV(first)->type == g.vertex_type, "vertex type of graph and first must match");
    CGX_INPUT(AV(second)->type == g.vertex_type, "vertex type of graph and second must match");
    CGX_INPUT(AV(first)->size == AV(second)->size, "Invalid input arguments: first and second differ in length");
    hipStream_t s = H(handle)->stream;
    auto res      = std::make_unique<vertex_pairs_t>();
    res->first    = copy_of(*AV(first), s);
    res->second   = copy_of(*AV(second), s);
    HIP_CHECK(hipStreamSynchronize(s));
    *vertex_pairs = reinterpret_cast<cugraph_vertex_pairs_t*>(res.release());
  });
}

extern "C" cugraph_type_erased_device_array_view_t* cugraph_vertex_pairs_get_first(
  cugraph_vertex_pairs_t* vertex_pairs)
{
  return new_view(reinterpret_cast<vertex_pairs_t*>(vertex_pairs)->first.get());
}

extern "C" cugraph_type_erased_device_array_view_t* cugraph_vertex_pairs_get_second(
  cugraph_vertex_pairs_t* vertex_pairs)
{
  return new_view(reinterpret_cast<vertex_pairs_t*>(vertex_pairs)->second.get());
}

extern "C" void cugraph_vertex_pairs_free(cugraph_vertex_pairs_t* vertex_pairs)
{
  delete reinterpret_cast<vertex_pairs_t*>(vertex_pairs);
}

// ============================================================== two-hop neighbours
extern "C" cugraph_error_code_t cugraph_two_hop_neighbors(const cugraph_resource_handle_t* handle,
                                                          const cugraph_graph_t* graph,
                                                          const cugraph_type_erased_device_array_view_t* start_vertices,
                                                          cugraph_vertex_pairs_t** result,
                                                          cugraph_error_t** error)
{
  *result = nullptr;
  *error  = nullptr;
  return guarded(error, [&] {
    CGX_EXPECTS(handle != nullptr, CUGRAPH_INVALID_HANDLE, "invalid resource handle");
    CGX_INPUT(graph != nullptr, "Invalid input argument: graph is NULL");
    auto& g = *const_cast<graph_t*>(G(graph));  // the out-edge adjacency is built on first use
    CGX_EXPECTS(!g.multi_gpu, CUGRAPH_NOT_IMPLEMENTED,
                "multi-GPU two_hop_neighbors is not implemented in this build");
    CGX_INPUT(start_vertices == nullptr || AV(start_vertices)->type == g.vertex_type,
              "vertex type of graph and start_vertices must match");
    auto res = std::make_unique<vertex_pairs_t>();
    run_two_hop(*H(handle), g, start_vertices ? AV(start_vertices) : nullptr, *res);
    HIP_CHECK(hipStreamSynchronize(H(handle)->stream));
    *result = reinterpret_cast<cugraph_vertex_pairs_t*>(res.release());
  });
}

// ============================================================== similarity
extern "C" cugraph_type_erased_device_array_view_t* cugraph_similarity_result_get_similarity(
  cugraph_similarity_result_t* result)
{
  return new_view(reinterpret_cast<similarity_result_t*>(result)->similarity.get());
}

extern "C" void cugraph_similarity_result_free(cugraph_similarity_result_t* result)
{
  delete reinterpret_cast<similarity_result_t*>(result);
}

extern "C" cugraph_error_code_t cugraph_jaccard_coefficients(const cugraph_resource_handle_t* handle,
                                                             cugraph_graph_t* graph,
                                                             const cugraph_vertex_pairs_t* vertex_pairs,
                                                             bool_t use_weight,
                                                             bool_t do_expensive_check,
                                                             cugraph_similarity_result_t** result,
                                                             cugraph_error_t** error)
{
  return similarity("jaccard", 0, handle, graph, vertex_pairs, use_weight, do_expensive_check, result, error);
}

extern "C" cugraph_error_code_t cugraph_sorensen_coefficients(const cugraph_resource_handle_t* handle,
                                                              cugraph_graph_t* graph,
                                                              const cugraph_vertex_pairs_t* vertex_pairs,
                                                              bool_t use_weight,
                                                              bool_t do_expensive_check,
                                                              cugraph_similarity_result_t** result,
                                                              cugraph_error_t** error)
{
  return similarity("sorensen", 1, handle, graph, vertex_pairs, use_weight, do_expensive_check, result, error);
}

extern "C" cugraph_error_code_t cugraph_overlap_coefficients(const cugraph_resource_handle_t* handle,
                                                             cugraph_graph_t* graph,
                                                             const cugraph_vertex_pairs_t* vertex_pairs,
                                                             bool_t use_weight,
                                                             bool_t do_expensive_check,
                                                             cugraph_similarity_result_t** result,
                                                             cugraph_error_t** error)
{
  return similarity("overlap", 2, handle, graph, vertex_pairs, use_weight, do_expensive_check, result, error);
}
