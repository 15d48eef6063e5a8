// libcugraph_c algorithm entry points on the hot path (MI355X build):
// PageRank, personalised PageRank, BFS, SSSP, Louvain, connected components, triangle
// counting, core number / k-core, k-truss, induced subgraphs / ego nets and their result objects.
//
// Argument checks and error behaviour follow cpp/src/c_api/{pagerank.cpp:244-304,
// bfs.cpp:187-230, sssp.cpp:146-190, louvain.cpp:152-190} and the result getters
// cpp/src/c_api/{centrality_result.cpp, paths_result.cpp, louvain.cpp}.
#include "capi.hpp"

#include <cugraph_amd/ext.h>

using namespace cgx;

namespace cgx {
void run_pagerank(handle_t& h, graph_t& g, array_view_t const* pow_v, array_view_t const* pow_s,
                  array_view_t const* guess_v, array_view_t const* guess_s, array_view_t const* pers_v,
                  array_view_t const* pers_s, double alpha, double eps, size_t max_iter, bool expensive,
                  centrality_result_t& res);
void run_bfs(handle_t& h, graph_t& g, array_view_t* sources, bool direction_optimizing, size_t depth_limit,
             bool compute_predecessors, bool expensive, paths_result_t& res);
void run_sssp(handle_t& h, graph_t& g, size_t source, double cutoff, bool compute_predecessors, bool expensive,
              paths_result_t& res);
void run_louvain(handle_t& h, graph_t& g, size_t max_level, double resolution, bool expensive,
                 clustering_result_t& res);
void run_katz(handle_t& h, graph_t& g, array_view_t const* betas, double alpha, double beta, double eps,
              size_t max_iter, bool expensive, centrality_result_t& res);
void run_eigenvector(handle_t& h, graph_t& g, double eps, size_t max_iter, bool expensive, centrality_result_t& res);
void run_hits(handle_t& h, graph_t& g, double eps, size_t max_iter, array_view_t const* guess_v,
              array_view_t const* guess_s, bool normalize, bool expensive, hits_result_t& res);
void run_extract_paths(handle_t& h, graph_t& g, paths_result_t const& pr, array_view_t const* dests,
                       extract_paths_result_t& res);
void run_wcc(handle_t& h, graph_t& g, bool expensive, labeling_result_t& res);
void run_triangle_count(handle_t& h, graph_t& g, array_view_t const* start, bool expensive,
                        triangle_count_result_t& res);
void run_core_number(handle_t& h, graph_t& g, int delta, bool expensive, core_result_t& res);
void run_k_core(handle_t& h, graph_t& g, size_t k, int delta, core_result_t const* given, bool expensive,
                k_core_result_t& res);
void run_k_truss(handle_t& h, graph_t& g, size_t k, induced_subgraph_result_t& res);
void run_betweenness(handle_t& h, graph_t& g, array_view_t const* vertex_list, bool normalized, bool endpoints,
                     centrality_result_t* vres, edge_centrality_result_t* eres);
void mg_run_pagerank(handle_t& h, graph_t& g, array_view_t const* pow_v, array_view_t const* pow_s,
                     array_view_t const* guess_v, array_view_t const* guess_s, array_view_t const* pers_v,
                     array_view_t const* pers_s, double alpha, double eps, size_t max_iter, bool expensive,
                     centrality_result_t& res);
void mg_run_bfs(handle_t& h, graph_t& g, array_view_t* sources, bool direction_optimizing, size_t depth_limit,
                bool compute_predecessors, bool expensive, paths_result_t& res);
void mg_run_sssp(handle_t& h, graph_t& g, size_t source, double cutoff, bool compute_predecessors, bool expensive,
                 paths_result_t& res);
}  // namespace cgx

namespace {

template <typename R>
R* out_ptr(R** p)
{
  *p = nullptr;
  return nullptr;
}

cugraph_error_code_t pagerank_common(const cugraph_resource_handle_t* handle,
                                     cugraph_graph_t* graph,
                                     const cugraph_type_erased_device_array_view_t* pow_v,
                                     const cugraph_type_erased_device_array_view_t* pow_s,
                                     const cugraph_type_erased_device_array_view_t* guess_v,
                                     const cugraph_type_erased_device_array_view_t* guess_s,
                                     const cugraph_type_erased_device_array_view_t* pers_v,
                                     const cugraph_type_erased_device_array_view_t* pers_s,
                                     double alpha,
                                     double epsilon,
                                     size_t max_iterations,
                                     bool_t do_expensive_check,
                                     cugraph_centrality_result_t** result,
                                     cugraph_error_t** error)
{
  *result = nullptr;
  *error  = nullptr;
  return guarded(error, [&] {
    CGX_EXPECTS(handle != nullptr, CUGRAPH_INVALID_HANDLE, "invalid resource handle");
    CGX_INPUT(graph != nullptr, "Invalid input argument: graph is NULL");
    auto& g = *G(graph);
    // dtype checks of c_api/pagerank.cpp:260-290
    CGX_INPUT(!pow_v || AV(pow_v)->type == g.vertex_type,
              "vertex type of graph and precomputed_vertex_out_weight_vertices must match");
    CGX_INPUT(!pow_s || AV(pow_s)->type == g.weight_type,
              "weight type of graph and precomputed_vertex_out_weight_sums must match");
    CGX_INPUT(!guess_v || AV(guess_v)->type == g.vertex_type,
              "vertex type of graph and initial_guess_vertices must match");
    CGX_INPUT(!guess_s || AV(guess_s)->type == g.weight_type, "weight type of graph and initial_guess_values must match");
    CGX_INPUT(!pers_v || AV(pers_v)->type == g.vertex_type,
              "vertex type of graph and personalization_vertices must match");
    CGX_INPUT(!pers_s || AV(pers_s)->type == g.weight_type,
              "weight type of graph and personalization_values must match");
    auto res = std::make_unique<centrality_result_t>();
    auto f   = g.multi_gpu ? mg_run_pagerank : run_pagerank;
    f(*H(handle), g, pow_v ? AV(pow_v) : nullptr, pow_s ? AV(pow_s) : nullptr, guess_v ? AV(guess_v) : nullptr,
      guess_s ? AV(guess_s) : nullptr, pers_v ? AV(pers_v) : nullptr, pers_s ? AV(pers_s) : nullptr, alpha, epsilon,
      max_iterations, do_expensive_check == TRUE, *res);
    HIP_CHECK(hipStreamSynchronize(H(handle)->stream));
    *result = reinterpret_cast<cugraph_centrality_result_t*>(res.release());
  });
}

}  // namespace

// ============================================================== PageRank
extern "C" cugraph_error_code_t cugraph_pagerank(
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
  cugraph_error_t** error)
{
  return pagerank_common(handle, graph, precomputed_vertex_out_weight_vertices, precomputed_vertex_out_weight_sums,
                         initial_guess_vertices, initial_guess_values, nullptr, nullptr, alpha, epsilon,
                         max_iterations, do_expensive_check, result, error);
}

extern "C" cugraph_error_code_t cugraph_personalized_pagerank(
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
  cugraph_error_t** error)
{
  return pagerank_common(handle, graph, precomputed_vertex_out_weight_vertices, precomputed_vertex_out_weight_sums,
                         initial_guess_vertices, initial_guess_values, personalization_vertices,
                         personalization_values, alpha, epsilon, max_iterations, do_expensive_check, result, error);
}

extern "C" cugraph_type_erased_device_array_view_t* cugraph_centrality_result_get_vertices(
  cugraph_centrality_result_t* result)
{
  return new_view(reinterpret_cast<centrality_result_t*>(result)->vertices.get());
}

extern "C" cugraph_type_erased_device_array_view_t* cugraph_centrality_result_get_values(
  cugraph_centrality_result_t* result)
{
  return new_view(reinterpret_cast<centrality_result_t*>(result)->values.get());
}

extern "C" void cugraph_centrality_result_free(cugraph_centrality_result_t* result)
{
  delete reinterpret_cast<centrality_result_t*>(result);
}

// ============================================================== BFS / SSSP
extern "C" cugraph_error_code_t cugraph_bfs(const cugraph_resource_handle_t* handle,
                                           cugraph_graph_t* graph,
                                           cugraph_type_erased_device_array_view_t* sources,
                                           bool_t direction_optimizing,
                                           size_t depth_limit,
                                           bool_t compute_predecessors,
                                           bool_t do_expensive_check,
                                           cugraph_paths_result_t** result,
                                           cugraph_error_t** error)
{
  *result = nullptr;
  *error  = nullptr;
  return guarded(error, [&] {
    CGX_EXPECTS(handle != nullptr, CUGRAPH_INVALID_HANDLE, "invalid resource handle");
    CGX_INPUT(graph != nullptr && sources != nullptr, "Invalid input argument: graph/sources is NULL");
    auto& g = *G(graph);
    // c_api/bfs.cpp:196-200
    CGX_INPUT(AV(sources)->type == g.vertex_type, "vertex type of graph and sources must match");
    auto res = std::make_unique<paths_result_t>();
    auto f   = g.multi_gpu ? mg_run_bfs : run_bfs;
    f(*H(handle), g, AV(sources), direction_optimizing == TRUE, depth_limit, compute_predecessors == TRUE,
      do_expensive_check == TRUE, *res);
    HIP_CHECK(hipStreamSynchronize(H(handle)->stream));
    *result = reinterpret_cast<cugraph_paths_result_t*>(res.release());
  });
}

extern "C" cugraph_error_code_t cugraph_sssp(const cugraph_resource_handle_t* handle,
                                            cugraph_graph_t* graph,
                                            size_t source,
                                            double cutoff,
                                            bool_t compute_predecessors,
                                            bool_t do_expensive_check,
                                            cugraph_paths_result_t** result,
                                            cugraph_error_t** error)
{
  *result = nullptr;
  *error  = nullptr;
  return guarded(error, [&] {
    CGX_EXPECTS(handle != nullptr, CUGRAPH_INVALID_HANDLE, "invalid resource handle");
    CGX_INPUT(graph != nullptr, "Invalid input argument: graph is NULL");
    auto& g = *G(graph);
    auto res = std::make_unique<paths_result_t>();
    (g.multi_gpu ? mg_run_sssp : run_sssp)(*H(handle), g, source, cutoff, compute_predecessors == TRUE,
                                           do_expensive_check == TRUE, *res);
    HIP_CHECK(hipStreamSynchronize(H(handle)->stream));
    *result = reinterpret_cast<cugraph_paths_result_t*>(res.release());
  });
}

extern "C" cugraph_type_erased_device_array_view_t* cugraph_paths_result_get_vertices(cugraph_paths_result_t* result)
{
  return new_view(reinterpret_cast<paths_result_t*>(result)->vertices.get());
}

extern "C" cugraph_type_erased_device_array_view_t* cugraph_paths_result_get_distances(cugraph_paths_result_t* result)
{
  return new_view(reinterpret_cast<paths_result_t*>(result)->distances.get());
}

extern "C" cugraph_type_erased_device_array_view_t* cugraph_paths_result_get_predecessors(
  cugraph_paths_result_t* result)
{
  return new_view(reinterpret_cast<paths_result_t*>(result)->predecessors.get());
}

extern "C" void cugraph_paths_result_free(cugraph_paths_result_t* result)
{
  delete reinterpret_cast<paths_result_t*>(result);
}

// ============================================================== connected components
// (reference c_api/weakly_connected_components.cpp, strongly_connected_components.cpp, labeling_result.cpp)
extern "C" cugraph_error_code_t cugraph_weakly_connected_components(const cugraph_resource_handle_t* handle,
                                                                   cugraph_graph_t* graph,
                                                                   bool_t do_expensive_check,
                                                                   cugraph_labeling_result_t** result,
                                                                   cugraph_error_t** error)
{
  *result = nullptr;
  *error  = nullptr;
  return guarded(error, [&] {
    CGX_EXPECTS(handle != nullptr, CUGRAPH_INVALID_HANDLE, "invalid resource handle");
    CGX_INPUT(graph != nullptr, "Invalid input argument: graph is NULL");
    auto& g = *G(graph);
    // weakly_connected_components_impl.cuh:285-287
    CGX_INPUT(g.symmetric,
              "Invalid input argument: input graph should be symmetric for weakly connected components.");
    CGX_EXPECTS(!g.multi_gpu, CUGRAPH_NOT_IMPLEMENTED,
                "multi-GPU weakly connected components is not implemented in this build");
    auto res = std::make_unique<labeling_result_t>();
    run_wcc(*H(handle), g, do_expensive_check == TRUE, *res);
    HIP_CHECK(hipStreamSynchronize(H(handle)->stream));
    *result = reinterpret_cast<cugraph_labeling_result_t*>(res.release());
  });
}

extern "C" cugraph_error_code_t cugraph_strongly_connected_components(const cugraph_resource_handle_t* handle,
                                                                     cugraph_graph_t* graph,
                                                                     bool_t do_expensive_check,
                                                                     cugraph_labeling_result_t** result,
                                                                     cugraph_error_t** error)
{
  *result = nullptr;
  *error  = nullptr;
  return guarded(error, [&] {
    CGX_EXPECTS(handle != nullptr, CUGRAPH_INVALID_HANDLE, "invalid resource handle");
    CGX_INPUT(graph != nullptr, "Invalid input argument: graph is NULL");
    (void)do_expensive_check;
    // c_api/strongly_connected_components.cpp:69-70
    fail(CUGRAPH_NOT_IMPLEMENTED, "SCC Not currently implemented");
  });
}

extern "C" cugraph_type_erased_device_array_view_t* cugraph_labeling_result_get_vertices(
  cugraph_labeling_result_t* result)
{
  return new_view(reinterpret_cast<labeling_result_t*>(result)->vertices.get());
}

extern "C" cugraph_type_erased_device_array_view_t* cugraph_labeling_result_get_labels(
  cugraph_labeling_result_t* result)
{
  return new_view(reinterpret_cast<labeling_result_t*>(result)->labels.get());
}

extern "C" void cugraph_labeling_result_free(cugraph_labeling_result_t* result)
{
  delete reinterpret_cast<labeling_result_t*>(result);
}

// ============================================================== triangle counting
// (reference c_api/triangle_count.cpp, community/triangle_count_impl.cuh:152-188)
extern "C" cugraph_error_code_t cugraph_triangle_count(const cugraph_resource_handle_t* handle,
                                                      cugraph_graph_t* graph,
                                                      const cugraph_type_erased_device_array_view_t* start,
                                                      bool_t do_expensive_check,
                                                      cugraph_triangle_count_result_t** result,
                                                      cugraph_error_t** error)
{
  *result = nullptr;
  *error  = nullptr;
  return guarded(error, [&] {
    CGX_EXPECTS(handle != nullptr, CUGRAPH_INVALID_HANDLE, "invalid resource handle");
    CGX_INPUT(graph != nullptr, "Invalid input argument: graph is NULL");
    auto& g = *G(graph);
    CGX_EXPECTS(!g.multi_gpu, CUGRAPH_NOT_IMPLEMENTED, "multi-GPU triangle_count is not implemented in this build");
    CGX_INPUT(!start || AV(start)->type == g.vertex_type, "vertex type of graph and start must match");
    // triangle_count_impl.cuh:154-159
    CGX_INPUT(g.symmetric, "Invalid input arguments: triangle_count currently supports undirected graphs only.");
    CGX_INPUT(!g.multigraph, "Invalid input arguments: triangle_count currently does not support multi-graphs.");
    auto res = std::make_unique<triangle_count_result_t>();
    run_triangle_count(*H(handle), g, start ? AV(start) : nullptr, do_expensive_check == TRUE, *res);
    HIP_CHECK(hipStreamSynchronize(H(handle)->stream));
    *result = reinterpret_cast<cugraph_triangle_count_result_t*>(res.release());
  });
}

extern "C" cugraph_type_erased_device_array_view_t* cugraph_triangle_count_result_get_vertices(
  cugraph_triangle_count_result_t* result)
{
  return new_view(reinterpret_cast<triangle_count_result_t*>(result)->vertices.get());
}

extern "C" cugraph_type_erased_device_array_view_t* cugraph_triangle_count_result_get_counts(
  cugraph_triangle_count_result_t* result)
{
  return new_view(reinterpret_cast<triangle_count_result_t*>(result)->counts.get());
}

extern "C" void cugraph_triangle_count_result_free(cugraph_triangle_count_result_t* result)
{
  delete reinterpret_cast<triangle_count_result_t*>(result);
}

// ============================================================== core number / k-core
// (reference c_api/core_number.cpp, c_api/k_core.cpp, c_api/core_result.cpp, cores/core_number_impl.cuh:93-106)
namespace {

// the peeling step per neighbour: 1, or 2 for INOUT (core_number_impl.cuh:110-122)
int core_delta(cugraph_k_core_degree_type_t degree_type)
{
  CGX_INPUT(degree_type == K_CORE_DEGREE_TYPE_IN || degree_type == K_CORE_DEGREE_TYPE_OUT ||
              degree_type == K_CORE_DEGREE_TYPE_INOUT,
            "Invalid input argument: degree_type should be IN, OUT, or INOUT.");
  return degree_type == K_CORE_DEGREE_TYPE_INOUT ? 2 : 1;
}

void core_graph_checks(graph_t const& g, char const* multi_gpu_message)
{
  CGX_EXPECTS(!g.multi_gpu, CUGRAPH_NOT_IMPLEMENTED, multi_gpu_message);
  CGX_INPUT(g.symmetric, "Invalid input argument: core_number currently supports only undirected graphs.");
  CGX_INPUT(!g.multigraph, "Invalid input argument: core_number currently does not support multi-graphs.");
}

}  // namespace

extern "C" cugraph_error_code_t cugraph_core_number(const cugraph_resource_handle_t* handle,
                                                   cugraph_graph_t* graph,
                                                   cugraph_k_core_degree_type_t degree_type,
                                                   bool_t do_expensive_check,
                                                   cugraph_core_result_t** result,
                                                   cugraph_error_t** error)
{
  *result = nullptr;
  *error  = nullptr;
  return guarded(error, [&] {
    CGX_EXPECTS(handle != nullptr, CUGRAPH_INVALID_HANDLE, "invalid resource handle");
    CGX_INPUT(graph != nullptr, "Invalid input argument: graph is NULL");
    auto& g = *G(graph);
    core_graph_checks(g, "multi-GPU core_number is not implemented in this build");
    int const delta = core_delta(degree_type);
    auto res        = std::make_unique<core_result_t>();
    run_core_number(*H(handle), g, delta, do_expensive_check == TRUE, *res);
    HIP_CHECK(hipStreamSynchronize(H(handle)->stream));
    *result = reinterpret_cast<cugraph_core_result_t*>(res.release());
  });
}

extern "C" cugraph_error_code_t cugraph_k_core(const cugraph_resource_handle_t* handle,
                                              cugraph_graph_t* graph,
                                              size_t k,
                                              cugraph_k_core_degree_type_t degree_type,
                                              const cugraph_core_result_t* core_result,
                                              bool_t do_expensive_check,
                                              cugraph_k_core_result_t** result,
                                              cugraph_error_t** error)
{
  *result = nullptr;
  *error  = nullptr;
  return guarded(error, [&] {
    CGX_EXPECTS(handle != nullptr, CUGRAPH_INVALID_HANDLE, "invalid resource handle");
    CGX_INPUT(graph != nullptr, "Invalid input argument: graph is NULL");
    auto& g = *G(graph);
    core_graph_checks(g, "multi-GPU k_core is not implemented in this build");
    int const delta = core_result ? 1 : core_delta(degree_type);  // ignored with a given result
    auto res        = std::make_unique<k_core_result_t>();
    run_k_core(*H(handle), g, k, delta, reinterpret_cast<core_result_t const*>(core_result),
               do_expensive_check == TRUE, *res);
    HIP_CHECK(hipStreamSynchronize(H(handle)->stream));
    *result = reinterpret_cast<cugraph_k_core_result_t*>(res.release());
  });
}

// c_api/core_result.cpp: both views are copied into a result of its own
extern "C" cugraph_error_code_t cugraph_core_result_create(const cugraph_resource_handle_t* handle,
                                                          cugraph_type_erased_device_array_view_t* vertices,
                                                          cugraph_type_erased_device_array_view_t* core_numbers,
                                                          cugraph_core_result_t** core_result,
                                                          cugraph_error_t** error)
{
  *core_result = nullptr;
  *error       = nullptr;
  return guarded(error, [&] {
    CGX_EXPECTS(handle != nullptr, CUGRAPH_INVALID_HANDLE, "invalid resource handle");
    CGX_INPUT(vertices != nullptr && core_numbers != nullptr, "Invalid input argument: a core result array is NULL");
    hipStream_t s = H(handle)->stream;
    auto res      = std::make_unique<core_result_t>();
    auto copy     = [&](array_view_t const& v) {
      auto a = std::make_unique<device_array_t>(v.size, v.type, s);
      if (v.size) HIP_CHECK(hipMemcpyAsync(a->buf.data(), v.data, v.size * dtype_size(v.type), hipMemcpyDefault, s));
      return a;
    };
    res->vertices     = copy(*AV(vertices));
    res->core_numbers = copy(*AV(core_numbers));
    HIP_CHECK(hipStreamSynchronize(s));
    *core_result = reinterpret_cast<cugraph_core_result_t*>(res.release());
  });
}

extern "C" cugraph_type_erased_device_array_view_t* cugraph_core_result_get_vertices(cugraph_core_result_t* result)
{
  return new_view(reinterpret_cast<core_result_t*>(result)->vertices.get());
}

extern "C" cugraph_type_erased_device_array_view_t* cugraph_core_result_get_core_numbers(
  cugraph_core_result_t* result)
{
  return new_view(reinterpret_cast<core_result_t*>(result)->core_numbers.get());
}

extern "C" void cugraph_core_result_free(cugraph_core_result_t* result)
{
  delete reinterpret_cast<core_result_t*>(result);
}

extern "C" cugraph_type_erased_device_array_view_t* cugraph_k_core_result_get_src_vertices(
  cugraph_k_core_result_t* result)
{
  return new_view(reinterpret_cast<k_core_result_t*>(result)->src.get());
}

extern "C" cugraph_type_erased_device_array_view_t* cugraph_k_core_result_get_dst_vertices(
  cugraph_k_core_result_t* result)
{
  return new_view(reinterpret_cast<k_core_result_t*>(result)->dst.get());
}

extern "C" cugraph_type_erased_device_array_view_t* cugraph_k_core_result_get_weights(
  cugraph_k_core_result_t* result)
{
  auto* r = reinterpret_cast<k_core_result_t*>(result);
  return r->weights ? new_view(r->weights.get()) : nullptr;
}

extern "C" void cugraph_k_core_result_free(cugraph_k_core_result_t* result)
{
  delete reinterpret_cast<k_core_result_t*>(result);
}

// ============================================================== k-truss
// (the names of later releases' c_api/k_truss.cpp and c_api/induced_subgraph_result.cpp; k_truss.hip)
extern "C" cugraph_error_code_t cugraph_k_truss_subgraph(const cugraph_resource_handle_t* handle,
                                                        cugraph_graph_t* graph,
                                                        size_t k,
                                                        bool_t do_expensive_check,
                                                        cugraph_induced_subgraph_result_t** result,
                                                        cugraph_error_t** error)
{
  *result = nullptr;
  *error  = nullptr;
  (void)do_expensive_check;  // the build of the edge ids finds a missing reverse edge either way
  return guarded(error, [&] {
    CGX_EXPECTS(handle != nullptr, CUGRAPH_INVALID_HANDLE, "invalid resource handle");
    CGX_INPUT(graph != nullptr, "Invalid input argument: graph is NULL");
    auto& g = *G(graph);
    CGX_EXPECTS(!g.multi_gpu, CUGRAPH_NOT_IMPLEMENTED, "multi-GPU k_truss_subgraph is not implemented in this build");
    CGX_INPUT(g.symmetric, "Invalid input argument: k_truss_subgraph supports only undirected graphs.");
    auto res = std::make_unique<induced_subgraph_result_t>();
    run_k_truss(*H(handle), g, k, *res);
    HIP_CHECK(hipStreamSynchronize(H(handle)->stream));
    *result = reinterpret_cast<cugraph_induced_subgraph_result_t*>(res.release());
  });
}

// ============================================================== induced subgraphs and ego nets
// (the names of later releases' c_api/induced_subgraph.cpp and c_api/extract_ego.cpp; subgraph.hip)
extern "C" cugraph_error_code_t cugraph_extract_induced_subgraph(
  const cugraph_resource_handle_t* handle,
  cugraph_graph_t* graph,
  const cugraph_type_erased_device_array_view_t* subgraph_offsets,
  const cugraph_type_erased_device_array_view_t* subgraph_vertices,
  bool_t do_expensive_check,
  cugraph_induced_subgraph_result_t** result,
  cugraph_error_t** error)
{
  *result = nullptr;
  *error  = nullptr;
  (void)do_expensive_check;  // the lookup finds an unknown id and the sort a repeated one either way
  return guarded(error, [&] {
    CGX_EXPECTS(handle != nullptr, CUGRAPH_INVALID_HANDLE, "invalid resource handle");
    CGX_INPUT(graph != nullptr, "Invalid input argument: graph is NULL");
    auto& g = *G(graph);
    CGX_EXPECTS(!g.multi_gpu, CUGRAPH_NOT_IMPLEMENTED,
                "multi-GPU extract_induced_subgraph is not implemented in this build");
    CGX_INPUT(subgraph_offsets != nullptr && subgraph_vertices != nullptr,
              "Invalid input argument: subgraph_offsets or subgraph_vertices is NULL");
    auto const& off = *AV(subgraph_offsets);
    auto const& ver = *AV(subgraph_vertices);
    CGX_INPUT(off.type == INT64, "Invalid input argument: subgraph_offsets must be INT64");
    CGX_INPUT(off.size >= 1, "Invalid input argument: subgraph_offsets needs at least one entry");
    CGX_INPUT(ver.type == g.vertex_type, "vertex type of graph and subgraph_vertices must match");
    auto res = std::make_unique<induced_subgraph_result_t>();
    run_induced_subgraph(*H(handle), g, off, ver, *res);
    HIP_CHECK(hipStreamSynchronize(H(handle)->stream));
    *result = reinterpret_cast<cugraph_induced_subgraph_result_t*>(res.release());
  });
}

extern "C" cugraph_error_code_t cugraph_extract_ego(const cugraph_resource_handle_t* handle,
                                                   cugraph_graph_t* graph,
                                                   const cugraph_type_erased_device_array_view_t* source_vertices,
                                                   size_t radius,
                                                   bool_t do_expensive_check,
                                                   cugraph_induced_subgraph_result_t** result,
                                                   cugraph_error_t** error)
{
  *result = nullptr;
  *error  = nullptr;
  (void)do_expensive_check;  // the lookup finds an unknown id either way
  return guarded(error, [&] {
    CGX_EXPECTS(handle != nullptr, CUGRAPH_INVALID_HANDLE, "invalid resource handle");
    CGX_INPUT(graph != nullptr, "Invalid input argument: graph is NULL");
    auto& g = *G(graph);
    CGX_EXPECTS(!g.multi_gpu, CUGRAPH_NOT_IMPLEMENTED, "multi-GPU extract_ego is not implemented in this build");
    CGX_INPUT(source_vertices != nullptr, "Invalid input argument: source_vertices is NULL");
    auto const& src = *AV(source_vertices);
    CGX_INPUT(src.type == g.vertex_type, "vertex type of graph and source_vertices must match");
    auto res = std::make_unique<induced_subgraph_result_t>();
    run_extract_ego(*H(handle), g, src, radius, *res);
    HIP_CHECK(hipStreamSynchronize(H(handle)->stream));
    *result = reinterpret_cast<cugraph_induced_subgraph_result_t*>(res.release());
  });
}

extern "C" cugraph_type_erased_device_array_view_t* cugraph_induced_subgraph_get_sources(
  cugraph_induced_subgraph_result_t* result)
{
  return new_view(reinterpret_cast<induced_subgraph_result_t*>(result)->src.get());
}

extern "C" cugraph_type_erased_device_array_view_t* cugraph_induced_subgraph_get_destinations(
  cugraph_induced_subgraph_result_t* result)
{
  return new_view(reinterpret_cast<induced_subgraph_result_t*>(result)->dst.get());
}

extern "C" cugraph_type_erased_device_array_view_t* cugraph_induced_subgraph_get_edge_weights(
  cugraph_induced_subgraph_result_t* result)
{
  auto* r = reinterpret_cast<induced_subgraph_result_t*>(result);
  return r->weights ? new_view(r->weights.get()) : nullptr;
}

extern "C" cugraph_type_erased_device_array_view_t* cugraph_induced_subgraph_get_subgraph_offsets(
  cugraph_induced_subgraph_result_t* result)
{
  return new_view(reinterpret_cast<induced_subgraph_result_t*>(result)->offsets.get());
}

extern "C" void cugraph_induced_subgraph_result_free(cugraph_induced_subgraph_result_t* result)
{
  delete reinterpret_cast<induced_subgraph_result_t*>(result);
}

// ============================================================== Louvain
extern "C" cugraph_error_code_t cugraph_louvain(const cugraph_resource_handle_t* handle,
                                               cugraph_graph_t* graph,
                                               size_t max_level,
                                               double resolution,
                                               bool_t do_expensive_check,
                                               cugraph_heirarchical_clustering_result_t** result,
                                               cugraph_error_t** error)
{
  *result = nullptr;
  *error  = nullptr;
  return guarded(error, [&] {
    CGX_EXPECTS(handle != nullptr, CUGRAPH_INVALID_HANDLE, "invalid resource handle");
    CGX_INPUT(graph != nullptr, "Invalid input argument: graph is NULL");
    auto& g = *G(graph);
    auto res = std::make_unique<clustering_result_t>();
    run_louvain(*H(handle), g, max_level, resolution, do_expensive_check == TRUE, *res);
    HIP_CHECK(hipStreamSynchronize(H(handle)->stream));
    *result = reinterpret_cast<cugraph_heirarchical_clustering_result_t*>(res.release());
  });
}

extern "C" cugraph_type_erased_device_array_view_t* cugraph_heirarchical_clustering_result_get_vertices(
  cugraph_heirarchical_clustering_result_t* result)
{
  return new_view(reinterpret_cast<clustering_result_t*>(result)->vertices.get());
}

extern "C" size_t cugraph_amd_heirarchical_clustering_result_get_num_levels(
  cugraph_heirarchical_clustering_result_t* result)
{
  return reinterpret_cast<clustering_result_t*>(result)->levels.size();
}

extern "C" cugraph_type_erased_device_array_view_t* cugraph_amd_heirarchical_clustering_result_get_level(
  cugraph_heirarchical_clustering_result_t* result, size_t level)
{
  auto* r = reinterpret_cast<clustering_result_t*>(result);
  return level < r->levels.size() ? new_view(r->levels[level].get()) : nullptr;
}

extern "C" cugraph_type_erased_device_array_view_t* cugraph_heirarchical_clustering_result_get_clusters(
  cugraph_heirarchical_clustering_result_t* result)
{
  return new_view(reinterpret_cast<clustering_result_t*>(result)->clusters.get());
}

extern "C" double cugraph_heirarchical_clustering_result_get_modularity(
  cugraph_heirarchical_clustering_result_t* result)
{
  return reinterpret_cast<clustering_result_t*>(result)->modularity;
}

extern "C" void cugraph_heirarchical_clustering_result_free(cugraph_heirarchical_clustering_result_t* result)
{
  delete reinterpret_cast<clustering_result_t*>(result);
}

// ---------------------------------------------------------------- Katz / eigenvector / HITS
// (reference c_api/katz.cpp, eigenvector_centrality.cpp, hits.cpp)
extern "C" cugraph_error_code_t cugraph_katz_centrality(const cugraph_resource_handle_t* handle,
                                                       cugraph_graph_t* graph,
                                                       const cugraph_type_erased_device_array_view_t* betas,
                                                       double alpha,
                                                       double beta,
                                                       double epsilon,
                                                       size_t max_iterations,
                                                       bool_t do_expensive_check,
                                                       cugraph_centrality_result_t** result,
                                                       cugraph_error_t** error)
{
  *result = nullptr;
  *error  = nullptr;
  return guarded(error, [&] {
    CGX_EXPECTS(handle != nullptr, CUGRAPH_INVALID_HANDLE, "invalid resource handle");
    CGX_INPUT(graph != nullptr, "Invalid input argument: graph is NULL");
    auto& g = *G(graph);
    CGX_EXPECTS(!g.multi_gpu, CUGRAPH_NOT_IMPLEMENTED, "multi-GPU Katz centrality is not implemented in this build");
    auto res = std::make_unique<centrality_result_t>();
    run_katz(*H(handle), g, betas ? AV(betas) : nullptr, alpha, beta, epsilon, max_iterations,
             do_expensive_check == TRUE, *res);
    HIP_CHECK(hipStreamSynchronize(H(handle)->stream));
    *result = reinterpret_cast<cugraph_centrality_result_t*>(res.release());
  });
}

extern "C" cugraph_error_code_t cugraph_eigenvector_centrality(const cugraph_resource_handle_t* handle,
                                                              cugraph_graph_t* graph,
                                                              double epsilon,
                                                              size_t max_iterations,
                                                              bool_t do_expensive_check,
                                                              cugraph_centrality_result_t** result,
                                                              cugraph_error_t** error)
{
  *result = nullptr;
  *error  = nullptr;
  return guarded(error, [&] {
    CGX_EXPECTS(handle != nullptr, CUGRAPH_INVALID_HANDLE, "invalid resource handle");
    CGX_INPUT(graph != nullptr, "Invalid input argument: graph is NULL");
    auto& g = *G(graph);
    CGX_EXPECTS(!g.multi_gpu, CUGRAPH_NOT_IMPLEMENTED,
                "multi-GPU eigenvector centrality is not implemented in this build");
    auto res = std::make_unique<centrality_result_t>();
    run_eigenvector(*H(handle), g, epsilon, max_iterations, do_expensive_check == TRUE, *res);
    HIP_CHECK(hipStreamSynchronize(H(handle)->stream));
    *result = reinterpret_cast<cugraph_centrality_result_t*>(res.release());
  });
}

// ---------------------------------------------------------------- betweenness / edge betweenness
// (names and argument order of later cuGraph releases' centrality_algorithms.h; the scores and their scaling
// are centrality/betweenness_centrality.cu's; betweenness.hip)
namespace {

graph_t& betweenness_checks(const cugraph_resource_handle_t* handle, cugraph_graph_t* graph,
                            const cugraph_type_erased_device_array_view_t* vertex_list, char const* multi_gpu_message)
{
  CGX_EXPECTS(handle != nullptr, CUGRAPH_INVALID_HANDLE, "invalid resource handle");
  CGX_INPUT(graph != nullptr, "Invalid input argument: graph is NULL");
  auto& g = *G(graph);
  CGX_EXPECTS(!g.multi_gpu, CUGRAPH_NOT_IMPLEMENTED, multi_gpu_message);
  CGX_INPUT(!vertex_list || AV(vertex_list)->type == g.vertex_type, "vertex type of graph and vertex_list must match");
  return g;
}

}  // namespace

extern "C" cugraph_error_code_t cugraph_betweenness_centrality(const cugraph_resource_handle_t* handle,
                                                              cugraph_graph_t* graph,
                                                              const cugraph_type_erased_device_array_view_t* vertex_list,
                                                              bool_t normalized,
                                                              bool_t include_endpoints,
                                                              bool_t do_expensive_check,
                                                              cugraph_centrality_result_t** result,
                                                              cugraph_error_t** error)
{
  *result = nullptr;
  *error  = nullptr;
  return guarded(error, [&] {
    auto& g = betweenness_checks(handle, graph, vertex_list,
                                 "multi-GPU betweenness centrality is not implemented in this build");
    (void)do_expensive_check;  // the one check there is, that every source is in the graph, is always made
    auto res = std::make_unique<centrality_result_t>();
    run_betweenness(*H(handle), g, vertex_list ? AV(vertex_list) : nullptr, normalized == TRUE,
                    include_endpoints == TRUE, res.get(), nullptr);
    HIP_CHECK(hipStreamSynchronize(H(handle)->stream));
    *result = reinterpret_cast<cugraph_centrality_result_t*>(res.release());
  });
}

extern "C" cugraph_error_code_t cugraph_edge_betweenness_centrality(
  const cugraph_resource_handle_t* handle,
  cugraph_graph_t* graph,
  const cugraph_type_erased_device_array_view_t* vertex_list,
  bool_t normalized,
  bool_t do_expensive_check,
  cugraph_edge_centrality_result_t** result,
  cugraph_error_t** error)
{
  *result = nullptr;
  *error  = nullptr;
  return guarded(error, [&] {
    auto& g = betweenness_checks(handle, graph, vertex_list,
                                 "multi-GPU betweenness centrality (edge scores) is not implemented in this build");
    (void)do_expensive_check;
    auto res = std::make_unique<edge_centrality_result_t>();
    run_betweenness(*H(handle), g, vertex_list ? AV(vertex_list) : nullptr, normalized == TRUE, false, nullptr,
                    res.get());
    HIP_CHECK(hipStreamSynchronize(H(handle)->stream));
    *result = reinterpret_cast<cugraph_edge_centrality_result_t*>(res.release());
  });
}

extern "C" cugraph_type_erased_device_array_view_t* cugraph_edge_centrality_result_get_src_vertices(
  cugraph_edge_centrality_result_t* result)
{
  return new_view(reinterpret_cast<edge_centrality_result_t*>(result)->src.get());
}

extern "C" cugraph_type_erased_device_array_view_t* cugraph_edge_centrality_result_get_dst_vertices(
  cugraph_edge_centrality_result_t* result)
{
  return new_view(reinterpret_cast<edge_centrality_result_t*>(result)->dst.get());
}

extern "C" cugraph_type_erased_device_array_view_t* cugraph_edge_centrality_result_get_values(
  cugraph_edge_centrality_result_t* result)
{
  return new_view(reinterpret_cast<edge_centrality_result_t*>(result)->values.get());
}

extern "C" void cugraph_edge_centrality_result_free(cugraph_edge_centrality_result_t* result)
{
  delete reinterpret_cast<edge_centrality_result_t*>(result);
}

extern "C" cugraph_error_code_t cugraph_hits(const cugraph_resource_handle_t* handle,
                                            cugraph_graph_t* graph,
                                            double epsilon,
                                            size_t max_iterations,
                                            const cugraph_type_erased_device_array_view_t* initial_hubs_guess_vertices,
                                            const cugraph_type_erased_device_array_view_t* initial_hubs_guess_values,
                                            bool_t normalize,
                                            bool_t do_expensive_check,
                                            cugraph_hits_result_t** result,
                                            cugraph_error_t** error)
{
  *result = nullptr;
  *error  = nullptr;
  return guarded(error, [&] {
    CGX_EXPECTS(handle != nullptr, CUGRAPH_INVALID_HANDLE, "invalid resource handle");
    CGX_INPUT(graph != nullptr, "Invalid input argument: graph is NULL");
    CGX_INPUT((initial_hubs_guess_vertices == nullptr) == (initial_hubs_guess_values == nullptr),
              "Invalid input argument: initial hubs guess vertices and values must be given together");
    auto& g = *G(graph);
    CGX_EXPECTS(!g.multi_gpu, CUGRAPH_NOT_IMPLEMENTED, "multi-GPU HITS is not implemented in this build");
    auto res = std::make_unique<hits_result_t>();
    run_hits(*H(handle), g, epsilon, max_iterations,
             initial_hubs_guess_vertices ? AV(initial_hubs_guess_vertices) : nullptr,
             initial_hubs_guess_values ? AV(initial_hubs_guess_values) : nullptr, normalize == TRUE,
             do_expensive_check == TRUE, *res);
    HIP_CHECK(hipStreamSynchronize(H(handle)->stream));
    *result = reinterpret_cast<cugraph_hits_result_t*>(res.release());
  });
}

extern "C" cugraph_type_erased_device_array_view_t* cugraph_hits_result_get_vertices(cugraph_hits_result_t* result)
{
  return new_view(reinterpret_cast<hits_result_t*>(result)->vertices.get());
}
extern "C" cugraph_type_erased_device_array_view_t* cugraph_hits_result_get_hubs(cugraph_hits_result_t* result)
{
  return new_view(reinterpret_cast<hits_result_t*>(result)->hubs.get());
}
extern "C" cugraph_type_erased_device_array_view_t* cugraph_hits_result_get_authorities(cugraph_hits_result_t* result)
{
  return new_view(reinterpret_cast<hits_result_t*>(result)->authorities.get());
}
extern "C" double cugraph_hits_result_get_hub_score_differences(cugraph_hits_result_t* result)
{
  return reinterpret_cast<hits_result_t*>(result)->hub_score_differences;
}
extern "C" size_t cugraph_hits_result_get_number_of_iterations(cugraph_hits_result_t* result)
{
  return reinterpret_cast<hits_result_t*>(result)->number_of_iterations;
}
extern "C" void cugraph_hits_result_free(cugraph_hits_result_t* result)
{
  delete reinterpret_cast<hits_result_t*>(result);
}

// ---------------------------------------------------------------- extract paths (c_api/extract_paths.cpp)
extern "C" cugraph_error_code_t cugraph_extract_paths(const cugraph_resource_handle_t* handle,
                                                     cugraph_graph_t* graph,
                                                     const cugraph_type_erased_device_array_view_t* sources,
                                                     const cugraph_paths_result_t* paths_result,
                                                     const cugraph_type_erased_device_array_view_t* destinations,
                                                     cugraph_extract_paths_result_t** result,
                                                     cugraph_error_t** error)
{
  *result = nullptr;
  *error  = nullptr;
  return guarded(error, [&] {
    CGX_EXPECTS(handle != nullptr, CUGRAPH_INVALID_HANDLE, "invalid resource handle");
    CGX_INPUT(graph != nullptr && paths_result != nullptr && destinations != nullptr,
              "Invalid input argument: graph, paths result and destinations must be given");
    (void)sources;
    auto& g = *G(graph);
    CGX_EXPECTS(!g.multi_gpu, CUGRAPH_NOT_IMPLEMENTED, "multi-GPU extract_paths is not implemented in this build");
    auto res = std::make_unique<extract_paths_result_t>();
    run_extract_paths(*H(handle), g, *reinterpret_cast<paths_result_t const*>(paths_result), AV(destinations), *res);
    *result = reinterpret_cast<cugraph_extract_paths_result_t*>(res.release());
  });
}

extern "C" size_t cugraph_extract_paths_result_get_max_path_length(cugraph_extract_paths_result_t* result)
{
  return reinterpret_cast<extract_paths_result_t*>(result)->max_path_length;
}

extern "C" cugraph_type_erased_device_array_view_t* cugraph_extract_paths_result_get_paths(
  cugraph_extract_paths_result_t* result)
{
  return new_view(reinterpret_cast<extract_paths_result_t*>(result)->paths.get());
}

extern "C" void cugraph_extract_paths_result_free(cugraph_extract_paths_result_t* result)
{
  delete reinterpret_cast<extract_paths_result_t*>(result);
}
