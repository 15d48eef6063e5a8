// libcugraph_c sampling entry points (MI355X build): uniform neighbour sampling, uniform and biased random
// walks, the node2vec stubs and both result objects.
//
// Argument checks follow cpp/src/c_api/uniform_neighbor_sampling.cpp:60-200 and c_api/random_walks.cpp;
// what is computed is specified in include/cugraph_c/sampling_algorithms.h (kernels: sampling.hip,
// random_walks.hip, the draw: sample.hpp).
#include "capi.hpp"

using namespace cgx;

namespace cgx {
void run_uniform_neighbor_sample(handle_t& h, graph_t& g, array_view_t const& start, int32_t const* fan_out,
                                 size_t hops, bool with_replacement, sample_result_t& res);
void run_random_walks(handle_t& h, graph_t& g, array_view_t const& start, size_t max_length, bool biased,
                      random_walk_result_t& res);
}  // namespace cgx

namespace {

std::unique_ptr<device_array_t> copy_of(array_view_t const& v, hipStream_t s)
{
  auto a = std::make_unique<device_array_t>(v.size, v.type, s);
  if (v.size) HIP_CHECK(hipMemcpyAsync(a->buf.data(), v.data, v.size * dtype_size(v.type), hipMemcpyDefault, s));
  return a;
}

cugraph_type_erased_device_array_view_t* view_or_null(std::unique_ptr<device_array_t> const& a)
{
  return a ? new_view(a.get()) : nullptr;
}

cugraph_error_code_t random_walks(char const* name, bool biased, const cugraph_resource_handle_t* handle,
                                  cugraph_graph_t* graph,
                                  const cugraph_type_erased_device_array_view_t* start_vertices, size_t max_length,
                                  cugraph_random_walk_result_t** result, cugraph_error_t** error)
{
  *result = nullptr;
  *error  = nullptr;
  return guarded(error, [&] {
    std::string const n(name);
    CGX_EXPECTS(handle != nullptr, CUGRAPH_INVALID_HANDLE, "invalid resource handle");
    CGX_INPUT(graph != nullptr, "Invalid input argument: graph is NULL");
    CGX_INPUT(start_vertices != nullptr, "Invalid input argument: start_vertices is NULL");
    auto& g = *G(graph);
    CGX_EXPECTS(!g.multi_gpu, CUGRAPH_NOT_IMPLEMENTED, "multi-GPU " + n + " is not implemented in this build");
    CGX_INPUT(AV(start_vertices)->type == g.vertex_type, "vertex type of graph and start_vertices must match");
    CGX_INPUT(!biased || g.weighted, "Invalid input argument: biased random walks need a weighted graph");
    auto res = std::make_unique<random_walk_result_t>();
    run_random_walks(*H(handle), g, *AV(start_vertices), max_length, biased, *res);
    HIP_CHECK(hipStreamSynchronize(H(handle)->stream));
    *result = reinterpret_cast<cugraph_random_walk_result_t*>(res.release());
  });
}

}  // namespace

// ============================================================== neighbour sampling
extern "C" cugraph_error_code_t cugraph_uniform_neighbor_sample(const cugraph_resource_handle_t* handle,
                                                               cugraph_graph_t* graph,
                                                               const cugraph_type_erased_device_array_view_t* start,
                                                               const cugraph_type_erased_host_array_view_t* fan_out,
                                                               bool_t with_replacement,
                                                               bool_t do_expensive_check,
                                                               cugraph_sample_result_t** result,
                                                               cugraph_error_t** error)
{
  *result = nullptr;
  *error  = nullptr;
  return guarded(error, [&] {
    CGX_EXPECTS(handle != nullptr, CUGRAPH_INVALID_HANDLE, "invalid resource handle");
    CGX_INPUT(graph != nullptr, "Invalid input argument: graph is NULL");
    CGX_INPUT(start != nullptr, "Invalid input argument: start is NULL");
    CGX_INPUT(fan_out != nullptr, "Invalid input argument: fan_out is NULL");
    auto& g = *G(graph);
    CGX_EXPECTS(!g.multi_gpu, CUGRAPH_NOT_IMPLEMENTED,
                "multi-GPU uniform_neighbor_sample is not implemented in this build");
    auto const* fo = reinterpret_cast<array_view_t const*>(fan_out);
    // c_api/uniform_neighbor_sampling.cpp:170-180
    CGX_INPUT(AV(start)->type == g.vertex_type, "vertex type of graph and start must match");
    CGX_INPUT(fo->type == INT32, "fan_out should be of type int");
    CGX_INPUT(fo->size > 0, "Invalid input argument: number of levels must be non-zero.");
    (void)do_expensive_check;  // the start ids are always checked
    auto res = std::make_unique<sample_result_t>();
    run_uniform_neighbor_sample(*H(handle), g, *AV(start), fo->as<int32_t>(), fo->size, with_replacement == TRUE,
                                *res);
    HIP_CHECK(hipStreamSynchronize(H(handle)->stream));
    *result = reinterpret_cast<cugraph_sample_result_t*>(res.release());
  });
}

extern "C" cugraph_type_erased_device_array_view_t* cugraph_sample_result_get_sources(
  const cugraph_sample_result_t* result)
{
  return view_or_null(reinterpret_cast<sample_result_t const*>(result)->src);
}

extern "C" cugraph_type_erased_device_array_view_t* cugraph_sample_result_get_destinations(
  const cugraph_sample_result_t* result)
{
  return view_or_null(reinterpret_cast<sample_result_t const*>(result)->dst);
}

// never set on this path by the reference either (its getter dereferences null there)
extern "C" cugraph_type_erased_device_array_view_t* cugraph_sample_result_get_start_labels(
  const cugraph_sample_result_t*)
{
  return nullptr;
}

extern "C" cugraph_type_erased_device_array_view_t* cugraph_sample_result_get_index(
  const cugraph_sample_result_t* result)
{
  return view_or_null(reinterpret_cast<sample_result_t const*>(result)->index);
}

extern "C" cugraph_type_erased_host_array_view_t* cugraph_sample_result_get_counts(
  const cugraph_sample_result_t* result)
{
  auto const& c = reinterpret_cast<sample_result_t const*>(result)->given_counts;
  if (!c) return nullptr;
  return reinterpret_cast<cugraph_type_erased_host_array_view_t*>(
    new array_view_t{c->data.data(), c->size, c->data.size(), c->type});
}

extern "C" cugraph_type_erased_device_array_view_t* cugraph_amd_sample_result_get_counts(
  const cugraph_sample_result_t* result)
{
  return view_or_null(reinterpret_cast<sample_result_t const*>(result)->counts);
}

extern "C" void cugraph_sample_result_free(cugraph_sample_result_t* result)
{
  delete reinterpret_cast<sample_result_t*>(result);
}

extern "C" cugraph_error_code_t cugraph_test_sample_result_create(
  const cugraph_resource_handle_t* handle,
  const cugraph_type_erased_device_array_view_t* srcs,
  const cugraph_type_erased_device_array_view_t* dsts,
  const cugraph_type_erased_device_array_view_t* weights,
  const cugraph_type_erased_device_array_view_t* counts,
  cugraph_sample_result_t** result,
  cugraph_error_t** error)
{
  *result = nullptr;
  *error  = nullptr;
  return guarded(error, [&] {
    CGX_EXPECTS(handle != nullptr, CUGRAPH_INVALID_HANDLE, "invalid resource handle");
    CGX_INPUT(srcs && dsts && weights && counts, "Invalid input argument: an array is NULL");
    hipStream_t s = H(handle)->stream;
    auto res      = std::make_unique<sample_result_t>();
    res->src      = copy_of(*AV(srcs), s);
    res->dst      = copy_of(*AV(dsts), s);
    res->index    = copy_of(*AV(weights), s);
    res->counts   = copy_of(*AV(counts), s);
    auto given    = std::make_unique<host_array_t>();
    given->size   = AV(counts)->size;
    given->type   = AV(counts)->type;
    given->data.resize(given->size * dtype_size(given->type));
    if (given->size)
      HIP_CHECK(hipMemcpyAsync(given->data.data(), AV(counts)->data, given->data.size(), hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    res->given_counts = std::move(given);
    *result           = reinterpret_cast<cugraph_sample_result_t*>(res.release());
  });
}

// ============================================================== random walks
extern "C" cugraph_error_code_t cugraph_uniform_random_walks(
  const cugraph_resource_handle_t* handle,
  cugraph_graph_t* graph,
  const cugraph_type_erased_device_array_view_t* start_vertices,
  size_t max_length,
  cugraph_random_walk_result_t** result,
  cugraph_error_t** error)
{
  return random_walks("uniform_random_walks", false, handle, graph, start_vertices, max_length, result, error);
}

extern "C" cugraph_error_code_t cugraph_biased_random_walks(
  const cugraph_resource_handle_t* handle,
  cugraph_graph_t* graph,
  const cugraph_type_erased_device_array_view_t* start_vertices,
  size_t max_length,
  cugraph_random_walk_result_t** result,
  cugraph_error_t** error)
{
  return random_walks("biased_random_walks", true, handle, graph, start_vertices, max_length, result, error);
}

extern "C" cugraph_error_code_t cugraph_node2vec_random_walks(
  const cugraph_resource_handle_t* handle,
  cugraph_graph_t* graph,
  const cugraph_type_erased_device_array_view_t* start_vertices,
  size_t max_length,
  double p,
  double q,
  cugraph_random_walk_result_t** result,
  cugraph_error_t** error)
{
  *result = nullptr;
  *error  = nullptr;
  return guarded(error, [&] {
    CGX_EXPECTS(handle != nullptr, CUGRAPH_INVALID_HANDLE, "invalid resource handle");
    CGX_INPUT(graph != nullptr, "Invalid input argument: graph is NULL");
    (void)start_vertices, (void)max_length, (void)p, (void)q;
    // random_walks_impl.cuh:139-148: the reference's node2vec selector fails the same way
    fail(CUGRAPH_NOT_IMPLEMENTED, "node2vec sampling is not implemented in this build");
  });
}

extern "C" cugraph_error_code_t cugraph_node2vec(const cugraph_resource_handle_t* handle,
                                                cugraph_graph_t* graph,
                                                const cugraph_type_erased_device_array_view_t* sources,
                                                size_t max_depth,
                                                bool_t compress_result,
                                                double p,
                                                double q,
                                                cugraph_random_walk_result_t** result,
                                                cugraph_error_t** error)
{
  *result = nullptr;
  *error  = nullptr;
  return guarded(error, [&] {
    CGX_EXPECTS(handle != nullptr, CUGRAPH_INVALID_HANDLE, "invalid resource handle");
    CGX_INPUT(graph != nullptr, "Invalid input argument: graph is NULL");
    (void)sources, (void)max_depth, (void)compress_result, (void)p, (void)q;
    fail(CUGRAPH_NOT_IMPLEMENTED, "node2vec sampling is not implemented in this build");
  });
}

extern "C" size_t cugraph_random_walk_result_get_max_path_length(cugraph_random_walk_result_t* result)
{
  return reinterpret_cast<random_walk_result_t*>(result)->max_length;
}

extern "C" cugraph_type_erased_device_array_view_t* cugraph_random_walk_result_get_paths(
  cugraph_random_walk_result_t* result)
{
  return view_or_null(reinterpret_cast<random_walk_result_t*>(result)->paths);
}

extern "C" cugraph_type_erased_device_array_view_t* cugraph_random_walk_result_get_weights(
  cugraph_random_walk_result_t* result)
{
  return view_or_null(reinterpret_cast<random_walk_result_t*>(result)->weights);
}

// the padded result has no sizes (the legacy compressed node2vec output is out of scope)
extern "C" cugraph_type_erased_device_array_view_t* cugraph_random_walk_result_get_path_sizes(
  cugraph_random_walk_result_t*)
{
  return nullptr;
}

extern "C" void cugraph_random_walk_result_free(cugraph_random_walk_result_t* result)
{
  delete reinterpret_cast<random_walk_result_t*>(result);
}
