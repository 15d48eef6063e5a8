/*
 * Plain-C client of libcugraph_c's sampling entry points, compiled against the include/cugraph_c
 * headers only (no HIP, no C++), in the manner of similarity_test.c.  It runs the two cases of the
 * reference's cpp/tests/c_api/uniform_neighbor_sample_test.c (tests/golden/sampling_vectors.json:
 * 6 vertices, 8 edges, int32 edge ids carried in the float32 weight array) and checks that every
 * returned edge carries its own id, then one uniform random walk, the getters that return NULL
 * and the node2vec stubs.
 *
 * Build: gcc -std=c99 -I include tests/c/sampling_test.c -L <lib> -lcugraph_c
 * Run:   ./sampling_test      (needs a GPU; exit status = number of failures)
 */
#include <cugraph_c/algorithms.h>
#include <cugraph_c/array.h>
#include <cugraph_c/graph.h>

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

static int g_failures = 0;

#define CHECK(cond, ...)                                                   \
  do {                                                                     \
    if (!(cond)) {                                                         \
      fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__);                 \
      fprintf(stderr, __VA_ARGS__);                                        \
      fprintf(stderr, "\n");                                               \
      ++g_failures;                                                        \
      return 1;                                                            \
    }                                                                      \
  } while (0)

#define CHECK_RC(rc, err, what)                                                          \
  CHECK((rc) == CUGRAPH_SUCCESS, "%s failed (%d): %s", what, (int)(rc),                   \
        (err) ? cugraph_error_message(err) : "(no message)")

#define NV 6
#define NE 8
static const int32_t SRC[NE] = {0, 1, 1, 2, 2, 2, 3, 4};
static const int32_t DST[NE] = {1, 3, 4, 0, 1, 3, 5, 5};

static cugraph_type_erased_device_array_t* to_device(const cugraph_resource_handle_t* h, const void* host,
                                                     size_t n, data_type_id_t t,
                                                     cugraph_type_erased_device_array_view_t** view)
{
  cugraph_type_erased_device_array_t* arr = NULL;
  cugraph_error_t* err                    = NULL;
  if (cugraph_type_erased_device_array_create(h, n, t, &arr, &err) != CUGRAPH_SUCCESS) {
    cugraph_error_free(err);
    return NULL;
  }
  *view = cugraph_type_erased_device_array_view(arr);
  if (cugraph_type_erased_device_array_view_copy_from_host(h, *view, (const byte_t*)host, &err) !=
      CUGRAPH_SUCCESS) {
    cugraph_error_free(err);
    cugraph_type_erased_device_array_view_free(*view);
    cugraph_type_erased_device_array_free(arr);
    return NULL;
  }
  return arr;
}

typedef struct {
  cugraph_type_erased_device_array_t *src, *dst, *ids;
  cugraph_type_erased_device_array_view_t *src_v, *dst_v, *ids_v, *wgt_v;
  cugraph_graph_t* graph;
} test_graph_t;

static void free_graph(test_graph_t* g)
{
  if (g->graph) cugraph_sg_graph_free(g->graph);
  if (g->wgt_v) cugraph_type_erased_device_array_view_free(g->wgt_v);
  if (g->src_v) cugraph_type_erased_device_array_view_free(g->src_v);
  if (g->dst_v) cugraph_type_erased_device_array_view_free(g->dst_v);
  if (g->ids_v) cugraph_type_erased_device_array_view_free(g->ids_v);
  if (g->src) cugraph_type_erased_device_array_free(g->src);
  if (g->dst) cugraph_type_erased_device_array_free(g->dst);
  if (g->ids) cugraph_type_erased_device_array_free(g->ids);
  memset(g, 0, sizeof(*g));
}

/* the graph above with int32 edge ids seen as its float32 weights, not renumbered */
static cugraph_error_code_t make_graph(const cugraph_resource_handle_t* h, const int32_t* ids, test_graph_t* g,
                                       cugraph_error_t** err)
{
  memset(g, 0, sizeof(*g));
  *err                            = NULL;
  cugraph_graph_properties_t prop = {FALSE, FALSE};
  g->src                          = to_device(h, SRC, NE, INT32, &g->src_v);
  g->dst                          = to_device(h, DST, NE, INT32, &g->dst_v);
  g->ids                          = to_device(h, ids, NE, INT32, &g->ids_v);
  if (!g->src || !g->dst || !g->ids) return CUGRAPH_ALLOC_ERROR;
  cugraph_error_code_t rc = cugraph_type_erased_device_array_view_as_type(g->ids, FLOAT32, &g->wgt_v, err);
  if (rc != CUGRAPH_SUCCESS) return rc;
  return cugraph_sg_graph_create(h, &prop, g->src_v, g->dst_v, g->wgt_v, NULL, NULL, FALSE, FALSE, FALSE,
                                 &g->graph, err);
}

static int copy_back(const cugraph_resource_handle_t* h, cugraph_type_erased_device_array_view_t* v, void* out,
                     size_t n, data_type_id_t t)
{
  cugraph_error_t* err = NULL;
  CHECK(v != NULL, "view is NULL");
  CHECK(cugraph_type_erased_device_array_view_size(v) == n, "view size %zu, expected %zu",
        cugraph_type_erased_device_array_view_size(v), n);
  CHECK(cugraph_type_erased_device_array_view_type(v) == t, "view dtype");
  if (n) {
    cugraph_error_code_t rc = cugraph_type_erased_device_array_view_copy_to_host(h, (byte_t*)out, v, &err);
    CHECK_RC(rc, err, "copy to host");
  }
  cugraph_type_erased_device_array_view_free(v);
  return 0;
}

/* one sample call; every returned (source, destination) must be an edge and carry that edge's id.
 * exact > 0: the number of distinct edges the call must return */
static int run_sample(const int32_t* ids, const int32_t* start, size_t nstart, int32_t* fan_out, size_t hops,
                      size_t exact)
{
  cugraph_resource_handle_t* h = cugraph_create_resource_handle(NULL);
  CHECK(h != NULL, "resource handle");
  test_graph_t g;
  cugraph_error_t* err    = NULL;
  cugraph_error_code_t rc = make_graph(h, ids, &g, &err);
  CHECK_RC(rc, err, "sg_graph_create");
  cugraph_type_erased_device_array_view_t* start_v = NULL;
  cugraph_type_erased_device_array_t* start_d      = to_device(h, start, nstart, INT32, &start_v);
  CHECK(start_d != NULL, "start array");
  cugraph_type_erased_host_array_view_t* fan_v = cugraph_type_erased_host_array_view_create(fan_out, hops, INT32);
  cugraph_sample_result_t* res                 = NULL;
  rc = cugraph_uniform_neighbor_sample(h, g.graph, start_v, fan_v, TRUE, FALSE, &res, &err);
  CHECK_RC(rc, err, "cugraph_uniform_neighbor_sample");
  CHECK(cugraph_sample_result_get_start_labels(res) == NULL, "start labels are never set");
  CHECK(cugraph_sample_result_get_counts(res) == NULL, "counts are never set by a sample call");
  cugraph_type_erased_device_array_view_t* sv = cugraph_sample_result_get_sources(res);
  CHECK(sv != NULL, "sources");
  size_t n = cugraph_type_erased_device_array_view_size(sv);
  CHECK(n > 0 && n <= NE, "%zu edges returned", n);
  CHECK(exact == 0 || n == exact, "%zu edges returned, expected %zu", n, exact);
  int32_t s[NE], d[NE], id[NE];
  if (copy_back(h, sv, s, n, INT32)) return 1;
  if (copy_back(h, cugraph_sample_result_get_destinations(res), d, n, INT32)) return 1;
  if (copy_back(h, cugraph_sample_result_get_index(res), id, n, FLOAT32)) return 1;
  int32_t m[NV][NV];
  for (int i = 0; i < NV; ++i)
    for (int j = 0; j < NV; ++j) m[i][j] = -1;
  for (int e = 0; e < NE; ++e) m[SRC[e]][DST[e]] = ids[e];
  for (size_t i = 0; i < n; ++i) {
    CHECK(s[i] >= 0 && s[i] < NV && d[i] >= 0 && d[i] < NV, "edge %zu out of range", i);
    CHECK(m[s[i]][d[i]] == id[i], "edge (%d, %d) carries id %d, expected %d", s[i], d[i], id[i], m[s[i]][d[i]]);
  }
  cugraph_sample_result_free(res);
  cugraph_type_erased_host_array_view_free(fan_v);
  cugraph_type_erased_device_array_view_free(start_v);
  cugraph_type_erased_device_array_free(start_d);
  free_graph(&g);
  cugraph_free_resource_handle(h);
  return 0;
}

static int test_sample(void)
{
  const int32_t ids[NE]  = {1, 2, 3, 4, 5, 6, 7, 8};
  const int32_t start[2] = {2, 2};
  int32_t fan_out[2]     = {1, 2};
  return run_sample(ids, start, 2, fan_out, 2, 0);
}

static int test_sample_all_neighbors(void)
{
  const int32_t ids[NE]  = {0, 1, 2, 3, 4, 5, 6, 7};
  const int32_t start[1] = {2};
  int32_t fan_out[1]     = {-1};
  return run_sample(ids, start, 1, fan_out, 1, 3);
}

static int is_edge(int32_t a, int32_t b, const int32_t* ids, float w)
{
  for (int e = 0; e < NE; ++e)
    if (SRC[e] == a && DST[e] == b) {
      int32_t bits;
      memcpy(&bits, &w, sizeof(bits));
      return bits == ids[e];
    }
  return 0;
}

static int test_uniform_walk(void)
{
#define LEN 4
  const int32_t ids[NE]  = {1, 2, 3, 4, 5, 6, 7, 8};
  const int32_t start[3] = {2, 5, 0};
  cugraph_resource_handle_t* h = cugraph_create_resource_handle(NULL);
  CHECK(h != NULL, "resource handle");
  test_graph_t g;
  cugraph_error_t* err    = NULL;
  cugraph_error_code_t rc = make_graph(h, ids, &g, &err);
  CHECK_RC(rc, err, "sg_graph_create");
  cugraph_type_erased_device_array_view_t* start_v = NULL;
  cugraph_type_erased_device_array_t* start_d      = to_device(h, start, 3, INT32, &start_v);
  CHECK(start_d != NULL, "start array");
  cugraph_random_walk_result_t* res = NULL;
  rc = cugraph_uniform_random_walks(h, g.graph, start_v, LEN, &res, &err);
  CHECK_RC(rc, err, "cugraph_uniform_random_walks");
  CHECK(cugraph_random_walk_result_get_max_path_length(res) == LEN, "max path length");
  CHECK(cugraph_random_walk_result_get_path_sizes(res) == NULL, "path sizes are never set");
  int32_t paths[3 * (LEN + 1)];
  float w[3 * LEN];
  if (copy_back(h, cugraph_random_walk_result_get_paths(res), paths, 3 * (LEN + 1), INT32)) return 1;
  if (copy_back(h, cugraph_random_walk_result_get_weights(res), w, 3 * LEN, FLOAT32)) return 1;
  for (int i = 0; i < 3; ++i) {
    const int32_t* row = paths + i * (LEN + 1);
    CHECK(row[0] == start[i], "walk %d starts at %d", i, row[0]);
    int ended = 0;
    for (int k = 0; k < LEN; ++k) {
      if (row[k + 1] < 0) ended = 1;
      if (ended) {
        CHECK(row[k + 1] == -1 && w[i * LEN + k] == 0.0f, "walk %d step %d after its end", i, k);
        CHECK(row[k] == -1 || row[k] == 5, "walk %d ended at %d, which has out-edges", i, row[k]);
      } else {
        CHECK(is_edge(row[k], row[k + 1], ids, w[i * LEN + k]), "walk %d step %d: (%d, %d) is no edge or its weight is wrong",
              i, k, row[k], row[k + 1]);
      }
    }
  }
  CHECK(paths[LEN + 1 + 1] == -1, "vertex 5 has no out-edges");
  cugraph_random_walk_result_free(res);

  /* the node2vec entry points are stubs */
  rc = cugraph_node2vec_random_walks(h, g.graph, start_v, LEN, 1.0, 1.0, &res, &err);
  CHECK(rc == CUGRAPH_NOT_IMPLEMENTED && res == NULL && err != NULL, "node2vec_random_walks returned %d", (int)rc);
  cugraph_error_free(err);
  rc = cugraph_node2vec(h, g.graph, start_v, LEN, FALSE, 1.0, 1.0, &res, &err);
  CHECK(rc == CUGRAPH_NOT_IMPLEMENTED && res == NULL && err != NULL, "node2vec returned %d", (int)rc);
  cugraph_error_free(err);
  /* a graph with weights that are really edge ids is still "weighted": a biased walk runs */
  rc = cugraph_biased_random_walks(h, g.graph, start_v, LEN, &res, &err);
  CHECK_RC(rc, err, "cugraph_biased_random_walks");
  cugraph_random_walk_result_free(res);

  cugraph_type_erased_device_array_view_free(start_v);
  cugraph_type_erased_device_array_free(start_d);
  free_graph(&g);
  cugraph_free_resource_handle(h);
  return 0;
#undef LEN
}

int main(void)
{
  struct { const char* name; int (*fn)(void); } tests[] = {
    {"sample", test_sample}, {"sample_all_neighbors", test_sample_all_neighbors}, {"uniform_walk", test_uniform_walk},
  };
  for (size_t i = 0; i < sizeof(tests) / sizeof(tests[0]); ++i) {
    int before = g_failures;
    tests[i].fn();
    printf("%s %s\n", g_failures == before ? "PASS" : "FAIL", tests[i].name);
  }
  printf("%d failure(s)\n", g_failures);
  return g_failures;
}
