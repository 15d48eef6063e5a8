/*
 * Plain-C client of libcugraph_c's k-truss entry point, compiled against the include/cugraph_c headers
 * only (no HIP, no C++), in the manner of core_test.c.  It runs Zachary's karate club (the 78 edges of
 * tests/golden/karate.csv) at k = 5 against the 14 edges tests/golden/k_truss_vectors.json records
 * (tests/test_k_truss_c.py checks that the arrays below are those files'), the diamond, and the error
 * paths, through cugraph_k_truss_subgraph and every cugraph_induced_subgraph_* getter and the free.
 *
 * Build: gcc -std=c99 -I include tests/c/k_truss_test.c -L <lib> -lcugraph_c
 * Run:   ./k_truss_test        (needs a GPU; exit status = number of failures)
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

/* tests/golden/karate.csv as undirected edges (lower id first) */
#define KARATE_EDGES 78
static const int32_t KARATE_U[KARATE_EDGES] = {
  0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 1, 1, 1, 1, 2, 2, 2, 2, 2, 2, 2, 2, 3, 3, 3, 4, 4, 5, 5,
  5, 6, 8, 8, 8, 9, 13, 14, 14, 15, 15, 18, 18, 19, 20, 20, 22, 22, 23, 23, 23, 23, 23, 24, 24, 24, 25, 26, 26, 27, 28,
  28, 29, 29, 30, 30, 31, 31, 32};
static const int32_t KARATE_V[KARATE_EDGES] = {
  1, 2, 3, 4, 5, 6, 7, 8, 10, 11, 12, 13, 17, 19, 21, 31, 2, 3, 7, 13, 17, 19, 21, 30, 3, 7, 8, 9, 13, 27, 28, 32, 7,
  12, 13, 6, 10, 6, 10, 16, 16, 30, 32, 33, 33, 33, 32, 33, 32, 33, 32, 33, 33, 32, 33, 32, 33, 25, 27, 29, 32, 33, 25,
  27, 31, 31, 29, 33, 33, 31, 33, 32, 33, 32, 33, 32, 33, 33};
/* tests/golden/k_truss_vectors.json, karate.csv, k = 5 */
#define TRUSS5_EDGES 14
static const int32_t TRUSS5_U[TRUSS5_EDGES] = {0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 3, 3};
static const int32_t TRUSS5_V[TRUSS5_EDGES] = {1, 2, 3, 7, 13, 2, 3, 7, 13, 3, 7, 13, 7, 13};
/* the diamond: K4 without the edge 2 - 3 */
#define DIAMOND_EDGES 5
static const int32_t DIAMOND_U[DIAMOND_EDGES] = {0, 0, 0, 1, 1};
static const int32_t DIAMOND_V[DIAMOND_EDGES] = {1, 2, 3, 2, 3};

#define MAX_ENTRIES (2 * KARATE_EDGES)

static float pair_weight(int32_t a, int32_t b) { return (float)((a < b ? a : b) * 64 + (a < b ? b : a)) + 0.25f; }

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
  cugraph_type_erased_device_array_t *src, *dst, *wgt;
  cugraph_type_erased_device_array_view_t *src_v, *dst_v, *wgt_v;
  cugraph_graph_t* graph;
} test_graph_t;

static void free_graph(test_graph_t* g)
{
  if (g->graph) cugraph_sg_graph_free(g->graph);
  if (g->src_v) cugraph_type_erased_device_array_view_free(g->src_v);
  if (g->dst_v) cugraph_type_erased_device_array_view_free(g->dst_v);
  if (g->wgt_v) cugraph_type_erased_device_array_view_free(g->wgt_v);
  if (g->src) cugraph_type_erased_device_array_free(g->src);
  if (g->dst) cugraph_type_erased_device_array_free(g->dst);
  if (g->wgt) cugraph_type_erased_device_array_free(g->wgt);
  memset(g, 0, sizeof(*g));
}

/* ne undirected edges; both_ways: each is stored in both directions.  Not renumbered. */
static cugraph_error_code_t make_graph(const cugraph_resource_handle_t* h, const int32_t* u, const int32_t* v,
                                       size_t ne, bool_t both_ways, bool_t weighted, bool_t symmetric,
                                       test_graph_t* g, cugraph_error_t** err)
{
  int32_t s[MAX_ENTRIES], d[MAX_ENTRIES];
  float w[MAX_ENTRIES];
  size_t n = 0;
  for (size_t i = 0; i < ne; ++i) {
    s[n] = u[i];
    d[n] = v[i];
    w[n] = pair_weight(u[i], v[i]);
    ++n;
    if (both_ways) {
      s[n] = v[i];
      d[n] = u[i];
      w[n] = pair_weight(u[i], v[i]);
      ++n;
    }
  }
  memset(g, 0, sizeof(*g));
  *err                            = NULL;
  cugraph_graph_properties_t prop = {symmetric, FALSE};
  g->src                          = to_device(h, s, n, INT32, &g->src_v);
  g->dst                          = to_device(h, d, n, INT32, &g->dst_v);
  if (weighted) g->wgt = to_device(h, w, n, FLOAT32, &g->wgt_v);
  if (!g->src || !g->dst || (weighted && !g->wgt)) return CUGRAPH_ALLOC_ERROR;
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

static int by_pair(const void* a, const void* b)
{
  const int32_t *x = (const int32_t*)a, *y = (const int32_t*)b;
  if (x[0] != y[0]) return x[0] < y[0] ? -1 : 1;
  return x[1] < y[1] ? -1 : (x[1] > y[1] ? 1 : 0);
}

/* the result holds both directions of the ne edges, in row order (ids are not renumbered: ascending pairs) */
static int check_result(const cugraph_resource_handle_t* h, cugraph_induced_subgraph_result_t* res,
                        const int32_t* u, const int32_t* v, size_t ne, bool_t weighted)
{
  int32_t want[MAX_ENTRIES][2], s[MAX_ENTRIES], d[MAX_ENTRIES];
  float w[MAX_ENTRIES];
  int64_t off[2] = {-1, -1};
  size_t n = 2 * ne;
  for (size_t i = 0; i < ne; ++i) {
    want[2 * i][0]     = u[i];
    want[2 * i][1]     = v[i];
    want[2 * i + 1][0] = v[i];
    want[2 * i + 1][1] = u[i];
  }
  qsort(want, n, sizeof(want[0]), by_pair);
  if (copy_back(h, cugraph_induced_subgraph_get_sources(res), s, n, INT32)) return 1;
  if (copy_back(h, cugraph_induced_subgraph_get_destinations(res), d, n, INT32)) return 1;
  for (size_t i = 0; i < n; ++i)
    CHECK(s[i] == want[i][0] && d[i] == want[i][1], "edge %zu = (%d, %d), expected (%d, %d)", i, s[i], d[i],
          want[i][0], want[i][1]);
  if (copy_back(h, cugraph_induced_subgraph_get_subgraph_offsets(res), off, 2, INT64)) return 1;
  CHECK(off[0] == 0 && off[1] == (int64_t)n, "offsets {%lld, %lld}, expected {0, %zu}", (long long)off[0],
        (long long)off[1], n);
  cugraph_type_erased_device_array_view_t* wv = cugraph_induced_subgraph_get_edge_weights(res);
  if (weighted) {
    if (copy_back(h, wv, w, n, FLOAT32)) return 1;
    for (size_t i = 0; i < n; ++i)
      CHECK(w[i] == pair_weight(s[i], d[i]), "weight %zu = %g, expected %g", i, (double)w[i],
            (double)pair_weight(s[i], d[i]));
  } else {
    CHECK(wv == NULL, "an unweighted graph gave a weights view");
  }
  return 0;
}

static int run_case(const int32_t* u, const int32_t* v, size_t ne, bool_t weighted, size_t k, const int32_t* wu,
                    const int32_t* wv, size_t wn)
{
  cugraph_resource_handle_t* h = cugraph_create_resource_handle(NULL);
  CHECK(h != NULL, "resource handle");
  test_graph_t g;
  cugraph_error_t* err    = NULL;
  cugraph_error_code_t rc = make_graph(h, u, v, ne, TRUE, weighted, TRUE, &g, &err);
  CHECK_RC(rc, err, "sg_graph_create");
  cugraph_induced_subgraph_result_t* res = NULL;
  rc = cugraph_k_truss_subgraph(h, g.graph, k, FALSE, &res, &err);
  CHECK_RC(rc, err, "cugraph_k_truss_subgraph");
  CHECK(res != NULL, "no result");
  if (check_result(h, res, wu, wv, wn, weighted)) return 1;
  cugraph_induced_subgraph_result_free(res);
  free_graph(&g);
  cugraph_free_resource_handle(h);
  return 0;
}

static int test_k_truss(void)
{
  if (run_case(KARATE_U, KARATE_V, KARATE_EDGES, FALSE, 5, TRUSS5_U, TRUSS5_V, TRUSS5_EDGES)) return 1;
  if (run_case(KARATE_U, KARATE_V, KARATE_EDGES, FALSE, 2, KARATE_U, KARATE_V, KARATE_EDGES)) return 1;
  if (run_case(KARATE_U, KARATE_V, KARATE_EDGES, FALSE, 6, NULL, NULL, 0)) return 1;
  /* the diamond is its own 3-truss; at k = 4 the outer edges go, then the spine */
  if (run_case(DIAMOND_U, DIAMOND_V, DIAMOND_EDGES, FALSE, 3, DIAMOND_U, DIAMOND_V, DIAMOND_EDGES)) return 1;
  if (run_case(DIAMOND_U, DIAMOND_V, DIAMOND_EDGES, FALSE, 4, NULL, NULL, 0)) return 1;
  return 0;
}

static int test_k_truss_weights(void)
{
  if (run_case(KARATE_U, KARATE_V, KARATE_EDGES, TRUE, 5, TRUSS5_U, TRUSS5_V, TRUSS5_EDGES)) return 1;
  if (run_case(DIAMOND_U, DIAMOND_V, DIAMOND_EDGES, TRUE, 3, DIAMOND_U, DIAMOND_V, DIAMOND_EDGES)) return 1;
  if (run_case(DIAMOND_U, DIAMOND_V, DIAMOND_EDGES, TRUE, 4, NULL, NULL, 0)) return 1;
  return 0;
}

static int expect_error(cugraph_error_code_t rc, cugraph_error_code_t want, cugraph_error_t** err, const void* result,
                        const char* needle, const char* what)
{
  CHECK(rc == want, "%s gave %d", what, (int)rc);
  CHECK(result == NULL, "%s: result not reset on error", what);
  CHECK(*err != NULL && strstr(cugraph_error_message(*err), needle) != NULL, "%s: message \"%s\" lacks \"%s\"", what,
        *err ? cugraph_error_message(*err) : "", needle);
  cugraph_error_free(*err);
  *err = NULL;
  return 0;
}

static int test_k_truss_errors(void)
{
  cugraph_resource_handle_t* h = cugraph_create_resource_handle(NULL);
  CHECK(h != NULL, "resource handle");
  cugraph_error_t* err = NULL;
  cugraph_error_code_t rc;
  cugraph_induced_subgraph_result_t* res = (cugraph_induced_subgraph_result_t*)&rc; /* must be reset to NULL */
  rc = cugraph_k_truss_subgraph(h, NULL, 3, FALSE, &res, &err);
  if (expect_error(rc, CUGRAPH_INVALID_INPUT, &err, res, "graph is NULL", "a NULL graph")) return 1;
  test_graph_t g;
  /* one direction of every edge, not flagged symmetric */
  rc = make_graph(h, DIAMOND_U, DIAMOND_V, DIAMOND_EDGES, FALSE, FALSE, FALSE, &g, &err);
  CHECK_RC(rc, err, "sg_graph_create");
  res = (cugraph_induced_subgraph_result_t*)&rc;
  rc  = cugraph_k_truss_subgraph(h, g.graph, 3, FALSE, &res, &err);
  if (expect_error(rc, CUGRAPH_INVALID_INPUT, &err, res, "only undirected graphs", "a directed graph")) return 1;
  free_graph(&g);
  res = (cugraph_induced_subgraph_result_t*)&rc;
  rc  = cugraph_k_truss_subgraph(NULL, NULL, 3, FALSE, &res, &err);
  if (expect_error(rc, CUGRAPH_INVALID_HANDLE, &err, res, "handle", "a NULL handle")) return 1;
  cugraph_free_resource_handle(h);
  return 0;
}

int main(void)
{
  struct { const char* name; int (*fn)(void); } tests[] = {
    {"k_truss", test_k_truss}, {"k_truss_weights", test_k_truss_weights}, {"k_truss_errors", test_k_truss_errors},
  };
  for (size_t i = 0; i < sizeof(tests) / sizeof(tests[0]); ++i) {
    int before = g_failures;
    tests[i].fn();
    printf("%s %s\n", g_failures == before ? "PASS" : "FAIL", tests[i].name);
  }
  printf("%d failure(s)\n", g_failures);
  return g_failures;
}
