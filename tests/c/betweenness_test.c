/*
 * Plain-C client of libcugraph_c's betweenness and edge betweenness entry points, compiled against the
 * include/cugraph_c headers only (no HIP, no C++), in the manner of core_test.c.  A 6-vertex graph (a
 * diamond 0-1-3, 0-2-3 with the tail 3-4-5) goes through cugraph_betweenness_centrality,
 * cugraph_edge_betweenness_centrality and every getter and free; the expected values are those of
 * tests/betweenness_ref.py, compared within 1e-10 relative, zeros exactly.
 *
 * Build: gcc -std=c99 -I include tests/c/betweenness_test.c -L <lib> -lcugraph_c
 * Run:   ./betweenness_test      (needs a GPU; exit status = number of failures)
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
#define NE 12
/* both directions of 0-1, 0-2, 1-3, 2-3, 3-4, 4-5; the first six alone are the directed graph */
static const int32_t SRC[NE] = {0, 0, 1, 2, 3, 4, 1, 2, 3, 3, 4, 5};
static const int32_t DST[NE] = {1, 2, 3, 3, 4, 5, 0, 0, 1, 2, 3, 4};
/* the stored edges in row order */
static const int32_t ROW_SRC[NE] = {0, 0, 1, 1, 2, 2, 3, 3, 3, 4, 4, 5};
static const int32_t ROW_DST[NE] = {1, 2, 0, 3, 0, 3, 1, 2, 4, 3, 5, 4};

static const double BC_NORM[NV]    = {0.05, 0.15000000000000002, 0.15000000000000002, 0.65, 0.4, 0.0};
static const double BC_RAW_EP[NV]  = {5.5, 6.5, 6.5, 11.5, 9.0, 5.0};
static const double BC_LIST[NV]    = {0.0, 0.25, 0.25, 0.8, 0.9, 0.0}; /* sources 0, 5, 5, normalized */
static const double BC_DIRECTED[NV] = {0.0, 1.5, 1.5, 6.0, 4.0, 0.0}; /* first six edges, not normalized */
static const double EBC_RAW[NE]    = {1.5, 1.5, 1.5, 2.5, 1.5, 2.5, 2.5, 2.5, 4.0, 4.0, 2.5, 2.5};
static const double EBC_FROM_2[NE] = {0.016666666666666666, 0.0, 0.0, 0.0, 0.05, 0.11666666666666667,
                                      0.016666666666666666, 0.0, 0.06666666666666667, 0.0, 0.03333333333333333,
                                      0.0}; /* source 2, normalized */
static const double EBC_DIRECTED[6] = {2.5, 2.5, 4.5, 4.5, 8.0, 5.0};

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
  cugraph_type_erased_device_array_t *src, *dst;
  cugraph_type_erased_device_array_view_t *src_v, *dst_v;
  cugraph_graph_t* graph;
} test_graph_t;

static void free_graph(test_graph_t* g)
{
  if (g->graph) cugraph_sg_graph_free(g->graph);
  if (g->src_v) cugraph_type_erased_device_array_view_free(g->src_v);
  if (g->dst_v) cugraph_type_erased_device_array_view_free(g->dst_v);
  if (g->src) cugraph_type_erased_device_array_free(g->src);
  if (g->dst) cugraph_type_erased_device_array_free(g->dst);
  memset(g, 0, sizeof(*g));
}

/* the first ne entries of the graph above, not renumbered */
static cugraph_error_code_t make_graph(const cugraph_resource_handle_t* h, size_t ne, bool_t symmetric,
                                       bool_t transposed, test_graph_t* g, cugraph_error_t** err)
{
  memset(g, 0, sizeof(*g));
  *err                            = NULL;
  cugraph_graph_properties_t prop = {symmetric, FALSE};
  g->src                          = to_device(h, SRC, ne, INT32, &g->src_v);
  g->dst                          = to_device(h, DST, ne, INT32, &g->dst_v);
  if (!g->src || !g->dst) return CUGRAPH_ALLOC_ERROR;
  return cugraph_sg_graph_create(h, &prop, g->src_v, g->dst_v, NULL, NULL, NULL, transposed, FALSE, FALSE,
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

static int close_to(const double* got, const double* want, size_t n, const char* what)
{
  for (size_t i = 0; i < n; ++i) {
    double const diff = got[i] > want[i] ? got[i] - want[i] : want[i] - got[i];
    CHECK(want[i] == 0.0 ? got[i] == 0.0 : diff <= 1e-10 * want[i], "%s[%zu] = %.17g, expected %.17g", what, i,
          got[i], want[i]);
  }
  return 0;
}

static int check_vertices(const cugraph_resource_handle_t* h, cugraph_centrality_result_t* res, const double* want,
                          const char* what)
{
  int32_t vert[NV];
  double val[NV];
  if (copy_back(h, cugraph_centrality_result_get_vertices(res), vert, NV, INT32)) return 1;
  if (copy_back(h, cugraph_centrality_result_get_values(res), val, NV, FLOAT64)) return 1;
  for (int i = 0; i < NV; ++i) CHECK(vert[i] == i, "%s: vertices[%d] = %d", what, i, vert[i]);
  return close_to(val, want, NV, what);
}

static int test_betweenness(void)
{
  cugraph_resource_handle_t* h = cugraph_create_resource_handle(NULL);
  CHECK(h != NULL, "resource handle");
  cugraph_error_t* err = NULL;
  for (int transposed = 0; transposed < 2; ++transposed) {
    test_graph_t g;
    cugraph_error_code_t rc = make_graph(h, NE, TRUE, transposed ? TRUE : FALSE, &g, &err);
    CHECK_RC(rc, err, "sg_graph_create");
    cugraph_centrality_result_t* res = NULL;
    rc = cugraph_betweenness_centrality(h, g.graph, NULL, TRUE, FALSE, FALSE, &res, &err);
    CHECK_RC(rc, err, "cugraph_betweenness_centrality");
    if (check_vertices(h, res, BC_NORM, "normalized")) return 1;
    cugraph_centrality_result_free(res);
    rc = cugraph_betweenness_centrality(h, g.graph, NULL, FALSE, TRUE, TRUE, &res, &err);
    CHECK_RC(rc, err, "cugraph_betweenness_centrality (endpoints)");
    if (check_vertices(h, res, BC_RAW_EP, "endpoints")) return 1;
    cugraph_centrality_result_free(res);
    /* a source list with a repeated id: every entry is a source */
    int32_t const list[3]                       = {0, 5, 5};
    cugraph_type_erased_device_array_view_t* lv = NULL;
    cugraph_type_erased_device_array_t* la      = to_device(h, list, 3, INT32, &lv);
    CHECK(la != NULL, "device array");
    rc = cugraph_betweenness_centrality(h, g.graph, lv, TRUE, FALSE, FALSE, &res, &err);
    CHECK_RC(rc, err, "cugraph_betweenness_centrality (vertex_list)");
    if (check_vertices(h, res, BC_LIST, "vertex_list")) return 1;
    cugraph_centrality_result_free(res);
    cugraph_type_erased_device_array_view_free(lv);
    cugraph_type_erased_device_array_free(la);
    free_graph(&g);
    /* the directed graph of the first six edges */
    rc = make_graph(h, 6, FALSE, transposed ? TRUE : FALSE, &g, &err);
    CHECK_RC(rc, err, "sg_graph_create (directed)");
    rc = cugraph_betweenness_centrality(h, g.graph, NULL, FALSE, FALSE, FALSE, &res, &err);
    CHECK_RC(rc, err, "cugraph_betweenness_centrality (directed)");
    if (check_vertices(h, res, BC_DIRECTED, "directed")) return 1;
    cugraph_centrality_result_free(res);
    free_graph(&g);
  }
  cugraph_free_resource_handle(h);
  return 0;
}

static int check_edges(const cugraph_resource_handle_t* h, cugraph_edge_centrality_result_t* res, size_t ne,
                       const int32_t* src, const int32_t* dst, const double* want, const char* what)
{
  int32_t s[NE], d[NE];
  double val[NE];
  if (copy_back(h, cugraph_edge_centrality_result_get_src_vertices(res), s, ne, INT32)) return 1;
  if (copy_back(h, cugraph_edge_centrality_result_get_dst_vertices(res), d, ne, INT32)) return 1;
  if (copy_back(h, cugraph_edge_centrality_result_get_values(res), val, ne, FLOAT64)) return 1;
  for (size_t i = 0; i < ne; ++i)
    CHECK(s[i] == src[i] && d[i] == dst[i], "%s: edge %zu = (%d, %d), expected (%d, %d)", what, i, s[i], d[i], src[i],
          dst[i]);
  return close_to(val, want, ne, what);
}

static int test_edge_betweenness(void)
{
  cugraph_resource_handle_t* h = cugraph_create_resource_handle(NULL);
  CHECK(h != NULL, "resource handle");
  cugraph_error_t* err = NULL;
  for (int transposed = 0; transposed < 2; ++transposed) {
    test_graph_t g;
    cugraph_error_code_t rc = make_graph(h, NE, TRUE, transposed ? TRUE : FALSE, &g, &err);
    CHECK_RC(rc, err, "sg_graph_create");
    cugraph_edge_centrality_result_t* res = NULL;
    rc = cugraph_edge_betweenness_centrality(h, g.graph, NULL, FALSE, FALSE, &res, &err);
    CHECK_RC(rc, err, "cugraph_edge_betweenness_centrality");
    if (check_edges(h, res, NE, ROW_SRC, ROW_DST, EBC_RAW, "edges")) return 1;
    cugraph_edge_centrality_result_free(res);
    int32_t const list[1]                       = {2};
    cugraph_type_erased_device_array_view_t* lv = NULL;
    cugraph_type_erased_device_array_t* la      = to_device(h, list, 1, INT32, &lv);
    CHECK(la != NULL, "device array");
    rc = cugraph_edge_betweenness_centrality(h, g.graph, lv, TRUE, TRUE, &res, &err);
    CHECK_RC(rc, err, "cugraph_edge_betweenness_centrality (vertex_list)");
    if (check_edges(h, res, NE, ROW_SRC, ROW_DST, EBC_FROM_2, "edges from 2")) return 1;
    cugraph_edge_centrality_result_free(res);
    cugraph_type_erased_device_array_view_free(lv);
    cugraph_type_erased_device_array_free(la);
    free_graph(&g);
    rc = make_graph(h, 6, FALSE, transposed ? TRUE : FALSE, &g, &err);
    CHECK_RC(rc, err, "sg_graph_create (directed)");
    rc = cugraph_edge_betweenness_centrality(h, g.graph, NULL, FALSE, FALSE, &res, &err);
    CHECK_RC(rc, err, "cugraph_edge_betweenness_centrality (directed)");
    if (check_edges(h, res, 6, SRC, DST, EBC_DIRECTED, "directed edges")) return 1;
    cugraph_edge_centrality_result_free(res);
    free_graph(&g);
  }
  cugraph_free_resource_handle(h);
  return 0;
}

static int expect_invalid(cugraph_error_code_t rc, cugraph_error_t** err, const void* result, const char* needle,
                          const char* what)
{
  CHECK(rc == CUGRAPH_INVALID_INPUT, "%s gave %d", what, (int)rc);
  CHECK(result == NULL, "%s: result not reset on error", what);
  CHECK(*err != NULL && strstr(cugraph_error_message(*err), needle) != NULL, "%s: message \"%s\" lacks \"%s\"", what,
        *err ? cugraph_error_message(*err) : "", needle);
  cugraph_error_free(*err);
  *err = NULL;
  return 0;
}

static int test_betweenness_errors(void)
{
  cugraph_resource_handle_t* h = cugraph_create_resource_handle(NULL);
  CHECK(h != NULL, "resource handle");
  cugraph_error_t* err = NULL;
  test_graph_t g;
  cugraph_error_code_t rc = make_graph(h, NE, TRUE, FALSE, &g, &err);
  CHECK_RC(rc, err, "sg_graph_create");
  /* a vertex_list of another type than the graph's vertices */
  int64_t const wide[2]                       = {0, 1};
  cugraph_type_erased_device_array_view_t* wv = NULL;
  cugraph_type_erased_device_array_t* wa      = to_device(h, wide, 2, INT64, &wv);
  CHECK(wa != NULL, "device array");
  cugraph_centrality_result_t* res       = (cugraph_centrality_result_t*)&rc; /* must be reset to NULL */
  cugraph_edge_centrality_result_t* eres = (cugraph_edge_centrality_result_t*)&rc;
  rc = cugraph_betweenness_centrality(h, g.graph, wv, TRUE, FALSE, FALSE, &res, &err);
  if (expect_invalid(rc, &err, res, "vertex type", "64-bit vertex_list on a 32-bit graph")) return 1;
  rc = cugraph_edge_betweenness_centrality(h, g.graph, wv, TRUE, FALSE, &eres, &err);
  if (expect_invalid(rc, &err, eres, "vertex type", "64-bit vertex_list on a 32-bit graph (edges)")) return 1;
  cugraph_type_erased_device_array_view_free(wv);
  cugraph_type_erased_device_array_free(wa);
  /* an id the graph does not have */
  int32_t const bad[3][2] = {{1, 6}, {-1, 2}, {3, 2147483647}};
  for (int i = 0; i < 3; ++i) {
    cugraph_type_erased_device_array_view_t* bv = NULL;
    cugraph_type_erased_device_array_t* ba      = to_device(h, bad[i], 2, INT32, &bv);
    CHECK(ba != NULL, "device array");
    res  = (cugraph_centrality_result_t*)&rc;
    eres = (cugraph_edge_centrality_result_t*)&rc;
    rc   = cugraph_betweenness_centrality(h, g.graph, bv, TRUE, FALSE, FALSE, &res, &err);
    if (expect_invalid(rc, &err, res, "not in the graph", "unknown source")) return 1;
    rc = cugraph_edge_betweenness_centrality(h, g.graph, bv, TRUE, FALSE, &eres, &err);
    if (expect_invalid(rc, &err, eres, "not in the graph", "unknown source (edges)")) return 1;
    cugraph_type_erased_device_array_view_free(bv);
    cugraph_type_erased_device_array_free(ba);
  }
  /* an empty list is no error: all zeros */
  int32_t const none[1]                       = {0};
  cugraph_type_erased_device_array_view_t* ev = NULL;
  cugraph_type_erased_device_array_t* ea      = to_device(h, none, 0, INT32, &ev);
  CHECK(ea != NULL, "device array");
  rc = cugraph_betweenness_centrality(h, g.graph, ev, TRUE, TRUE, FALSE, &res, &err);
  CHECK_RC(rc, err, "cugraph_betweenness_centrality (empty list)");
  double const zeros[NE] = {0};
  if (check_vertices(h, res, zeros, "empty list")) return 1;
  cugraph_centrality_result_free(res);
  rc = cugraph_edge_betweenness_centrality(h, g.graph, ev, TRUE, FALSE, &eres, &err);
  CHECK_RC(rc, err, "cugraph_edge_betweenness_centrality (empty list)");
  if (check_edges(h, eres, NE, ROW_SRC, ROW_DST, zeros, "empty list edges")) return 1;
  cugraph_edge_centrality_result_free(eres);
  cugraph_type_erased_device_array_view_free(ev);
  cugraph_type_erased_device_array_free(ea);
  free_graph(&g);
  cugraph_free_resource_handle(h);
  return 0;
}

int main(void)
{
  struct { const char* name; int (*fn)(void); } tests[] = {
    {"betweenness", test_betweenness},
    {"edge_betweenness", test_edge_betweenness},
    {"betweenness_errors", test_betweenness_errors},
  };
  for (size_t i = 0; i < sizeof(tests) / sizeof(tests[0]); ++i) {
    int before = g_failures;
    tests[i].fn();
    printf("%s %s\n", g_failures == before ? "PASS" : "FAIL", tests[i].name);
  }
  printf("%d failure(s)\n", g_failures);
  return g_failures;
}
