/*
 * Plain-C client of libcugraph_c's core number / k-core entry points, compiled against the
 * include/cugraph_c headers only (no HIP, no C++), in the manner of capi_test.c.  It runs the
 * 7-vertex graph of the reference's cpp/tests/c_api/core_number_test.c and k_core_test.c (the
 * numbers of tests/golden/core_vectors.json) through cugraph_core_number,
 * cugraph_core_result_create, cugraph_k_core and every getter and free.  The reference's
 * k_core test expects failure (its cugraph::k_core is unimplemented) and keeps the intended
 * result in a disabled branch (k_core_test.c:82-151); that result is what is checked here.
 *
 * Build: gcc -std=c99 -I include tests/c/core_test.c -L <lib> -lcugraph_c
 * Run:   ./core_test            (needs a GPU; exit status = number of failures)
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

#define NV 7
#define NE 22
static const int32_t SRC[NE] = {0, 1, 1, 2, 2, 2, 3, 4, 1, 3, 4, 0, 1, 3, 5, 5, 3, 1, 4, 5, 5, 6};
static const int32_t DST[NE] = {1, 3, 4, 0, 1, 3, 5, 5, 0, 1, 1, 2, 2, 2, 3, 4, 4, 5, 3, 1, 6, 5};
static const int32_t CORE[NV] = {2, 3, 2, 3, 3, 3, 1};
/* k = 3, in row order */
#define NK 12
static const int32_t K3_SRC[NK] = {1, 1, 1, 3, 3, 3, 4, 4, 4, 5, 5, 5};
static const int32_t K3_DST[NK] = {3, 4, 5, 1, 4, 5, 1, 3, 5, 1, 3, 4};

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

/* the graph above (ne of its entries), all weights 1, not renumbered */
static cugraph_error_code_t make_graph(const cugraph_resource_handle_t* h, size_t ne, bool_t weighted,
                                       bool_t symmetric, test_graph_t* g, cugraph_error_t** err)
{
  float w[NE];
  for (int i = 0; i < NE; ++i) w[i] = 1.0f;
  memset(g, 0, sizeof(*g));
  *err                            = NULL;
  cugraph_graph_properties_t prop = {symmetric, FALSE};
  g->src                          = to_device(h, SRC, ne, INT32, &g->src_v);
  g->dst                          = to_device(h, DST, ne, INT32, &g->dst_v);
  if (weighted) g->wgt = to_device(h, w, ne, FLOAT32, &g->wgt_v);
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

/* cpp/tests/c_api/core_number_test.c: IN gives {2,3,2,3,3,3,1}; OUT the same, INOUT twice that */
static int test_core_number(void)
{
  cugraph_resource_handle_t* h = cugraph_create_resource_handle(NULL);
  CHECK(h != NULL, "resource handle");
  test_graph_t g;
  cugraph_error_t* err    = NULL;
  cugraph_error_code_t rc = make_graph(h, NE, TRUE, TRUE, &g, &err);
  CHECK_RC(rc, err, "sg_graph_create");
  const cugraph_k_core_degree_type_t types[3] = {K_CORE_DEGREE_TYPE_IN, K_CORE_DEGREE_TYPE_OUT,
                                                 K_CORE_DEGREE_TYPE_INOUT};
  for (int t = 0; t < 3; ++t) {
    cugraph_core_result_t* res = NULL;
    rc = cugraph_core_number(h, g.graph, types[t], t == 0 ? TRUE : FALSE, &res, &err);
    CHECK_RC(rc, err, "cugraph_core_number");
    int32_t vert[NV], core[NV];
    if (copy_back(h, cugraph_core_result_get_vertices(res), vert, NV, INT32)) return 1;
    if (copy_back(h, cugraph_core_result_get_core_numbers(res), core, NV, INT32)) return 1;
    for (int i = 0; i < NV; ++i) {
      CHECK(vert[i] == i, "vertices[%d] = %d", i, vert[i]);
      CHECK(core[i] == CORE[i] * (t == 2 ? 2 : 1), "degree type %d: core[%d] = %d", t, i, core[i]);
    }
    cugraph_core_result_free(res);
  }
  free_graph(&g);
  cugraph_free_resource_handle(h);
  return 0;
}

static int check_k3(const cugraph_resource_handle_t* h, cugraph_k_core_result_t* res, bool_t weighted)
{
  int32_t s[NK], d[NK];
  float w[NK];
  if (copy_back(h, cugraph_k_core_result_get_src_vertices(res), s, NK, INT32)) return 1;
  if (copy_back(h, cugraph_k_core_result_get_dst_vertices(res), d, NK, INT32)) return 1;
  for (int i = 0; i < NK; ++i)
    CHECK(s[i] == K3_SRC[i] && d[i] == K3_DST[i], "k_core edge %d = (%d, %d), expected (%d, %d)", i, s[i], d[i],
          K3_SRC[i], K3_DST[i]);
  cugraph_type_erased_device_array_view_t* wv = cugraph_k_core_result_get_weights(res);
  if (weighted) {
    if (copy_back(h, wv, w, NK, FLOAT32)) return 1;
    for (int i = 0; i < NK; ++i) CHECK(w[i] == 1.0f, "k_core weight %d = %g", i, (double)w[i]);
  } else {
    CHECK(wv == NULL, "weights of an unweighted graph are not NULL");
  }
  return 0;
}

/* cpp/tests/c_api/k_core_test.c:82-151, the branch the reference keeps disabled */
static int test_k_core(void)
{
  cugraph_resource_handle_t* h = cugraph_create_resource_handle(NULL);
  CHECK(h != NULL, "resource handle");
  cugraph_error_t* err = NULL;
  for (int weighted = 1; weighted >= 0; --weighted) {
    test_graph_t g;
    cugraph_error_code_t rc = make_graph(h, NE, weighted ? TRUE : FALSE, TRUE, &g, &err);
    CHECK_RC(rc, err, "sg_graph_create");
    /* core numbers computed inside */
    cugraph_k_core_result_t* res = NULL;
    rc = cugraph_k_core(h, g.graph, 3, K_CORE_DEGREE_TYPE_IN, NULL, FALSE, &res, &err);
    CHECK_RC(rc, err, "cugraph_k_core (core_result NULL)");
    if (check_k3(h, res, weighted ? TRUE : FALSE)) return 1;
    cugraph_k_core_result_free(res);
    /* ... from cugraph_core_number's own result */
    cugraph_core_result_t* core = NULL;
    rc = cugraph_core_number(h, g.graph, K_CORE_DEGREE_TYPE_IN, FALSE, &core, &err);
    CHECK_RC(rc, err, "cugraph_core_number");
    rc = cugraph_k_core(h, g.graph, 3, K_CORE_DEGREE_TYPE_INOUT /* ignored */, core, TRUE, &res, &err);
    CHECK_RC(rc, err, "cugraph_k_core (core_result given)");
    if (check_k3(h, res, weighted ? TRUE : FALSE)) return 1;
    cugraph_k_core_result_free(res);
    /* ... and from a result made of the caller's arrays, in another order */
    int32_t ids[NV], vals[NV], back[NV];
    for (int i = 0; i < NV; ++i) {
      ids[i]  = NV - 1 - i;
      vals[i] = CORE[NV - 1 - i];
    }
    cugraph_type_erased_device_array_view_t *iv = NULL, *cv = NULL;
    cugraph_type_erased_device_array_t* ia = to_device(h, ids, NV, INT32, &iv);
    cugraph_type_erased_device_array_t* ca = to_device(h, vals, NV, INT32, &cv);
    CHECK(ia && ca, "device arrays");
    cugraph_core_result_t* made = NULL;
    rc = cugraph_core_result_create(h, iv, cv, &made, &err);
    CHECK_RC(rc, err, "cugraph_core_result_create");
    /* the result owns copies: the caller's arrays may go */
    cugraph_type_erased_device_array_view_free(iv);
    cugraph_type_erased_device_array_view_free(cv);
    cugraph_type_erased_device_array_free(ia);
    cugraph_type_erased_device_array_free(ca);
    if (copy_back(h, cugraph_core_result_get_vertices(made), back, NV, INT32)) return 1;
    CHECK(memcmp(back, ids, sizeof(ids)) == 0, "created result's vertices differ");
    if (copy_back(h, cugraph_core_result_get_core_numbers(made), back, NV, INT32)) return 1;
    CHECK(memcmp(back, vals, sizeof(vals)) == 0, "created result's core numbers differ");
    rc = cugraph_k_core(h, g.graph, 3, K_CORE_DEGREE_TYPE_IN, made, TRUE, &res, &err);
    CHECK_RC(rc, err, "cugraph_k_core (created core_result)");
    if (check_k3(h, res, weighted ? TRUE : FALSE)) return 1;
    cugraph_k_core_result_free(res);
    /* k = 0: every entry; k = 4: none */
    rc = cugraph_k_core(h, g.graph, 0, K_CORE_DEGREE_TYPE_IN, made, FALSE, &res, &err);
    CHECK_RC(rc, err, "cugraph_k_core k = 0");
    cugraph_type_erased_device_array_view_t* sv = cugraph_k_core_result_get_src_vertices(res);
    CHECK(cugraph_type_erased_device_array_view_size(sv) == NE, "k = 0 gave %zu entries",
          cugraph_type_erased_device_array_view_size(sv));
    cugraph_type_erased_device_array_view_free(sv);
    cugraph_k_core_result_free(res);
    rc = cugraph_k_core(h, g.graph, 4, K_CORE_DEGREE_TYPE_IN, made, FALSE, &res, &err);
    CHECK_RC(rc, err, "cugraph_k_core k = 4");
    sv = cugraph_k_core_result_get_src_vertices(res);
    CHECK(sv != NULL && cugraph_type_erased_device_array_view_size(sv) == 0, "k = 4 is not empty");
    cugraph_type_erased_device_array_view_free(sv);
    cugraph_k_core_result_free(res);
    cugraph_core_result_free(made);
    cugraph_core_result_free(core);
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

static int test_core_errors(void)
{
  cugraph_resource_handle_t* h = cugraph_create_resource_handle(NULL);
  CHECK(h != NULL, "resource handle");
  cugraph_error_t* err = NULL;
  test_graph_t g;
  /* the first 8 entries alone, not flagged symmetric (core_number_impl.cuh:93-94) */
  cugraph_error_code_t rc = make_graph(h, 8, TRUE, FALSE, &g, &err);
  CHECK_RC(rc, err, "sg_graph_create");
  cugraph_core_result_t* res = (cugraph_core_result_t*)&rc; /* must be reset to NULL */
  rc = cugraph_core_number(h, g.graph, K_CORE_DEGREE_TYPE_IN, FALSE, &res, &err);
  if (expect_invalid(rc, &err, res, "only undirected graphs", "core_number of a directed graph")) return 1;
  cugraph_k_core_result_t* kres = (cugraph_k_core_result_t*)&rc;
  rc = cugraph_k_core(h, g.graph, 2, K_CORE_DEGREE_TYPE_IN, NULL, FALSE, &kres, &err);
  if (expect_invalid(rc, &err, kres, "only undirected graphs", "k_core of a directed graph")) return 1;
  free_graph(&g);

  rc = make_graph(h, NE, FALSE, TRUE, &g, &err);
  CHECK_RC(rc, err, "sg_graph_create");
  rc = cugraph_core_number(h, g.graph, (cugraph_k_core_degree_type_t)3, FALSE, &res, &err);
  if (expect_invalid(rc, &err, res, "degree_type", "degree type 3")) return 1;
  /* a core result whose arrays differ in length, and one in the wrong dtype */
  int32_t ids[NV] = {0, 1, 2, 3, 4, 5, 6};
  int64_t wide[NV] = {2, 3, 2, 3, 3, 3, 1};
  cugraph_type_erased_device_array_view_t *iv = NULL, *cv = NULL, *wv = NULL;
  cugraph_type_erased_device_array_t* ia = to_device(h, ids, NV, INT32, &iv);
  cugraph_type_erased_device_array_t* ca = to_device(h, CORE, NV - 1, INT32, &cv);
  cugraph_type_erased_device_array_t* wa = to_device(h, wide, NV, INT64, &wv);
  CHECK(ia && ca && wa, "device arrays");
  cugraph_core_result_t* made = NULL;
  rc = cugraph_core_result_create(h, iv, cv, &made, &err);
  CHECK_RC(rc, err, "cugraph_core_result_create");
  rc = cugraph_k_core(h, g.graph, 2, K_CORE_DEGREE_TYPE_IN, made, FALSE, &kres, &err);
  if (expect_invalid(rc, &err, kres, "length", "core result of two lengths")) return 1;
  cugraph_core_result_free(made);
  rc = cugraph_core_result_create(h, iv, wv, &made, &err);
  CHECK_RC(rc, err, "cugraph_core_result_create");
  rc = cugraph_k_core(h, g.graph, 2, K_CORE_DEGREE_TYPE_IN, made, FALSE, &kres, &err);
  if (expect_invalid(rc, &err, kres, "edge type", "64-bit core numbers on a 32-bit graph")) return 1;
  cugraph_core_result_free(made);
  cugraph_type_erased_device_array_view_free(iv);
  cugraph_type_erased_device_array_view_free(cv);
  cugraph_type_erased_device_array_view_free(wv);
  cugraph_type_erased_device_array_free(ia);
  cugraph_type_erased_device_array_free(ca);
  cugraph_type_erased_device_array_free(wa);
  free_graph(&g);
  cugraph_free_resource_handle(h);
  return 0;
}

int main(void)
{
  struct { const char* name; int (*fn)(void); } tests[] = {
    {"core_number", test_core_number}, {"k_core", test_k_core}, {"core_errors", test_core_errors},
  };
  for (size_t i = 0; i < sizeof(tests) / sizeof(tests[0]); ++i) {
    int before = g_failures;
    tests[i].fn();
    printf("%s %s\n", g_failures == before ? "PASS" : "FAIL", tests[i].name);
  }
  printf("%d failure(s)\n", g_failures);
  return g_failures;
}
