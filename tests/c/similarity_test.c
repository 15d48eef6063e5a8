/*
 * Plain-C client of libcugraph_c's vertex pair, similarity and two-hop entry points, compiled
 * against the include/cugraph_c headers only (no HIP, no C++), in the manner of core_test.c.  It
 * runs the 6-vertex graph and the 10 pairs of the reference's cpp/tests/c_api/similarity_test.c
 * (the numbers of tests/golden/similarity_vectors.json; the reference leaves its expected values
 * as TODO zeros) through cugraph_create_vertex_pairs, the three coefficient calls,
 * cugraph_two_hop_neighbors and every getter and free, then the error codes.
 *
 * Build: gcc -std=c99 -I include tests/c/similarity_test.c -L <lib> -lcugraph_c
 * Run:   ./similarity_test      (needs a GPU; exit status = number of failures)
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
#define NE 16
#define NP 10
static const int32_t SRC[NE] = {0, 1, 1, 2, 2, 2, 3, 4, 1, 3, 4, 0, 1, 3, 5, 5};
static const int32_t DST[NE] = {1, 3, 4, 0, 1, 3, 5, 5, 0, 1, 1, 2, 2, 2, 3, 4};
static const int32_t FIRST[NP]  = {0, 0, 0, 1, 1, 1, 2, 2, 2, 3};
static const int32_t SECOND[NP] = {1, 3, 4, 2, 3, 5, 3, 4, 5, 4};
/* scores as fractions; the library rounds num / den (double) once to float */
static const int JACCARD[NP][2]  = {{1, 5}, {2, 3}, {1, 3}, {2, 5}, {1, 6}, {1, 2}, {1, 5}, {1, 4}, {1, 4}, {2, 3}};
static const int SORENSEN[NP][2] = {{1, 3}, {4, 5}, {1, 2}, {4, 7}, {2, 7}, {2, 3}, {1, 3}, {2, 5}, {2, 5}, {4, 5}};
static const int OVERLAP[NP][2]  = {{1, 2}, {1, 1}, {1, 2}, {2, 3}, {1, 3}, {1, 1}, {1, 3}, {1, 2}, {1, 2}, {1, 1}};
#define NT 22
static const int32_t TWO_HOP[NT][2] = {{0, 1}, {0, 2}, {0, 3}, {0, 4}, {1, 0}, {1, 2}, {1, 3}, {1, 5},
                                       {2, 0}, {2, 1}, {2, 3}, {2, 4}, {2, 5}, {3, 0}, {3, 1}, {3, 2},
                                       {3, 4}, {4, 0}, {4, 2}, {4, 3}, {5, 1}, {5, 2}};

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

/* the graph above (ne of its entries), unweighted, not renumbered */
static cugraph_error_code_t make_graph(const cugraph_resource_handle_t* h, size_t ne, bool_t symmetric,
                                       test_graph_t* g, cugraph_error_t** err)
{
  memset(g, 0, sizeof(*g));
  *err                            = NULL;
  cugraph_graph_properties_t prop = {symmetric, FALSE};
  g->src                          = to_device(h, SRC, ne, INT32, &g->src_v);
  g->dst                          = to_device(h, DST, ne, INT32, &g->dst_v);
  if (!g->src || !g->dst) return CUGRAPH_ALLOC_ERROR;
  return cugraph_sg_graph_create(h, &prop, g->src_v, g->dst_v, NULL, NULL, NULL, FALSE, FALSE, FALSE, &g->graph,
                                 err);
}

typedef struct {
  cugraph_type_erased_device_array_t *a, *b;
  cugraph_type_erased_device_array_view_t *av, *bv;
} pair_arrays_t;

static void free_pair_arrays(pair_arrays_t* p)
{
  if (p->av) cugraph_type_erased_device_array_view_free(p->av);
  if (p->bv) cugraph_type_erased_device_array_view_free(p->bv);
  if (p->a) cugraph_type_erased_device_array_free(p->a);
  if (p->b) cugraph_type_erased_device_array_free(p->b);
  memset(p, 0, sizeof(*p));
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

typedef cugraph_error_code_t (*similarity_fn)(const cugraph_resource_handle_t*, cugraph_graph_t*,
                                              const cugraph_vertex_pairs_t*, bool_t, bool_t,
                                              cugraph_similarity_result_t**, cugraph_error_t**);

/* the fixture's pairs through one measure, with and without the expensive check */
static int run_measure(similarity_fn fn, const int want[NP][2], const char* what)
{
  cugraph_resource_handle_t* h = cugraph_create_resource_handle(NULL);
  CHECK(h != NULL, "resource handle");
  test_graph_t g;
  cugraph_error_t* err    = NULL;
  cugraph_error_code_t rc = make_graph(h, NE, TRUE, &g, &err);
  CHECK_RC(rc, err, "sg_graph_create");
  pair_arrays_t p;
  memset(&p, 0, sizeof(p));
  p.a = to_device(h, FIRST, NP, INT32, &p.av);
  p.b = to_device(h, SECOND, NP, INT32, &p.bv);
  CHECK(p.a && p.b, "device arrays");
  cugraph_vertex_pairs_t* pairs = NULL;
  rc = cugraph_create_vertex_pairs(h, g.graph, p.av, p.bv, &pairs, &err);
  CHECK_RC(rc, err, "cugraph_create_vertex_pairs");
  /* the pairs own copies: the caller's arrays may go */
  free_pair_arrays(&p);
  int32_t back[NP];
  if (copy_back(h, cugraph_vertex_pairs_get_first(pairs), back, NP, INT32)) return 1;
  CHECK(memcmp(back, FIRST, sizeof(back)) == 0, "vertex pairs: first differs");
  if (copy_back(h, cugraph_vertex_pairs_get_second(pairs), back, NP, INT32)) return 1;
  CHECK(memcmp(back, SECOND, sizeof(back)) == 0, "vertex pairs: second differs");
  for (int expensive = 0; expensive < 2; ++expensive) {
    cugraph_similarity_result_t* res = NULL;
    rc = fn(h, g.graph, pairs, FALSE, expensive ? TRUE : FALSE, &res, &err);
    CHECK_RC(rc, err, what);
    float score[NP];
    if (copy_back(h, cugraph_similarity_result_get_similarity(res), score, NP, FLOAT32)) return 1;
    for (int i = 0; i < NP; ++i) {
      float const expected = (float)((double)want[i][0] / (double)want[i][1]);
      CHECK(score[i] == expected, "%s: pair %d (%d, %d) = %.9g, expected %.9g", what, i, FIRST[i], SECOND[i],
            (double)score[i], (double)expected);
    }
    cugraph_similarity_result_free(res);
  }
  cugraph_vertex_pairs_free(pairs);
  free_graph(&g);
  cugraph_free_resource_handle(h);
  return 0;
}

static int test_jaccard(void) { return run_measure(cugraph_jaccard_coefficients, JACCARD, "jaccard"); }
static int test_sorensen(void) { return run_measure(cugraph_sorensen_coefficients, SORENSEN, "sorensen"); }
static int test_overlap(void) { return run_measure(cugraph_overlap_coefficients, OVERLAP, "overlap"); }

static int cmp_pair(const void* x, const void* y)
{
  const int32_t* a = (const int32_t*)x;
  const int32_t* b = (const int32_t*)y;
  if (a[0] != b[0]) return a[0] < b[0] ? -1 : 1;
  return a[1] < b[1] ? -1 : (a[1] > b[1] ? 1 : 0);
}

static int test_two_hop(void)
{
  cugraph_resource_handle_t* h = cugraph_create_resource_handle(NULL);
  CHECK(h != NULL, "resource handle");
  test_graph_t g;
  cugraph_error_t* err    = NULL;
  cugraph_error_code_t rc = make_graph(h, NE, TRUE, &g, &err);
  CHECK_RC(rc, err, "sg_graph_create");
  /* every vertex */
  cugraph_vertex_pairs_t* res = NULL;
  rc = cugraph_two_hop_neighbors(h, g.graph, NULL, &res, &err);
  CHECK_RC(rc, err, "cugraph_two_hop_neighbors");
  int32_t a[NT], b[NT], got[NT][2];
  if (copy_back(h, cugraph_vertex_pairs_get_first(res), a, NT, INT32)) return 1;
  if (copy_back(h, cugraph_vertex_pairs_get_second(res), b, NT, INT32)) return 1;
  for (int i = 0; i < NT; ++i) {
    got[i][0] = a[i];
    got[i][1] = b[i];
  }
  qsort(got, NT, sizeof(got[0]), cmp_pair);
  for (int i = 0; i < NT; ++i)
    CHECK(got[i][0] == TWO_HOP[i][0] && got[i][1] == TWO_HOP[i][1], "two-hop pair %d = (%d, %d), expected (%d, %d)", i,
          got[i][0], got[i][1], TWO_HOP[i][0], TWO_HOP[i][1]);
  cugraph_vertex_pairs_free(res);
  /* start vertices 5, 0, 5: the pairs of 0 and 5, once */
  int32_t start[3] = {5, 0, 5};
  cugraph_type_erased_device_array_view_t* sv = NULL;
  cugraph_type_erased_device_array_t* sa      = to_device(h, start, 3, INT32, &sv);
  CHECK(sa != NULL, "device array");
  rc = cugraph_two_hop_neighbors(h, g.graph, sv, &res, &err);
  CHECK_RC(rc, err, "cugraph_two_hop_neighbors (start vertices)");
  int32_t c[6], d[6], some[6][2];
  if (copy_back(h, cugraph_vertex_pairs_get_first(res), c, 6, INT32)) return 1;
  if (copy_back(h, cugraph_vertex_pairs_get_second(res), d, 6, INT32)) return 1;
  for (int i = 0; i < 6; ++i) {
    some[i][0] = c[i];
    some[i][1] = d[i];
  }
  qsort(some, 6, sizeof(some[0]), cmp_pair);
  for (int i = 0; i < 6; ++i) {
    const int32_t* want = TWO_HOP[i < 4 ? i : NT - 6 + i]; /* (0, *) are the first 4, (5, *) the last 2 */
    CHECK(some[i][0] == want[0] && some[i][1] == want[1], "two-hop from {0, 5}: pair %d = (%d, %d)", i, some[i][0],
          some[i][1]);
  }
  cugraph_vertex_pairs_free(res);
  /* a start vertex that is not in the graph */
  start[1] = 17;
  rc       = cugraph_type_erased_device_array_view_copy_from_host(h, sv, (const byte_t*)start, &err);
  CHECK_RC(rc, err, "copy from host");
  res = (cugraph_vertex_pairs_t*)&rc; /* must be reset to NULL */
  rc  = cugraph_two_hop_neighbors(h, g.graph, sv, &res, &err);
  CHECK(rc == CUGRAPH_INVALID_INPUT && res == NULL && err != NULL, "unknown start vertex gave %d", (int)rc);
  cugraph_error_free(err);
  cugraph_type_erased_device_array_view_free(sv);
  cugraph_type_erased_device_array_free(sa);
  free_graph(&g);
  cugraph_free_resource_handle(h);
  return 0;
}

static int expect_error(cugraph_error_code_t rc, cugraph_error_code_t want, cugraph_error_t** err, const void* result,
                        const char* needle, const char* what)
{
  CHECK(rc == want, "%s gave %d, expected %d", what, (int)rc, (int)want);
  CHECK(result == NULL, "%s: result not reset on error", what);
  CHECK(*err != NULL && strstr(cugraph_error_message(*err), needle) != NULL, "%s: message \"%s\" lacks \"%s\"", what,
        *err ? cugraph_error_message(*err) : "", needle);
  cugraph_error_free(*err);
  *err = NULL;
  return 0;
}

static int test_similarity_errors(void)
{
  cugraph_resource_handle_t* h = cugraph_create_resource_handle(NULL);
  CHECK(h != NULL, "resource handle");
  cugraph_error_t* err = NULL;
  test_graph_t g;
  cugraph_error_code_t rc = make_graph(h, NE, TRUE, &g, &err);
  CHECK_RC(rc, err, "sg_graph_create");
  int64_t wide[NP];
  int32_t with_unknown[NP];
  for (int i = 0; i < NP; ++i) {
    wide[i]         = SECOND[i];
    with_unknown[i] = SECOND[i];
  }
  with_unknown[3] = 99;
  cugraph_type_erased_device_array_view_t *av = NULL, *bv = NULL, *wv = NULL, *sv = NULL, *uv = NULL;
  cugraph_type_erased_device_array_t* aa = to_device(h, FIRST, NP, INT32, &av);
  cugraph_type_erased_device_array_t* ba = to_device(h, SECOND, NP, INT32, &bv);
  cugraph_type_erased_device_array_t* wa = to_device(h, wide, NP, INT64, &wv);
  cugraph_type_erased_device_array_t* sa = to_device(h, SECOND, NP - 1, INT32, &sv);
  cugraph_type_erased_device_array_t* ua = to_device(h, with_unknown, NP, INT32, &uv);
  CHECK(aa && ba && wa && sa && ua, "device arrays");
  /* type and size mismatches (c_api/graph_functions.cpp:75-82) */
  cugraph_vertex_pairs_t* pairs = (cugraph_vertex_pairs_t*)&rc; /* must be reset to NULL */
  rc = cugraph_create_vertex_pairs(h, g.graph, wv, bv, &pairs, &err);
  if (expect_error(rc, CUGRAPH_INVALID_INPUT, &err, pairs, "vertex type of graph and first must match",
                   "64-bit first"))
    return 1;
  pairs = (cugraph_vertex_pairs_t*)&rc;
  rc    = cugraph_create_vertex_pairs(h, g.graph, av, wv, &pairs, &err);
  if (expect_error(rc, CUGRAPH_INVALID_INPUT, &err, pairs, "vertex type of graph and second must match",
                   "64-bit second"))
    return 1;
  pairs = (cugraph_vertex_pairs_t*)&rc;
  rc    = cugraph_create_vertex_pairs(h, g.graph, av, sv, &pairs, &err);
  if (expect_error(rc, CUGRAPH_INVALID_INPUT, &err, pairs, "length", "arrays of two lengths")) return 1;
  /* use_weight */
  rc = cugraph_create_vertex_pairs(h, g.graph, av, bv, &pairs, &err);
  CHECK_RC(rc, err, "cugraph_create_vertex_pairs");
  cugraph_similarity_result_t* res = (cugraph_similarity_result_t*)&rc;
  rc = cugraph_jaccard_coefficients(h, g.graph, pairs, TRUE, FALSE, &res, &err);
  if (expect_error(rc, CUGRAPH_NOT_IMPLEMENTED, &err, res,
                   "weighted similarity computations are not supported in this release", "use_weight"))
    return 1;
  /* an id that is not in the graph: scores 0, or is refused by the expensive check */
  cugraph_vertex_pairs_t* unknown = NULL;
  rc = cugraph_create_vertex_pairs(h, g.graph, av, uv, &unknown, &err);
  CHECK_RC(rc, err, "cugraph_create_vertex_pairs (unknown id)");
  rc = cugraph_sorensen_coefficients(h, g.graph, unknown, FALSE, FALSE, &res, &err);
  CHECK_RC(rc, err, "sorensen with an unknown id");
  float score[NP];
  if (copy_back(h, cugraph_similarity_result_get_similarity(res), score, NP, FLOAT32)) return 1;
  CHECK(score[3] == 0.0f, "unknown id scored %g", (double)score[3]);
  CHECK(score[4] == (float)(2.0 / 7.0), "pair after the unknown id scored %g", (double)score[4]);
  cugraph_similarity_result_free(res);
  res = (cugraph_similarity_result_t*)&rc;
  rc  = cugraph_overlap_coefficients(h, g.graph, unknown, FALSE, TRUE, &res, &err);
  if (expect_error(rc, CUGRAPH_INVALID_INPUT, &err, res, "invalid vertex IDs", "unknown id, expensive check"))
    return 1;
  cugraph_vertex_pairs_free(unknown);
  /* the first 8 entries alone, not flagged symmetric */
  test_graph_t d;
  rc = make_graph(h, 8, FALSE, &d, &err);
  CHECK_RC(rc, err, "sg_graph_create");
  similarity_fn fns[3] = {cugraph_jaccard_coefficients, cugraph_sorensen_coefficients, cugraph_overlap_coefficients};
  for (int i = 0; i < 3; ++i) {
    res = (cugraph_similarity_result_t*)&rc;
    rc  = fns[i](h, d.graph, pairs, FALSE, FALSE, &res, &err);
    if (expect_error(rc, CUGRAPH_INVALID_INPUT, &err, res, "undirected graphs only", "asymmetric graph")) return 1;
  }
  /* ... which two-hop accepts: 0 -> 1 -> {3, 4} among others */
  cugraph_vertex_pairs_t* hop = NULL;
  rc = cugraph_two_hop_neighbors(h, d.graph, NULL, &hop, &err);
  CHECK_RC(rc, err, "two-hop of a directed graph");
  cugraph_type_erased_device_array_view_t* hv = cugraph_vertex_pairs_get_first(hop);
  CHECK(cugraph_type_erased_device_array_view_size(hv) > 0, "two-hop of a directed graph is empty");
  cugraph_type_erased_device_array_view_free(hv);
  cugraph_vertex_pairs_free(hop);
  free_graph(&d);
  cugraph_vertex_pairs_free(pairs);
  cugraph_type_erased_device_array_view_free(av);
  cugraph_type_erased_device_array_view_free(bv);
  cugraph_type_erased_device_array_view_free(wv);
  cugraph_type_erased_device_array_view_free(sv);
  cugraph_type_erased_device_array_view_free(uv);
  cugraph_type_erased_device_array_free(aa);
  cugraph_type_erased_device_array_free(ba);
  cugraph_type_erased_device_array_free(wa);
  cugraph_type_erased_device_array_free(sa);
  cugraph_type_erased_device_array_free(ua);
  free_graph(&g);
  cugraph_free_resource_handle(h);
  return 0;
}

int main(void)
{
  struct { const char* name; int (*fn)(void); } tests[] = {
    {"jaccard", test_jaccard},   {"sorensen", test_sorensen}, {"overlap", test_overlap},
    {"two_hop", test_two_hop},   {"similarity_errors", test_similarity_errors},
  };
  for (size_t i = 0; i < sizeof(tests) / sizeof(tests[0]); ++i) {
    int before = g_failures;
    tests[i].fn();
    printf("%s %s\n", g_failures == before ? "PASS" : "FAIL", tests[i].name);
  }
  printf("%d failure(s)\n", g_failures);
  return g_failures;
}
