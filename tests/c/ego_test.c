/*
 * Plain-C client of libcugraph_c's induced-subgraph and ego-net entry points, compiled against the
 * include/cugraph_c headers only (no HIP, no C++), in the manner of k_truss_test.c.  It runs Zachary's
 * karate club (the 78 edges of tests/golden/karate.csv) through cugraph_extract_ego against the ego nets
 * of vertices 0 and 33 at radius 1 that tests/golden/ego_vectors.json records (tests/test_ego_c.py checks
 * that the arrays below are those files'), the same vertex sets through cugraph_extract_induced_subgraph
 * in a scrambled order with an empty set between them, the weights, and the error returns.
 *
 * Build: gcc -std=c99 -I include tests/c/ego_test.c -L <lib> -lcugraph_c
 * Run:   ./ego_test        (needs a GPU; exit status = number of failures)
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
#define KARATE_VERTICES 34
static const int32_t KARATE_U[KARATE_EDGES] = {
  0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 1, 1, 1, 1, 2, 2, 2, 2, 2, 2, 2, 2, 3, 3, 3, 4, 4, 5, 5,
  5, 6, 8, 8, 8, 9, 13, 14, 14, 15, 15, 18, 18, 19, 20, 20, 22, 22, 23, 23, 23, 23, 23, 24, 24, 24, 25, 26, 26, 27, 28,
  28, 29, 29, 30, 30, 31, 31, 32};
static const int32_t KARATE_V[KARATE_EDGES] = {
  1, 2, 3, 4, 5, 6, 7, 8, 10, 11, 12, 13, 17, 19, 21, 31, 2, 3, 7, 13, 17, 19, 21, 30, 3, 7, 8, 9, 13, 27, 28, 32, 7,
  12, 13, 6, 10, 6, 10, 16, 16, 30, 32, 33, 33, 33, 32, 33, 32, 33, 32, 33, 33, 32, 33, 32, 33, 25, 27, 29, 32, 33, 25,
  27, 31, 31, 29, 33, 33, 31, 33, 32, 33, 32, 33, 32, 33, 33};
/* tests/golden/ego_vectors.json, karate.csv, seed 0, radius 1 */
#define EGO0_EDGES 34
static const int32_t EGO0_U[EGO0_EDGES] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1,
                                           1, 1, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 4, 4, 5, 5};
static const int32_t EGO0_V[EGO0_EDGES] = {1, 2,  3,  4,  5,  6,  7, 8, 10, 11, 12, 13, 17, 19, 21, 31, 2,
                                           3, 7, 13, 17, 19, 21, 3, 7, 8,  13, 7,  12, 13, 6,  10, 6,  10};
/* tests/golden/ego_vectors.json, karate.csv, seed 33, radius 1 */
#define EGO33_EDGES 32
static const int32_t EGO33_U[EGO33_EDGES] = {8,  8,  8,  9,  13, 14, 14, 15, 15, 18, 18, 19, 20, 20, 22, 22,
                                             23, 23, 23, 23, 26, 26, 27, 28, 28, 29, 29, 30, 30, 31, 31, 32};
static const int32_t EGO33_V[EGO33_EDGES] = {30, 32, 33, 33, 33, 32, 33, 32, 33, 32, 33, 33, 32, 33, 32, 33,
                                             27, 29, 32, 33, 29, 33, 33, 31, 33, 32, 33, 32, 33, 32, 33, 33};

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

/* karate, both directions of every edge, not renumbered */
static cugraph_error_code_t make_karate(const cugraph_resource_handle_t* h, bool_t weighted, test_graph_t* g,
                                        cugraph_error_t** err)
{
  int32_t s[MAX_ENTRIES], d[MAX_ENTRIES];
  float w[MAX_ENTRIES];
  size_t n = 0;
  for (size_t i = 0; i < KARATE_EDGES; ++i) {
    s[n] = KARATE_U[i];
    d[n] = KARATE_V[i];
    w[n] = pair_weight(KARATE_U[i], KARATE_V[i]);
    ++n;
    s[n] = KARATE_V[i];
    d[n] = KARATE_U[i];
    w[n] = pair_weight(KARATE_U[i], KARATE_V[i]);
    ++n;
  }
  memset(g, 0, sizeof(*g));
  *err                            = NULL;
  cugraph_graph_properties_t prop = {TRUE, FALSE};
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

typedef struct {
  const int32_t *u, *v; /* the expected undirected edges of one subgraph */
  size_t ne;
} expected_t;

/* subgraph i holds both directions of want[i]'s edges, ascending by (source, destination): the ids are not
 * renumbered, so the order of the internal ids is the order of the ids */
static int check_result(const cugraph_resource_handle_t* h, cugraph_induced_subgraph_result_t* res,
                        const expected_t* want, size_t nsub, bool_t weighted)
{
  static int32_t pairs[4 * MAX_ENTRIES][2], s[4 * MAX_ENTRIES], d[4 * MAX_ENTRIES];
  static float w[4 * MAX_ENTRIES];
  int64_t off[8], at = 0;
  CHECK(nsub + 1 <= 8, "too many subgraphs for this client");
  for (size_t k = 0; k < nsub; ++k) {
    size_t n = 2 * want[k].ne;
    for (size_t i = 0; i < want[k].ne; ++i) {
      pairs[at + 2 * i][0]     = want[k].u[i];
      pairs[at + 2 * i][1]     = want[k].v[i];
      pairs[at + 2 * i + 1][0] = want[k].v[i];
      pairs[at + 2 * i + 1][1] = want[k].u[i];
    }
    qsort(pairs + at, n, sizeof(pairs[0]), by_pair);
    at += (int64_t)n;
  }
  size_t total = (size_t)at;
  if (copy_back(h, cugraph_induced_subgraph_get_subgraph_offsets(res), off, nsub + 1, INT64)) return 1;
  at = 0;
  for (size_t k = 0; k <= nsub; ++k) {
    CHECK(off[k] == at, "offsets[%zu] = %lld, expected %lld", k, (long long)off[k], (long long)at);
    if (k < nsub) at += 2 * (int64_t)want[k].ne;
  }
  if (copy_back(h, cugraph_induced_subgraph_get_sources(res), s, total, INT32)) return 1;
  if (copy_back(h, cugraph_induced_subgraph_get_destinations(res), d, total, INT32)) return 1;
  for (size_t i = 0; i < total; ++i)
    CHECK(s[i] == pairs[i][0] && d[i] == pairs[i][1], "edge %zu = (%d, %d), expected (%d, %d)", i, s[i], d[i],
          pairs[i][0], pairs[i][1]);
  cugraph_type_erased_device_array_view_t* wv = cugraph_induced_subgraph_get_edge_weights(res);
  if (weighted) {
    if (copy_back(h, wv, w, total, FLOAT32)) return 1;
    for (size_t i = 0; i < total; ++i)
      CHECK(w[i] == pair_weight(s[i], d[i]), "weight %zu = %g, expected %g", i, (double)w[i],
            (double)pair_weight(s[i], d[i]));
  } else {
    CHECK(wv == NULL, "an unweighted graph gave a weights view");
  }
  return 0;
}

/* the endpoints of ne edges, each once, from the last edge to the first: an order that is not ascending */
static size_t endpoints(const int32_t* u, const int32_t* v, size_t ne, int32_t* out)
{
  int seen[KARATE_VERTICES] = {0};
  size_t n = 0;
  for (size_t i = ne; i-- > 0;) {
    if (!seen[v[i]]) { seen[v[i]] = 1; out[n++] = v[i]; }
    if (!seen[u[i]]) { seen[u[i]] = 1; out[n++] = u[i]; }
  }
  return n;
}

static const expected_t EGO0  = {EGO0_U, EGO0_V, EGO0_EDGES};
static const expected_t EGO33 = {EGO33_U, EGO33_V, EGO33_EDGES};
static const expected_t NONE  = {NULL, NULL, 0};

static int run_ego(bool_t weighted)
{
  cugraph_resource_handle_t* h = cugraph_create_resource_handle(NULL);
  CHECK(h != NULL, "resource handle");
  test_graph_t g;
  cugraph_error_t* err    = NULL;
  cugraph_error_code_t rc = make_karate(h, weighted, &g, &err);
  CHECK_RC(rc, err, "sg_graph_create");
  /* a repeated source gets its own subgraph */
  int32_t seeds[3] = {0, 33, 0};
  cugraph_type_erased_device_array_view_t* sv = NULL;
  cugraph_type_erased_device_array_t* sa      = to_device(h, seeds, 3, INT32, &sv);
  CHECK(sa != NULL, "seeds");
  cugraph_induced_subgraph_result_t* res = NULL;
  rc = cugraph_extract_ego(h, g.graph, sv, 1, FALSE, &res, &err);
  CHECK_RC(rc, err, "cugraph_extract_ego");
  expected_t want[3] = {EGO0, EGO33, EGO0};
  if (check_result(h, res, want, 3, weighted)) return 1;
  cugraph_induced_subgraph_result_free(res);
  /* radius 0: karate has no self-loop */
  rc = cugraph_extract_ego(h, g.graph, sv, 0, FALSE, &res, &err);
  CHECK_RC(rc, err, "cugraph_extract_ego, radius 0");
  expected_t none[3] = {NONE, NONE, NONE};
  if (check_result(h, res, none, 3, weighted)) return 1;
  cugraph_induced_subgraph_result_free(res);
  /* a radius beyond the diameter: the whole graph, for every source */
  rc = cugraph_extract_ego(h, g.graph, sv, 100, TRUE, &res, &err);
  CHECK_RC(rc, err, "cugraph_extract_ego, radius 100");
  expected_t whole   = {KARATE_U, KARATE_V, KARATE_EDGES};
  expected_t all3[3] = {whole, whole, whole};
  if (check_result(h, res, all3, 3, weighted)) return 1;
  cugraph_induced_subgraph_result_free(res);
  /* no sources: no edges, offsets {0} */
  cugraph_type_erased_device_array_view_t* ev = cugraph_type_erased_device_array_view_create(NULL, 0, INT32);
  rc = cugraph_extract_ego(h, g.graph, ev, 2, FALSE, &res, &err);
  CHECK_RC(rc, err, "cugraph_extract_ego, no sources");
  if (check_result(h, res, none, 0, weighted)) return 1;
  cugraph_induced_subgraph_result_free(res);
  cugraph_type_erased_device_array_view_free(ev);
  cugraph_type_erased_device_array_view_free(sv);
  cugraph_type_erased_device_array_free(sa);
  free_graph(&g);
  cugraph_free_resource_handle(h);
  return 0;
}

static int run_induced(bool_t weighted)
{
  cugraph_resource_handle_t* h = cugraph_create_resource_handle(NULL);
  CHECK(h != NULL, "resource handle");
  test_graph_t g;
  cugraph_error_t* err    = NULL;
  cugraph_error_code_t rc = make_karate(h, weighted, &g, &err);
  CHECK_RC(rc, err, "sg_graph_create");
  /* the vertex sets of the two ego nets, unsorted, with an empty set between them */
  int32_t verts[2 * KARATE_VERTICES];
  int64_t offs[4];
  offs[0] = 0;
  offs[1] = (int64_t)endpoints(EGO0_U, EGO0_V, EGO0_EDGES, verts);
  offs[2] = offs[1];
  offs[3] = offs[2] + (int64_t)endpoints(EGO33_U, EGO33_V, EGO33_EDGES, verts + offs[2]);
  CHECK(offs[1] == 17 && offs[3] - offs[2] == 18, "the ego nets have 17 and 18 vertices");
  cugraph_type_erased_device_array_view_t *vv = NULL, *ov = NULL;
  cugraph_type_erased_device_array_t* va      = to_device(h, verts, (size_t)offs[3], INT32, &vv);
  cugraph_type_erased_device_array_t* oa      = to_device(h, offs, 4, INT64, &ov);
  CHECK(va != NULL && oa != NULL, "vertex sets");
  cugraph_induced_subgraph_result_t* res = NULL;
  rc = cugraph_extract_induced_subgraph(h, g.graph, ov, vv, FALSE, &res, &err);
  CHECK_RC(rc, err, "cugraph_extract_induced_subgraph");
  expected_t want[3] = {EGO0, NONE, EGO33};
  if (check_result(h, res, want, 3, weighted)) return 1;
  cugraph_induced_subgraph_result_free(res);
  cugraph_type_erased_device_array_view_free(vv);
  cugraph_type_erased_device_array_view_free(ov);
  cugraph_type_erased_device_array_free(va);
  cugraph_type_erased_device_array_free(oa);
  free_graph(&g);
  cugraph_free_resource_handle(h);
  return 0;
}

static int test_ego(void) { return run_ego(FALSE); }
static int test_induced_subgraph(void) { return run_induced(FALSE); }
static int test_weights(void) { return run_ego(TRUE) || run_induced(TRUE); }

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

/* one induced-subgraph call that must fail with CUGRAPH_INVALID_INPUT */
static int bad_sets(const cugraph_resource_handle_t* h, cugraph_graph_t* graph, const int32_t* verts, size_t nv,
                    const int64_t* offs, size_t no, const char* needle, const char* what)
{
  cugraph_error_t* err = NULL;
  cugraph_type_erased_device_array_view_t *vv = NULL, *ov = NULL;
  cugraph_type_erased_device_array_t* va = to_device(h, verts, nv, INT32, &vv);
  cugraph_type_erased_device_array_t* oa = to_device(h, offs, no, INT64, &ov);
  CHECK(va != NULL && oa != NULL, "vertex sets");
  cugraph_error_code_t rc;
  cugraph_induced_subgraph_result_t* res = (cugraph_induced_subgraph_result_t*)&rc; /* must be reset to NULL */
  rc = cugraph_extract_induced_subgraph(h, graph, ov, vv, FALSE, &res, &err);
  if (expect_error(rc, CUGRAPH_INVALID_INPUT, &err, res, needle, what)) return 1;
  cugraph_type_erased_device_array_view_free(vv);
  cugraph_type_erased_device_array_view_free(ov);
  cugraph_type_erased_device_array_free(va);
  cugraph_type_erased_device_array_free(oa);
  return 0;
}

static int test_errors(void)
{
  cugraph_resource_handle_t* h = cugraph_create_resource_handle(NULL);
  CHECK(h != NULL, "resource handle");
  test_graph_t g;
  cugraph_error_t* err    = NULL;
  cugraph_error_code_t rc = make_karate(h, FALSE, &g, &err);
  CHECK_RC(rc, err, "sg_graph_create");
  const int32_t verts[4]  = {5, 0, 6, 4};
  const int64_t good[3]   = {0, 2, 4};
  const int64_t late[3]   = {1, 2, 4};
  const int64_t falls[3]  = {0, 3, 2};
  const int64_t short_[3] = {0, 2, 3};
  const int64_t long_[3]  = {0, 2, 5};
  const int32_t twice[4]  = {5, 0, 6, 6};
  const int32_t alien[4]  = {5, 0, 99, 4};
  if (bad_sets(h, g.graph, verts, 4, late, 3, "subgraph_offsets", "offsets that start at 1")) return 1;
  if (bad_sets(h, g.graph, verts, 4, falls, 3, "subgraph_offsets", "offsets that decrease")) return 1;
  if (bad_sets(h, g.graph, verts, 4, short_, 3, "subgraph_offsets", "offsets that end early")) return 1;
  if (bad_sets(h, g.graph, verts, 4, long_, 3, "subgraph_offsets", "offsets that end late")) return 1;
  if (bad_sets(h, g.graph, twice, 4, good, 3, "repeated", "a repeated vertex")) return 1;
  if (bad_sets(h, g.graph, alien, 4, good, 3, "not in the graph", "an unknown id")) return 1;
  /* the same vertex in two different sets is fine */
  {
    const int32_t shared[4] = {5, 0, 0, 4};
    cugraph_type_erased_device_array_view_t *vv = NULL, *ov = NULL;
    cugraph_type_erased_device_array_t* va = to_device(h, shared, 4, INT32, &vv);
    cugraph_type_erased_device_array_t* oa = to_device(h, good, 3, INT64, &ov);
    CHECK(va != NULL && oa != NULL, "vertex sets");
    cugraph_induced_subgraph_result_t* res = NULL;
    rc = cugraph_extract_induced_subgraph(h, g.graph, ov, vv, FALSE, &res, &err);
    CHECK_RC(rc, err, "a vertex shared by two sets");
    const int32_t u0[1] = {0}, v0[1] = {5}, u1[1] = {0}, v1[1] = {4};
    expected_t want[2] = {{u0, v0, 1}, {u1, v1, 1}};
    if (check_result(h, res, want, 2, FALSE)) return 1;
    cugraph_induced_subgraph_result_free(res);
    cugraph_type_erased_device_array_view_free(vv);
    cugraph_type_erased_device_array_view_free(ov);
    cugraph_type_erased_device_array_free(va);
    cugraph_type_erased_device_array_free(oa);
  }
  /* ego: an unknown source, a NULL graph, a NULL handle */
  cugraph_type_erased_device_array_view_t* sv = NULL;
  cugraph_type_erased_device_array_t* sa      = to_device(h, alien, 4, INT32, &sv);
  CHECK(sa != NULL, "sources");
  cugraph_induced_subgraph_result_t* res = (cugraph_induced_subgraph_result_t*)&rc;
  rc = cugraph_extract_ego(h, g.graph, sv, 1, FALSE, &res, &err);
  if (expect_error(rc, CUGRAPH_INVALID_INPUT, &err, res, "not in the graph", "an unknown source")) return 1;
  res = (cugraph_induced_subgraph_result_t*)&rc;
  rc  = cugraph_extract_ego(h, NULL, sv, 1, FALSE, &res, &err);
  if (expect_error(rc, CUGRAPH_INVALID_INPUT, &err, res, "graph is NULL", "ego of a NULL graph")) return 1;
  res = (cugraph_induced_subgraph_result_t*)&rc;
  rc  = cugraph_extract_induced_subgraph(h, NULL, sv, sv, FALSE, &res, &err);
  if (expect_error(rc, CUGRAPH_INVALID_INPUT, &err, res, "graph is NULL", "subgraph of a NULL graph")) return 1;
  res = (cugraph_induced_subgraph_result_t*)&rc;
  rc  = cugraph_extract_ego(NULL, g.graph, sv, 1, FALSE, &res, &err);
  if (expect_error(rc, CUGRAPH_INVALID_HANDLE, &err, res, "handle", "a NULL handle")) return 1;
  cugraph_type_erased_device_array_view_free(sv);
  cugraph_type_erased_device_array_free(sa);
  free_graph(&g);
  cugraph_free_resource_handle(h);
  return 0;
}

int main(void)
{
  struct { const char* name; int (*fn)(void); } tests[] = {
    {"ego", test_ego}, {"induced_subgraph", test_induced_subgraph}, {"ego_weights", test_weights},
    {"ego_errors", test_errors},
  };
  for (size_t i = 0; i < sizeof(tests) / sizeof(tests[0]); ++i) {
    int before = g_failures;
    tests[i].fn();
    printf("%s %s\n", g_failures == before ? "PASS" : "FAIL", tests[i].name);
  }
  printf("%d failure(s)\n", g_failures);
  return g_failures;
}
