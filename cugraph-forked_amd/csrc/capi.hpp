// Internal representations behind the opaque libcugraph_c handles (MI355X build).
//
// Layout mirrors what the reference keeps behind the same opaque pointers
// (cpp/src/c_api/{resource_handle,array,error,graph}.hpp) but the storage is our
// own: a graph owns its compressed adjacency in one or both orientations
// (out-edges "CSR", in-edges "CSC"; one shared object when the graph is
// symmetric), the number map, and lazily-built per-orientation scheduling data
// for the degree-binned kernels.
#pragma once

#include "common.hpp"

#include <cugraph_c/algorithms.h>

#include <memory>
#include <string>
#include <cstring>
#include <vector>

namespace cgx {

struct mg_graph_t;  // mg_graph.hpp
struct mg_context;  // comm.hpp (multi-GPU); nullptr for single GPU

// Measurement / A-B switches of the kernels, per handle (cugraph_amd_set_option,
// include/cugraph_amd/ext.h).  The defaults are the production choices; the other
// values select the measured alternatives DESIGN.md records, for the A/B scripts and
// the bitwise-equality tests.  Nothing here is read from the environment.
// Schedule-time switches (pr_win_bits, pr_packed, pr_whole) apply to schedules built
// after they are set: the push schedule is cached on the graph.
struct tuning_t {
  int pr_win_bits      = 0;     // 0: by size (push_win_bits); 12 / 13 / 14 / 15 force 4K / 8K / 16K / 32K windows
                                // (15: single-GPU symmetric unweighted schedules only, else 14)
  bool pr_packed       = true;  // 16-bit entries for unweighted graphs (else 32-bit)
  bool pr_whole        = true;  // windows summed by one item are stored, not added
  bool pr_calib        = true;  // measured-cost queues after the first launch
  bool pr_deal_global  = false; // measured items in one longest-first queue instead of 8 XCD queues
  bool pr_unit_w       = true;  // all-ones weights run the unweighted push
  bool pr_fuse         = true;  // apply fused into the 16K-window push
  bool pr_enc          = true;  // x~ as fixed-point words (fp32 single GPU)
  bool pr_hub          = true;  // hub x~ staged in LDS (16K windows)
  int64_t pr_band_cut  = -1;    // banded push source cut (-1: by size, 0: no bands)
  int pr_perm          = -1;    // x~ layout map of the symmetric packed schedule (pagerank.hip build_x_layout):
                                // -1 by window size (push_perm_default), 1 on, 0 off
  int64_t pr_perm_cut  = -1;    // first vertex the map may move (-1: 2^20), rounded up to a whole window
  int pr_perm_span     = -1;    // windows per range the map permutes within (-1: by window size, 0: the whole tail)
  int pr_runs          = -1;    // run rows of the symmetric packed schedule (pagerank.hip k_run_flags): whole
                                // 64-entry rows of one (window, source) stored as slots + one source; -1 by
                                // window size (push_runs_on), 1 on, 0 off
  int64_t pr_run_min   = -1;    // shortest run that gives run rows (-1: kRunMin; at least 64)
  bool pr_dense        = true;  // dense flags on the packed schedule's wave segments (pagerank.hip kSegDense):
                                // a flagged segment is decoded four rows per scan; 0 sets no flag
  int pr_share_div     = 0;     // items per push block on average (0: kShareDiv); windows above 1.5x are shared
  bool pr_fast_build   = true;  // symmetric unweighted schedules through one-word keys (else the general build)
  int mg_chunks        = 0;     // MG overlap chunks (0: one chunk, no overlap)
  double bfs_alpha     = 40.0;  // direction switch (Beamer's alpha / beta)
  double bfs_beta      = 64.0;
  double mg_bfs_alpha  = 40.0;  // multi-GPU BFS direction switch (mg_bfs.hip; one-rank RMAT-24: 40 / 64
  double mg_bfs_beta   = 64.0;  // 2.92 vs Beamer's 14 / 24 3.20 ms per traversal)
  int mg_bfs_pipelined = 1;     // MG BFS: bottom-up levels enqueued a level ahead, counts read late (mg_bfs.hip bu_state)
  bool bfs_probe_vec   = true;  // bottom-up probe by 16-byte loads
  bool bfs_head        = true;  // bottom-up probe's head table
  int bfs_res_grid     = 1024;  // residual scan blocks
  int bfs_probe_grid   = 4096;  // probe blocks
  int64_t bfs_td_cap   = 1024;  // top-down blocks per degree-class segment
  bool louvain_hash    = true;  // LDS-hash local move (else sort + reduce-by-key)
  bool louvain_big_hash = true; // heavy rows on the LDS passes (else the sort path)
  int louvain_big_cap  = 0;     // (row, bucket) table cap below the built-in one (tests of the fallback)
  int64_t louvain_big_maxdeg = 0;  // heavy rows above this degree on the sort path (0: the table limit)
  bool louvain_wide_keys = false;  // 64-bit hash keys below 2^24 ids (tests)
  double sssp_delta    = 0;     // SSSP delta = sssp_delta * average weight / average degree (0: sssp.hip kDeltaScale)
  int sssp_pull        = 0;     // SSSP dense rounds by pull: 0 by size (sssp.hip kPullDiv), -1 never, n: list > part / n
  int wcc_sample       = 2;     // WCC: neighbours linked per vertex before the giant component is guessed
                                // (wcc.hip; 0: no guess, every row fully linked)
  int tc_path          = 0;     // triangle count: 0 an oriented edge goes to a thread or a wave by its row sizes,
                                // 1 every edge to a thread, 2 every edge to a wave (triangle_count.hip)
  int core_scan        = 0;     // core number: 0 a level's scan reads every vertex, 1 it reads the compacted list of
                                // the vertices not yet peeled (core_number.hip; 0 measured faster)
  int sim_path         = 0;     // similarity: 0 a pair goes to a thread, a wave or the split tier by its row sizes,
                                // 1 every pair to a thread, 2 every pair to a wave, 3 every pair through the split
                                // tier (similarity.hip)
  int64_t sim_split_min = 4096; // similarity: a pair whose shorter row has at least this many entries is cut into
                                // segments, a wave each (similarity.hip; at least 1)
  int64_t two_hop_budget = (int64_t)1 << 26;  // two-hop neighbours: walks expanded and sorted per batch of source
                                // rows; a row above it goes through a V-bit map (two_hop.hip; 2^26 measured)
  uint64_t sample_seed = 0;     // neighbour sampling and random walks: the seed of sample.hpp's draw (below 2^53; the
                                // reference's ABI has no seed argument and its C API passes 0)
  int sample_path      = 0;     // neighbour sampling without replacement: 0 a slot's Floyd sampler goes to a thread or
                                // a wave by the fan-out, 1 always a thread, 2 always a wave (sampling.hip)
  int bc_batch         = 64;    // betweenness: sources per batch, one per lane of a wave (1 .. 64; halved while the
                                // V x batch x 20 bytes of state do not fit; betweenness.hip)
  int64_t bc_row_split = 2048;  // betweenness: a row above this many entries is cut into segments of that many, a
                                // wave each (a multiple of 64, the block of a row's sum: the cut changes no bit)
  int kt_path          = 0;     // k-truss: 0 a frontier edge (and an edge of the support pass) goes to a thread, a wave
                                // or the split tier by its row sizes, 1 every one to a thread, 2 every one to a wave
                                // (k_truss.hip)
  int sg_path          = 0;     // induced subgraph / ego net extraction: 0 a (subgraph, member) row goes to a thread, a
                                // wave or the split tier by its length, 1 every row to a thread, 2 every row to a
                                // wave (subgraph.hip)
  int64_t sg_split_min = 64;    // extraction: a row of at least this many entries is cut into segments of
                                // kSgSegLen entries, a wave each (sg_path 0 only; at least 1)
  int64_t ego_budget   = (int64_t)1 << 26;  // ego nets: candidate keys expanded and sorted per batch of whole source
                                // slots; a slot whose hop alone exceeds it goes through a V-bit map (subgraph.hip)
};

struct handle_t {
  int device         = 0;
  hipStream_t stream = nullptr;
  mg_context* mg     = nullptr;
  bool profiling     = false;
  tuning_t tune;
  // statistics of the last algorithm call (see include/cugraph_amd/ext.h)
  size_t last_iterations     = 0;
  double last_hot_ms         = 0;
  size_t last_hot_launches   = 0;
  int64_t last_pr_stream     = 0;  // single-GPU PageRank: the push schedule's packed stream entries,
  int64_t last_pr_permuted   = 0;  // and the vertices its x~ layout map moves (0: no map)
  int64_t last_pr_run_rows    = 0;  // its run rows (64 entries of one source each, padding rows not counted)
  int64_t last_pr_run_entries = 0;  // and the entries they hold
  int64_t last_pr_dense_segs  = 0;  // its packed stream's wave segments flagged dense,
  int64_t last_pr_packed_segs = 0;  // of this many (run units' segments not counted)
  size_t last_bfs_levels    = 0;
  size_t last_bfs_bottom_up  = 0;
  size_t last_louvain_levels = 0;
  double last_louvain_sweep_bytes = 0;  // MG: average bytes sent per sweep by this rank
  int64_t last_louvain_local_edges = 0;  // MG: this rank's level-0 edges (rows it owns)
  int64_t last_louvain_ghosts      = 0;  // MG: its level-0 ghosts (distinct remote destinations)
  // Host-pinned scratch for the per-level / per-chunk device state reads and a pool
  // of profiling events, both kept for the handle's lifetime: hipHostMalloc +
  // hipHostFree per call measured ~250 us of host stall per BFS traversal.
  void* pinned = nullptr;
  std::vector<hipEvent_t> events;
  template <typename T>
  T* pinned_as()
  {
    static_assert(sizeof(T) <= kPinnedBytes, "pinned scratch too small");
    if (!pinned) HIP_CHECK(hipHostMalloc(&pinned, kPinnedBytes, hipHostMallocDefault));
    return static_cast<T*>(pinned);
  }
  // Coherent (fine-grained) pinned block the host polls while the stream runs on:
  // a kernel publishes values and then a sequence number with system-scope stores.
  // It must stay hipHostMallocCoherent (uncached): bfs.hip k_publish_seq orders the
  // words before the sequence number with a vmcnt wait only, no release.
  void* polled = nullptr;
  template <typename T>
  T* polled_as()
  {
    static_assert(sizeof(T) <= kPinnedBytes, "polled scratch too small");
    if (!polled) {
      HIP_CHECK(hipHostMalloc(&polled, kPinnedBytes, hipHostMallocCoherent));
      std::memset(polled, 0, kPinnedBytes);
    }
    return static_cast<T*>(polled);
  }
  hipEvent_t event(size_t i)  // the i-th pooled event (created on first use)
  {
    while (events.size() <= i) {
      hipEvent_t e;
      HIP_CHECK(hipEventCreate(&e));
      events.push_back(e);
    }
    return events[i];
  }
  static constexpr size_t kPinnedBytes = 4096;
  ~handle_t()
  {
    if (pinned) (void)hipHostFree(pinned);
    if (polled) (void)hipHostFree(polled);
    for (auto e : events) (void)hipEventDestroy(e);
  }
};

// every algorithm call starts its statistics from zero
inline void reset_hot(handle_t& h)
{
  h.last_iterations   = 0;
  h.last_hot_ms       = 0;
  h.last_hot_launches = 0;
}

// Profiling: pairs of pooled HIP events around the hot launches, summed into last_hot_ms.
// One pair spans a whole chunk of launches (PageRank: an event between every two
// iterations cost a ~10 us queue gap per iteration, and chunk time / iterations run is the
// result, so the no-op launches after convergence in the last chunk count against the
// kernels).  fold() adds the finished intervals to the total and hands their events back,
// so a caller that folds after every chunk's host synchronisation (core number: one
// interval per round) holds no more events than a chunk records.  With profiling off
// nothing is recorded and nothing synchronises.
struct chunk_timer {
  handle_t& h;
  hipStream_t s;
  size_t live     = 0;  // events recorded since the last fold
  double total_ms = 0;
  void begin()
  {
    if (h.profiling) HIP_CHECK(hipEventRecord(h.event(live), s));
  }
  void end()
  {
    if (!h.profiling) return;
    HIP_CHECK(hipEventRecord(h.event(live + 1), s));
    live += 2;
  }
  void fold()
  {
    if (!live) return;
    HIP_CHECK(hipEventSynchronize(h.event(live - 1)));  // returns at once after a host synchronisation
    for (size_t i = 0; i < live; i += 2) {
      float ms = 0;
      HIP_CHECK(hipEventElapsedTime(&ms, h.event(i), h.event(i + 1)));
      total_ms += ms;
    }
    live = 0;
  }
  void report(size_t launches)  // launches: what last_hot_launches counts for this algorithm
  {
    if (!h.profiling) return;
    fold();
    h.last_hot_ms       = total_ms;
    h.last_hot_launches = launches;
  }
};

struct array_view_t {  // reference c_api/array.hpp:30-35
  void* data           = nullptr;
  size_t size          = 0;
  size_t num_bytes     = 0;
  data_type_id_t type  = INT32;
  template <typename T>
  T* as() const
  {
    return static_cast<T*>(data);
  }
};

struct device_array_t {
  buffer buf;
  size_t size         = 0;
  data_type_id_t type = INT32;
  device_array_t(size_t n, data_type_id_t t, hipStream_t s) : buf(n * dtype_size(t), s), size(n), type(t) {}
  array_view_t view() const { return array_view_t{buf.data(), size, size * dtype_size(type), type}; }
};

struct host_array_t {
  std::vector<std::byte> data;
  size_t size         = 0;
  data_type_id_t type = INT32;
};

struct err_t {
  std::string message;
};

// PageRank windowed-push schedule of one edge set (pagerank.hip): packed entries
// sorted by (destination window, source), work units and fixed-point accumulators
struct pr_push_t {
  bool built = false;
  bool ok    = false;  // ids and edge positions fit the 32-bit packing
  int win_bits = 12;   // destination window = 2^win_bits consecutive rows
  buffer ent;          // uint32[E + unit]: (source - unit's first source) << win_bits | (row - window base)
  buffer ew;           // weight_t[E + unit] for weighted graphs
  bool packed = false; // 16-bit entries (unweighted): ent16 + seg_base instead of ent
  buffer ent16;        // uint16[E' + unit]: delta << win_bits | slot, or a source jump
  buffer seg_base;     // uint32[nunits * 16]: running source before each 512-entry wave segment
  buffer units;        // push_unit[nunits], in (window, source) order
  int64_t nunits = 0;
  buffer acc;          // u64[nacc] fixed-point sums by row; windows stored whole by one item are
                       // overwritten each iteration, the others (win_multi) are cleared by the apply
  int64_t nacc = 0;
  buffer items;        // int64[nitems + 1]: first unit of every item (a window or a share of one)
  buffer queue;        // int64[nitems]: item ids of queue 0, 1, ..., 7
  std::vector<int64_t> qoff;  // queue q = queue[qoff[q], qoff[q + 1])
  int64_t nitems = 0;
  int64_t nwin   = 0;
  buffer tile_ctr;     // uint32 queue heads (128 B apart); zero between iterations
  buffer win_multi;    // uint8[nwin]: 1 = window summed by several items (flushes add), 0 = one item stores it
  // fused apply (pagerank.hip fused_finish): items per window, windows without items
  buffer win_items;       // uint32[nwin]
  buffer win_left;        // uint32[nwin]: win_items between iterations
  buffer empty_wins;      // int64[nempty]
  int64_t nempty = 0, nwin_items = 0;
  // measured-cost queues (pagerank.hip calibrate_queues): the first launch on a schedule
  // records every item's duration, the host then re-deals the items by those costs
  buffer item_ticks;      // uint32[nitems], s_memrealtime ticks
  int calib = 0;          // 0 not yet, 1 recorded (re-deal pending), 2 done or off
  // source bands (pagerank.hip, banded push): every window's entries are split at a
  // source cut into two virtual windows, vw = band * nwin_real + window; the stream
  // and the items are band-major, so the whole grid sweeps the low sources first
  bool bands = false;
  int64_t nwin_real = 0;  // real windows (nwin counts the virtual ones)
  buffer win_pub;         // uint32[nwin_real]: items of the window that published this iteration
  buffer carry;           // uint32[nacc]: 32K windows' carry words (push_args::carry), zero between iterations
  // x~ layout (pagerank.hip build_x_layout; symmetric packed single-GPU schedules): x~ of vertex
  // v lives at pos[v], pos[v] = v below perm_cut; sources in the stream are positions
  buffer pos;             // uint32[V], empty: x~[v] at v
  int64_t perm_cut = 0;   // first vertex that may move (a window multiple), 0 without a map
  int64_t stream_len = 0; // packed 16-bit stream entries, padding included (0: 32-bit entries)
  // run rows (pagerank.hip k_run_flags): whole 64-entry rows of one (window, source) leave the
  // packed stream; their slots follow it in ent16, in units of their own (push_unit::base < 0)
  buffer run_src;          // uint32[rows + a unit's]: the source of every row, kRunPad on padding rows
  int64_t run_rows = 0, run_entries = 0;
  // wave segments of the packed stream, and those of them flagged dense (pagerank.hip kSegDense)
  int64_t packed_segs = 0, dense_segs = 0;
  // the last call's iteration count (plain calls: no guess, no personalization) with
  // its alpha and epsilon: the first chunk of the next such call (pagerank.hip)
  int last_iters = 0;
  double last_alpha = -1.0, last_eps = -1.0;
};

// One orientation of the adjacency: majors (rows) -> minors (indices).
constexpr int64_t kIdxPad = 16;  // entries past the end of adjacency_t::indices (vector loads)

struct adjacency_t {
  buffer offsets;  // edge_t[V+1]
  buffer indices;  // vertex_t[E], ascending within each row (+ kIdxPad entries when idx_padded)
  buffer weights;  // weight_t[E] or empty
  bool idx_padded = false;
  // degree-binned schedule (built on first use, see schedule.hpp)
  bool degree_sorted = false;  // majors already in descending-degree order (renumbered build)
  int64_t max_degree = -1;     // cached on first use (BFS), -1 = not known yet
  int unit_weights   = -1;     // weighted: 1 if every weight is exactly 1 (PageRank: unweighted push), -1 unknown
  bool sched_valid   = false;
  buffer order;                         // vertex_t[V] processing order if !degree_sorted
  std::vector<int64_t> bin_begin;       // positions (in processing order) where each bin starts
  buffer items;                         // work items for the SpMV-like kernels
  int64_t num_items = 0;
  // BFS bottom-up probe's head table: 16 B per vertex (16 * kHeadQ, bfs.hip k_bfs_head; RMAT-24 142 MB),
  // built on the first direction-optimising BFS and kept for the adjacency's lifetime like pr and
  // items (freed with the graph; trim_device_cache returns only the allocator's free blocks)
  buffer bfs_head;
  double wsum = -1;  // SSSP: sum of the weights (delta), cached on first use; -1 = not known yet
  // SSSP (sssp.hip): the light (w < delta) and heavy edges as two CSRs, with each part's
  // chunk rows, for one delta
  double sssp_delta = -1;
  int64_t sssp_eL = 0, sssp_eH = 0;
  buffer sssp_offL, sssp_offH, sssp_idxL, sssp_wL, sssp_idxH, sssp_wH, sssp_crowL, sssp_crowH;
  // Triangle counting (triangle_count.hip): the rows oriented towards the higher-ranked endpoint, built on
  // the first call.  tc_ooff is the prefix sum of the oriented row sizes; a degree-sorted adjacency needs
  // nothing else (the oriented row of u is the head of its row, the ids below u), any other one keeps the
  // oriented entries compacted in tc_oidx
  int64_t tc_edges = -1;  // oriented edges, -1 = not built yet
  buffer tc_ooff;         // edge_t[V + 1]
  buffer tc_oidx;         // vertex_t[tc_edges], ascending within each row (!degree_sorted only)
  // Similarity (similarity.hip): distinct ids per row, built on the first call
  bool sim_deg_valid = false;
  buffer sim_deg;         // edge_t[V]
  // Biased random walks (random_walks.hip): every row's inclusive prefix sum of its weights, in double, added
  // left to right; built on the first call
  bool cum_valid = false;
  buffer cum;             // double[E]
  // k-truss (k_truss.hip): the simple rows (the adjacency's own when it holds no loop and no repeat, else a
  // cleaned copy), one id per undirected edge at every position of them, and every edge's triangle support;
  // none of it depends on k.  Built on the first call
  bool kt_valid = false;
  bool kt_clean = true;      // no loop, no repeat: kt_off / kt_idx / kt_orig stay empty
  int64_t kt_edges = 0;      // undirected edges of the simple graph
  int64_t kt_heavy = 0;      // those whose two rows both have k_truss.hip kKtSplitMin entries or more
  buffer kt_off;             // edge_t[V + 1]   cleaned copy: offsets,
  buffer kt_idx;             // vertex_t[...]   entries,
  buffer kt_orig;            // edge_t[...]     and the stored position each entry came from
  buffer kt_eid;             // edge_t[entries of the simple rows]: the edge's id
  buffer kt_esrc;            // vertex_t[kt_edges]: the smaller endpoint u of edge (u, v), u < v
  buffer kt_epos;            // edge_t[kt_edges]: the position of v in u's simple row
  buffer kt_sup;             // int32[kt_edges]: |N(u) & N(v)|
  pr_push_t pr;  // PageRank windowed-push schedule (pagerank.hip), built on first use
};

struct graph_t {
  data_type_id_t vertex_type = INT32;
  data_type_id_t edge_type   = INT32;
  data_type_id_t weight_type = FLOAT32;
  bool store_transposed      = false;  // orientation the user asked for (the reference mutates it)
  bool symmetric             = false;
  bool multigraph            = false;
  bool weighted              = false;
  bool renumbered            = false;
  bool multi_gpu             = false;
  int64_t num_vertices       = 0;
  int64_t num_edges          = 0;
  std::shared_ptr<adjacency_t> out;  // CSR (may be null until built)
  std::shared_ptr<adjacency_t> in;   // CSC (== out when symmetric)
  buffer number_map;                 // vertex_t[V]: internal -> external id
  // cached external -> internal lookup (sorted external ids + their internal ids)
  bool ext_lookup_valid = false;
  buffer ext_sorted;    // vertex_t[V]
  buffer ext_internal;  // vertex_t[V]
  // cached per-vertex out-weight sums (weight_t[V]) and their dangling mask source
  bool outw_valid = false;
  buffer outw;
  std::shared_ptr<mg_graph_t> mg;  // multi-GPU partition state (mg_graph.hpp); null for SG
};

struct centrality_result_t {
  std::unique_ptr<device_array_t> vertices;
  std::unique_ptr<device_array_t> values;
};

struct edge_centrality_result_t {  // edge betweenness: one entry per stored edge, in out-edge order
  std::unique_ptr<device_array_t> src;
  std::unique_ptr<device_array_t> dst;
  std::unique_ptr<device_array_t> values;  // FLOAT64
};

struct labeling_result_t {  // reference c_api/labeling_result.hpp
  std::unique_ptr<device_array_t> vertices;
  std::unique_ptr<device_array_t> labels;  // vertex type, internal ids (wcc.hip)
};

struct triangle_count_result_t {  // reference c_api/triangle_count.cpp
  std::unique_ptr<device_array_t> vertices;
  std::unique_ptr<device_array_t> counts;  // edge type
};

struct core_result_t {  // reference c_api/core_result.hpp
  std::unique_ptr<device_array_t> vertices;
  std::unique_ptr<device_array_t> core_numbers;  // edge type
};

struct k_core_result_t {  // reference c_api/core_result.hpp
  std::unique_ptr<device_array_t> src;
  std::unique_ptr<device_array_t> dst;
  std::unique_ptr<device_array_t> weights;  // null for an unweighted graph
};

// k-truss (one subgraph), induced subgraphs and ego nets (one per vertex set / source); the layout of later
// releases' c_api/induced_subgraph_result.hpp
struct induced_subgraph_result_t {
  std::unique_ptr<device_array_t> src;
  std::unique_ptr<device_array_t> dst;
  std::unique_ptr<device_array_t> weights;  // null for an unweighted graph
  std::unique_ptr<device_array_t> offsets;  // subgraphs + 1 entries, subgraph i = edges [offsets[i], offsets[i + 1]);
                                            // 8-byte values, typed INT64 (this ABI has no SIZE_T id)
};

struct vertex_pairs_t {  // reference c_api/graph_helper / vertex_pairs.hpp
  std::unique_ptr<device_array_t> first;
  std::unique_ptr<device_array_t> second;
};

struct similarity_result_t {  // reference c_api/similarity.cpp
  std::unique_ptr<device_array_t> similarity;  // weight type
};

struct sample_result_t {  // reference c_api/uniform_neighbor_sampling.cpp:31-38
  std::unique_ptr<device_array_t> src;
  std::unique_ptr<device_array_t> dst;
  std::unique_ptr<device_array_t> index;   // weight type: the edges' weight bits, ones without weights
  std::unique_ptr<device_array_t> counts;  // edge type: how often each triple was drawn (cugraph_amd_sample_result_get_counts)
  // cugraph_test_sample_result_create only: the counts it was given, on the host, for the reference's
  // host-view getter; a sample call leaves it null and that getter returns NULL
  std::unique_ptr<host_array_t> given_counts;
};

struct random_walk_result_t {  // reference c_api/random_walks.cpp:34-40
  size_t max_length = 0;
  std::unique_ptr<device_array_t> paths;    // vertex type [n x (max_length + 1)], row major, -1 after a sink
  std::unique_ptr<device_array_t> weights;  // weight type [n x max_length]; null for an unweighted graph
};

struct paths_result_t {
  std::unique_ptr<device_array_t> vertices;
  std::unique_ptr<device_array_t> distances;
  std::unique_ptr<device_array_t> predecessors;
};

struct extract_paths_result_t {
  size_t max_path_length = 0;
  std::unique_ptr<device_array_t> paths;  // [destinations x max_path_length], row major
};

struct hits_result_t {
  std::unique_ptr<device_array_t> vertices;
  std::unique_ptr<device_array_t> hubs;
  std::unique_ptr<device_array_t> authorities;
  double hub_score_differences = 0;
  size_t number_of_iterations  = 0;
};

struct clustering_result_t {
  std::unique_ptr<device_array_t> vertices;
  std::unique_ptr<device_array_t> clusters;
  double modularity = 0;
  // dendrogram (reference Dendrogram<vertex_t>, dendrogram.hpp): level i holds the
  // cluster of every level-i vertex this rank owns, in global-id order; its values
  // are level-(i+1) vertex ids (the last level: that level's cluster ids)
  std::vector<std::unique_ptr<device_array_t>> levels;
};

// ------------------------------------------------------------------ helpers
inline handle_t* H(cugraph_resource_handle_t const* h) { return reinterpret_cast<handle_t*>(const_cast<cugraph_resource_handle_t*>(h)); }
inline graph_t* G(cugraph_graph_t* g) { return reinterpret_cast<graph_t*>(g); }
inline graph_t const* G(cugraph_graph_t const* g) { return reinterpret_cast<graph_t const*>(g); }
inline array_view_t const* AV(cugraph_type_erased_device_array_view_t const* v)
{
  return reinterpret_cast<array_view_t const*>(v);
}
inline array_view_t* AV(cugraph_type_erased_device_array_view_t* v) { return reinterpret_cast<array_view_t*>(v); }

inline cugraph_type_erased_device_array_view_t* new_view(device_array_t const* a)
{
  return reinterpret_cast<cugraph_type_erased_device_array_view_t*>(new array_view_t(a->view()));
}

// Run `f` converting every exception into the reference's error protocol
// (cpp/src/c_api/utils.hpp:24-56): cgx::error keeps its code, anything else is
// CUGRAPH_UNKNOWN_ERROR; the message goes into a fresh error object.
template <typename F>
cugraph_error_code_t guarded(cugraph_error_t** error, F&& f)
{
  try {
    f();
    return CUGRAPH_SUCCESS;
  } catch (cgx::error const& e) {
    if (error) *error = reinterpret_cast<cugraph_error_t*>(new err_t{e.what()});
    return e.code;
  } catch (std::bad_alloc const& e) {
    if (error) *error = reinterpret_cast<cugraph_error_t*>(new err_t{std::string("allocation failed: ") + e.what()});
    return CUGRAPH_ALLOC_ERROR;
  } catch (std::exception const& e) {
    if (error) *error = reinterpret_cast<cugraph_error_t*>(new err_t{e.what()});
    return CUGRAPH_UNKNOWN_ERROR;
  }
}

// ------------------------------------------------------------------ shared graph services
// (graph_build.hip)
void build_sg_graph(handle_t& h, graph_t& g, array_view_t const& src, array_view_t const& dst,
                    array_view_t const* weights, bool renumber);
adjacency_t& ensure_adjacency(handle_t& h, graph_t& g, bool transposed);  // builds the other orientation
void ensure_schedule(handle_t& h, graph_t& g, adjacency_t& adj);
// external ids (device, graph vertex type) -> internal ids, in place; throws on unknown ids
void renumber_ext_to_int(handle_t& h, graph_t& g, void* ids, size_t n, bool check);
// the same lookup with no check and no host sync: ids not in the graph become -1,
// for callers that range-check the internal ids on the device anyway (BFS sources)
void renumber_ext_to_int_unchecked(handle_t& h, graph_t& g, void* ids, size_t n);
// sorted external ids + their internal ids (g.ext_sorted / g.ext_internal), renumbered graphs
void ensure_ext_lookup(handle_t& h, graph_t& g);
// internal ids -> external ids (values < 0 or >= V are left untouched), in place
void unrenumber_int_to_ext(handle_t& h, graph_t& g, void* ids, size_t n);
// copy of the number map as a result array
std::unique_ptr<device_array_t> number_map_copy(handle_t& h, graph_t& g);
// per-vertex out-weight sums in weight_t (cached on the graph)
void const* out_weight_sums(handle_t& h, graph_t& g);

// ------------------------------------------------------------------ subgraph extraction
// (subgraph.hip)  offsets: INT64 [subgraphs + 1], vertices / sources: external ids in the graph's vertex type
void run_induced_subgraph(handle_t& h, graph_t& g, array_view_t const& offsets, array_view_t const& vertices,
                          induced_subgraph_result_t& res);
void run_extract_ego(handle_t& h, graph_t& g, array_view_t const& sources, size_t radius,
                     induced_subgraph_result_t& res);

}  // namespace cgx
