/*
 * MI355X build extensions around the libcugraph_c boundary.
 *
 * These are the data formats either side of the hot path that the reference
 * provides through other layers (RAFT's R-MAT generator behind
 * cugraph.generators.rmat, cudf-based symmetrize/dedup behind
 * cugraph.Graph.from_cudf_edgelist) plus measurement hooks.  Nothing here is
 * needed by a caller that only uses the reference ABI.
 */
#pragma once
#include <cugraph_c/algorithms.h>

#ifdef __cplusplus
extern "C" {
#endif

/*
 * Counter-based Graph500 R-MAT edge generator (definition in oracle/rmat.py;
 * role of the reference cpp/src/generators/generate_rmat_edgelist.cu:36-103).
 * Edges [first_edge, first_edge + num_edges) of the stream for `seed`.
 * vertex_dtype: INT32 or INT64.
 */
cugraph_error_code_t cugraph_amd_generate_rmat_edgelist(const cugraph_resource_handle_t* handle,
                                                        size_t scale,
                                                        size_t num_edges,
                                                        double a,
                                                        double b,
                                                        double c,
                                                        uint64_t seed,
                                                        bool_t clip_and_flip,
                                                        bool_t scramble_vertex_ids,
                                                        size_t first_edge,
                                                        data_type_id_t vertex_dtype,
                                                        cugraph_type_erased_device_array_t** src,
                                                        cugraph_type_erased_device_array_t** dst,
                                                        cugraph_error_t** error);

/* Uniform [0,1) edge weights, 24-bit exact (oracle/rmat.py rmat_weights). */
cugraph_error_code_t cugraph_amd_generate_edge_weights(const cugraph_resource_handle_t* handle,
                                                       size_t num_edges,
                                                       uint64_t seed,
                                                       size_t first_edge,
                                                       data_type_id_t weight_dtype,
                                                       cugraph_type_erased_device_array_t** weights,
                                                       cugraph_error_t** error);

/*
 * cugraph.Graph edge-list preprocessing on the device
 * (python/cugraph/cugraph/structure/symmetrize.py:78-93): optionally append
 * reversed edges, then drop duplicate (src, dst) pairs keeping the minimum
 * weight.  Output is sorted by (src, dst).  weights may be NULL.
 */
cugraph_error_code_t cugraph_amd_symmetrize_dedup(const cugraph_resource_handle_t* handle,
                                                  const cugraph_type_erased_device_array_view_t* src,
                                                  const cugraph_type_erased_device_array_view_t* dst,
                                                  const cugraph_type_erased_device_array_view_t* weights,
                                                  bool_t symmetrize,
                                                  cugraph_type_erased_device_array_t** src_out,
                                                  cugraph_type_erased_device_array_t** dst_out,
                                                  cugraph_type_erased_device_array_t** weights_out,
                                                  cugraph_error_t** error);

/* Graph introspection (vertex count after renumbering, stored edge count). */
int64_t cugraph_amd_graph_get_number_of_vertices(const cugraph_graph_t* graph);
int64_t cugraph_amd_graph_get_number_of_edges(const cugraph_graph_t* graph);
bool_t cugraph_amd_graph_is_symmetric(const cugraph_graph_t* graph);

/*
 * Copy the graph's compressed adjacency to caller device buffers (for tests):
 * transposed=FALSE gives CSR (out-edges), TRUE gives CSC (in-edges), in the
 * graph's internal (renumbered) ids.  Pass NULL to query sizes only.
 */
cugraph_error_code_t cugraph_amd_graph_get_adjacency(const cugraph_resource_handle_t* handle,
                                                     cugraph_graph_t* graph,
                                                     bool_t transposed,
                                                     cugraph_type_erased_device_array_t** offsets,
                                                     cugraph_type_erased_device_array_t** indices,
                                                     cugraph_type_erased_device_array_t** weights,
                                                     cugraph_error_t** error);

/*
 * Copy the graph's per-vertex out-weight sums (weight_t[V], internal order; the
 * out-degree for unweighted graphs) -- compute_out_weight_sums of
 * pagerank_impl.cuh:158-164, as PageRank computes and caches them -- to a new
 * device array (for tests).
 */
cugraph_error_code_t cugraph_amd_graph_get_out_weight_sums(const cugraph_resource_handle_t* handle,
                                                           cugraph_graph_t* graph,
                                                           cugraph_type_erased_device_array_t** sums,
                                                           cugraph_error_t** error);

/*
 * Copy n device array views (dst[i] <- src[i], same type and size) with one
 * stream synchronize at the end: the batched form of
 * cugraph_type_erased_device_array_view_copy (array.h) for result extraction.
 */
cugraph_error_code_t cugraph_amd_device_array_views_copy(const cugraph_resource_handle_t* handle,
                                                         size_t n,
                                                         cugraph_type_erased_device_array_view_t* const* dst,
                                                         const cugraph_type_erased_device_array_view_t* const* src,
                                                         cugraph_error_t** error);

/*
 * Measurement hooks.  When profiling is on, algorithms record HIP events
 * around every launch of their dominant kernel (on the handle's stream) and
 * keep the total; stats are per handle and reset by each algorithm call.
 */
void cugraph_amd_set_profiling(cugraph_resource_handle_t* handle, bool_t enable);
size_t cugraph_amd_last_iterations(const cugraph_resource_handle_t* handle);
/*
 * Measurement / A-B switches, per handle (the reference's tuning constants are
 * constexpr; these select the alternatives DESIGN.md measured, for A/B scripts and
 * the bitwise-equality tests).  Names: pr_win_bits (0 | 12 | 13 | 14 | 15), pr_packed,
 * pr_whole, pr_calib, pr_deal_global, pr_unit_w, pr_fuse, pr_enc, pr_hub, pr_band_cut (-1 | 0 | cut),
 * pr_perm (x~ layout map of symmetric unweighted single-GPU schedules: 1 | 0 | -1 by window size),
 * pr_perm_cut (first vertex the map may move, rounded up to a whole window; -1: 2^20), pr_perm_span
 * (windows per range the map permutes within: 1 window-local | n | 0 the whole tail | -1 by window size),
 * pr_runs (run rows of symmetric unweighted single-GPU schedules -- whole 64-entry rows of one destination
 * window and one source, stored as slots plus one source per row: 1 | 0 | -1 by window size; fp32 ranks
 * and 32-bit ids only, and never at 8K windows (pr_win_bits 13) nor at 4K windows with pr_enc 0: those
 * kernels have no path for such rows, 1 is then ignored and cugraph_amd_last_pagerank_runs reports 0),
 * pr_run_min (shortest run that gives such rows, at least 64; -1: the default),
 * pr_dense (dense flags on the 512-entry wave segments of a packed 16-bit schedule -- 512 real entries of one
 * window, no jump, no padding, every 64-entry row's sources rising by at most 255: 1 | 0, default 1; the
 * 16K-window kernels of 32-bit ids and fp32 ranks decode a flagged segment four rows per scan, the others
 * ignore the flag; 0 sets none; the sums are the same integers either way),
 * mg_bfs_alpha, mg_bfs_beta, mg_bfs_pipelined (1 | 0), pr_fast_build, pr_share_div (0 | n),
 * mg_chunks, bfs_alpha, bfs_beta, bfs_probe_vec, bfs_head, bfs_res_grid,
 * bfs_probe_grid, bfs_td_cap, louvain_hash, louvain_big_hash, louvain_big_cap,
 * louvain_big_maxdeg, louvain_wide_keys, sssp_delta (0 | scale: delta = scale * average weight /
 * average degree), sssp_pull (0 by size | -1 never | n), wcc_sample (neighbours linked per vertex before
 * the giant component is guessed, 0: none), tc_path (triangle count: 0 thread or wave per oriented edge by
 * row size | 1 always a thread | 2 always a wave), core_scan (core number: 0 the scan of a level reads every
 * vertex | 1 it reads the compacted list of the vertices not yet peeled), sim_path (similarity: 0 a pair
 * goes to a thread, a wave or the split tier by its row sizes | 1 always a thread | 2 always a wave | 3 always
 * the split tier), sim_split_min (similarity: a pair whose shorter row has at least this many entries is cut
 * into segments, a wave each; at least 1), two_hop_budget (two-hop neighbours: walks expanded and sorted per
 * batch of source rows, a row above it goes through a V-bit map; at least 1), sample_seed (neighbour sampling and
 * random walks: the seed of the draw defined in cugraph_c/sampling_algorithms.h, an integer in [0, 2^53), default
 * 0; the one of these options that changes a result), sample_path (neighbour sampling without replacement: 0 the
 * Floyd sampler of a slot goes to a thread or a wave by the fan-out | 1 always a thread | 2 always a wave; the
 * sample is the same under all three), bc_batch (betweenness: sources per batch, one per lane of a wave, an
 * integer in [1, 64], default 64; the state is vertices x batch x 20 bytes and the batch is halved while that
 * does not fit in free device memory), bc_row_split (betweenness: a row above this many entries is cut into
 * segments of that many, a wave each; a multiple of 64, at least 64, default 2048; neither option changes a bit
 * of a vertex score, and bc_row_split none of an edge score), kt_path (k-truss: 0 a frontier edge of the peel and
 * an edge of the support pass go to a thread, a wave or the split tier by their row sizes | 1 always a thread |
 * 2 always a wave; the result, its order included, is the same under all three), sg_path (induced subgraphs and ego
 * nets: 0 the row of a (subgraph, member vertex) goes to a thread, a wave or the split tier by its length | 1 always
 * a thread | 2 always a wave), sg_split_min (the same extraction: a row of at least this many entries is cut into
 * segments of 1024 entries, a wave each; an integer, at least 1, default 64; read with sg_path 0 only),
 * ego_budget (ego nets: candidate keys expanded and sorted per batch of whole sources' hops, a source whose hop
 * alone exceeds it goes through a V-bit map; an integer, at least 1, default 2^26); the three change no byte of a
 * result, its order included; "defaults" resets them all.  Booleans
 * are 0 / 1.  Unknown names: CUGRAPH_INVALID_INPUT.
 */
cugraph_error_code_t cugraph_amd_set_option(cugraph_resource_handle_t* handle, const char* name, double value,
                                            cugraph_error_t** error);
double cugraph_amd_last_hot_kernel_ms(const cugraph_resource_handle_t* handle);
/* After cugraph_extract_induced_subgraph / cugraph_extract_ego, with or without profiling: the segments the
 * extraction's split tier cut hub rows into (0: no row went there). */
size_t cugraph_amd_last_hot_kernel_launches(const cugraph_resource_handle_t* handle);
/* PageRank (single GPU): the push schedule of the last call -- its packed 16-bit stream entries (jumps and
 * padding included; 0 for 32-bit entries or the pull path) and the vertices whose x~ its layout map moves
 * (0: no map) */
void cugraph_amd_last_pagerank_schedule(const cugraph_resource_handle_t* handle, int64_t* stream_entries,
                                        int64_t* permuted_vertices);
/* PageRank (single GPU): the run rows of the last call's push schedule (64 entries of one source each;
 * rows that only pad a window are not counted) and the entries they hold (64 x rows); 0, 0 without them.
 * These entries are not part of cugraph_amd_last_pagerank_schedule's packed stream. */
void cugraph_amd_last_pagerank_runs(const cugraph_resource_handle_t* handle, int64_t* run_rows, int64_t* run_entries);
/* PageRank (single GPU): the 512-entry wave segments of the last call's packed 16-bit stream that carry the
 * dense flag (option pr_dense), and all of its segments (run rows' segments not counted); 0, 0 for the other
 * entry formats or the pull path. */
void cugraph_amd_last_pagerank_dense(const cugraph_resource_handle_t* handle, int64_t* dense_segments,
                                     int64_t* packed_segments);
/* BFS: edges examined, levels, top-down/bottom-up steps of the last call */
size_t cugraph_amd_last_bfs_levels(const cugraph_resource_handle_t* handle);
size_t cugraph_amd_last_bfs_bottom_up_steps(const cugraph_resource_handle_t* handle);
/* Louvain: levels of the last call */
size_t cugraph_amd_last_louvain_levels(const cugraph_resource_handle_t* handle);
/* Multi-GPU Louvain: average bytes this rank sent per local-move sweep (cluster
 * lookups, weight deltas, ghost updates) in the last call; 0 on one GPU */
double cugraph_amd_last_louvain_sweep_bytes(const cugraph_resource_handle_t* handle);
/* Multi-GPU Louvain: this rank's level-0 share of the 1D partition in the last call --
 * its edges (the rows it owns) and its ghosts (distinct destinations owned elsewhere,
 * whose clusters it mirrors); 0 and 0 on one GPU */
void cugraph_amd_last_louvain_partition(const cugraph_resource_handle_t* handle, int64_t* local_edges,
                                        int64_t* ghosts);
/* Louvain dendrogram (the reference C++ API returns Dendrogram<vertex_t>,
 * louvain_impl.cuh:280-301; the C ABI only exposes the flattened clustering).
 * Level i holds the cluster of every level-i vertex this rank owns, in global-id
 * order (a rank's level-i vertices are one contiguous id range, ranks in order);
 * its values are level-(i+1) vertex ids.  The view lives as long as the result. */
size_t cugraph_amd_heirarchical_clustering_result_get_num_levels(cugraph_heirarchical_clustering_result_t* result);
cugraph_type_erased_device_array_view_t* cugraph_amd_heirarchical_clustering_result_get_level(
  cugraph_heirarchical_clustering_result_t* result, size_t level);

/* Neighbour sampling: how often each returned (source, destination, index) triple was drawn, a device array
 * of the graph's edge type aligned with cugraph_sample_result_get_sources.  The reference computes these
 * counts and offers no working getter for them (its cugraph_sample_result_get_counts is never set on this
 * path).  For a result of cugraph_test_sample_result_create: the counts it was given.  The view is freed
 * by the caller and lives as long as the result. */
cugraph_type_erased_device_array_view_t* cugraph_amd_sample_result_get_counts(const cugraph_sample_result_t* result);

/* Return every cached HBM block of libcugraph_c's caching allocator to the driver
 * (synchronises the device).  Returns the bytes released.  The reference's
 * equivalent is releasing its RMM pool. */
size_t cugraph_amd_trim_device_cache(void);

/* The caching allocator's counters since the process started: out[0] driver
 * allocations (hipMalloc), out[1] their bytes, out[2] the seconds spent in them,
 * out[3] out-of-memory trims (every cached block released, then one retry),
 * out[4] bytes cached now.  Measurement aid. */
void cugraph_amd_allocator_stats(double* out);

/* Measured HBM ceiling: a 16-B-per-lane grid-stride copy of `bytes` (nontemporal
 * loads and stores), `reps` launches timed with HIP events on the handle's stream.
 * Returns (read + write bytes) / time in GB/s, or a negative value on error. */
double cugraph_amd_measure_copy_bandwidth(const cugraph_resource_handle_t* handle, size_t bytes, int reps);

/* Library build string, e.g. "cugraph-forked_amd gfx950 <date>". */
const char* cugraph_amd_version(void);

#ifdef __cplusplus
}
#endif
