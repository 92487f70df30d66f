/*
 * include/drm_hip.h -- C ABI of libdrm_hip.so, the MI355X-native drop-in for DeepReadMapper's
 * query hot path (HNSW-PQ candidate search + Smith-Waterman rerank).
 *
 * Every entry point is plain C: pointers + sizes, no C++/torch types. Return value 0 = success,
 * negative = error (message via drm_last_error(), thread-local), mirroring the reference's
 * exception + "Error: ..." convention (src/main.cpp:439-448). All citations are to the reference
 * (/root/reference, hunglongtrangithub/DeepReadMapper) unless marked [faiss].
 */
#ifndef DRM_HIP_H
#define DRM_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DRM_OK 0
#define DRM_ERR_ARG (-1)       /* bad argument (std::invalid_argument / runtime_error in reference) */
#define DRM_ERR_IO (-2)        /* file missing / unreadable                                          */
#define DRM_ERR_FORMAT (-3)    /* index file not an IndexHNSWPQ we can read                          */
#define DRM_ERR_HIP (-4)       /* HIP runtime error                                                  */
#define DRM_ERR_CANDS (-5)     /* "Not enough candidates (n < k)"  src/utils/reranker.cpp:26-29      */
#define DRM_ERR_K (-6)         /* "Final k too large..."           src/utils/post_processor.cpp:486-489 */
#define DRM_ERR_UNSUPPORTED (-7)
#define DRM_ERR_INTERNAL (-8)  /* a kernel detected broken bookkeeping (e.g. a search past its hop bound)   */

/* Threading: every handle (drm_index, drm_flat_index, drm_refs) owns mutable device scratch (visited
 * bitmaps, clear lists, queue counters, rerank workspace). A handle is single-stream: its calls must be
 * serialised in stream order (one in-flight call per handle). Concurrent work on one device uses one
 * handle per stream; multi-device fan-out (drm_multi_*) keeps one handle per device. The diagnostic
 * counters (drm_*_overflows / _fallbacks) describe the handle's most recent search. */
typedef struct drm_index drm_index; /* device-resident IndexHNSWPQ */
typedef struct drm_refs drm_refs;   /* device-resident static window table (ref_seqs) */
typedef struct drm_encoder drm_encoder; /* device-resident GRU read encoder */

typedef struct {
    int32_t d;             /* vector dimension                                  */
    int64_t ntotal;        /* number of indexed vectors                         */
    int32_t pq_M;          /* PQ sub-quantizers (M_pq)                          */
    int32_t pq_nbits;      /* bits per sub-quantizer code                       */
    int32_t M_hnsw;        /* HNSW M; level-0 degree = 2*M_hnsw                 */
    int32_t max_level;     /* HNSW max_level                                    */
    int32_t entry_point;   /* HNSW entry point                                  */
    int32_t efConstruction;
    int32_t efSearch;      /* value stored in the file                          */
    int32_t metric_type;   /* 1 = METRIC_L2 (the only one the reference builds) */
    int64_t device_bytes;  /* HBM held by the index on its device              */
    int32_t device;        /* HIP device the index lives on                     */
} drm_index_info;

typedef struct {
    int64_t nq;            /* queries searched                                       */
    int64_t ndis;          /* sum of HNSWStats.ndis  [faiss hnsw_stats]               */
    int64_t nhops;         /* sum of HNSWStats.nhops                                  */
    double kernel_ms;      /* device time of the search kernel(s) (hipEvent)          */
} drm_search_stats;

/* ---------------------------------------------------------------- runtime / errors */
const char *drm_last_error(void);
int drm_version(void); /* major*10000 + minor*100 + patch */
int drm_device_count(int *n);
int drm_set_device(int device);
/* The device's shape, read at run time (hipGetDeviceProperties): compute units, peak engine clock (kHz), HBM
 * bytes, LDS bytes per CU, architecture name. bench.py prices its issue ceilings with these. */
typedef struct {
    int32_t cu_count;
    int32_t clock_khz;
    int64_t total_mem;
    int32_t lds_per_cu;
    char arch[64];
} drm_device_props;
int drm_device_get_props(int device, drm_device_props *out);
int drm_device_sync(void);
int drm_malloc(void **ptr, size_t bytes);
int drm_free(void *ptr);
int drm_memset(void *ptr, int value, size_t bytes);
int drm_memcpy_h2d(void *dst, const void *src, size_t bytes);
/* A 64-bit checksum of nbytes of device memory (8-byte aligned): the sum, mod 2^64, over the little-endian 8-byte
 * words w_i (the last one zero-padded) of splitmix64(w_i + i * 0x9E3779B97F4A7C15). Position-dependent, so rows
 * landing at the wrong offset change it; used to verify the RCCL result gather (bench.py) and the index broadcast
 * without copying the rows to the host. It reads the buffer after all device work this process enqueued before the
 * call has finished, on any stream (a device synchronisation), then runs on `stream`, which it synchronises. No
 * reference counterpart (a tool). */
int drm_device_checksum(const void *d_ptr, int64_t nbytes, uint64_t *out, void *stream);
int drm_memcpy_d2h(void *dst, const void *src, size_t bytes);
/* A measurement tool (no reference counterpart): the latency of the search's dependent row load on this device.
 * `waves` waves (one per workgroup) each walk `hops` 384-B rows -- the lean kernel's level-0 row, 12 B per lane on
 * 32 lanes -- of a footprint_bytes table of random contents, each next row chosen by the row just read; returns the
 * device time per hop in ns (hipEvent). bench.py prices its search latency floor with it. */
int drm_device_chase_latency(int device, int64_t footprint_bytes, int32_t waves, int32_t hops, double *ns_per_load);
/* The same walk loading only the first row_lines (1..3) 128-B lines of each 384-B row (10, 21 or 32 links): prices a
 * row load gated on the row's valid link count. drm_device_chase_latency is row_lines = 3. */
int drm_device_chase_rows(int device, int64_t footprint_bytes, int32_t waves, int32_t hops, int32_t row_lines,
                          double *ns_per_load);
int drm_stream_create(void **stream);
int drm_stream_destroy(void *stream);
int drm_stream_sync(void *stream);
int drm_event_create(void **ev);
int drm_event_destroy(void *ev);
int drm_event_record(void *ev, void *stream);
/* Work enqueued on `stream` after this call waits for `ev` (pipelining search and rerank on two streams). */
int drm_stream_wait_event(void *stream, void *ev);
int drm_event_elapsed_ms(void *start, void *stop, float *ms);

/* ---------------------------------------------------------------- index (search side)
 * drm_index_load replaces `faiss::read_index(index_file) + dynamic_cast<faiss::IndexHNSWPQ*>`
 * (src/main.cpp:236-237). It parses the faiss "IHNp" file [faiss impl/index_read.cpp], validates
 * it, re-lays it out for HBM (dense level-0 rows, compact upper levels) and uploads it to
 * `device`. drm_index_free replaces `delete alg_hnsw` (src/main.cpp:299). */
int drm_index_load(const char *path, int device, drm_index **out);
int drm_index_free(drm_index *index);
/* drm_index_clone: a replica of a loaded index on `device` (device-to-device copies of its buffers, over xGMI
 * between GPUs, the inline rows derived on the target), for one process driving several GPUs: the file is parsed
 * once (drm_multi_create does this). The source is not changed. */
int drm_index_clone(const drm_index *src, int device, drm_index **out);
int drm_index_get_info(const drm_index *index, drm_index_info *info);

/* drm_search replaces faiss_search(index, query_data, k, ef) (includes/hnswpq/search.hpp:18-21,
 * src/hnswpq/search.cpp:6-56), i.e. `index->hnsw.efSearch = ef; index->search(n, x, k, D, I)`.
 * Host pointers: x [n x d] f32 row-major; D [n x k] f32 and I [n x k] int64 are caller-owned and
 * filled like faiss (ascending distance, ties by id, missing slots (+inf, -1)).
 * Throws-equivalent: n == 0 -> DRM_ERR_ARG "Query data is empty" (search.cpp:16-19).
 * stats may be NULL.
 * Limits (each DRM_ERR_UNSUPPORTED from the search, of drm_search_device[_ex] too; the handle stays usable):
 * 1 <= k <= 1024; max(ef, k) <= 4096; level-0 degree 2 * M_hnsw <= 64 and every upper-level degree <= 64;
 * a PQ distance table of M * 2^nbits <= 16384 entries (64 KB). Within them any PQ shape drm_index_load accepts
 * is searched (nbits 1..16 in faiss's packed layout, any M dividing d). The table, and above max(ef, k) = 512
 * the heaps beside it, live in one workgroup's dynamic LDS -- 105 KB at all three limits at once, which the
 * gfx950 runtime grants without an opt-in (160 KB per workgroup); the queries need no alignment. */
int drm_search(drm_index *index, const float *x, int64_t n, int32_t d, int32_t k, int32_t ef, float *D, int64_t *I,
               drm_search_stats *stats);

/* Same search on device-resident buffers, enqueued on `stream` (a hipStream_t, NULL = default).
 * ndis / nhops ([n] int32, may be NULL) receive the per-query HNSWStats the kernel measured: nhops always as
 * faiss counts it; ndis as faiss counts it (links never seen before) with drm_index_set_exact_stats on, else, on
 * the PQ 8x8 lean kernel, the distances the kernel computed. A query that exceeded its hop bound (broken
 * bookkeeping, never expected) reports nhops = ndis = -1; drm_search turns that into DRM_ERR_INTERNAL. */
int drm_search_device(drm_index *index, const float *d_x, int64_t n, int32_t k, int32_t ef, float *d_D,
                      int64_t *d_I, int32_t *d_ndis, int32_t *d_nhops, void *stream);
/* As drm_search_device, plus d_nhops_upper[n] (may be NULL): the greedy hops on levels >= 1
 * contained in nhops (they read M_hnsw-wide rows instead of 2*M_hnsw-wide ones). */
int drm_search_device_ex(drm_index *index, const float *d_x, int64_t n, int32_t k, int32_t ef, float *d_D,
                         int64_t *d_I, int32_t *d_ndis, int32_t *d_nhops, int32_t *d_nhops_upper, void *stream);
/* Tuning (no reference counterpart): resident search waves per CU of this index's persistent search grid
 * (0 = the default, 20: every CU's LDS holds 20 PQ lookup tables of 8 KB). Used by the occupancy scans of
 * DESIGN.md sec. 4.1. Results do not depend on it. */
int drm_index_set_search_waves(drm_index *index, int32_t waves_per_cu);
/* Statistics (no reference counterpart): on (1), ndis counts faiss's HNSWStats.ndis exactly -- the links each
 * hop finds not yet visited -- with a per-slot visited bitmap kept beside the search (the lean kernel needs none
 * for its results). Off (0, the default; DRM_SEARCH_EXACT_STATS=1 at load sets it) the lean
 * kernel reports the distances it computed. Results (D, I, nhops) do not depend on it. */
int drm_index_set_exact_stats(drm_index *index, int32_t on);
/* Safety (no reference counterpart): every search kernel bounds its loops -- a query past ntotal level-0 hops, or
 * a persistent wave past n work items, means broken search state, and ends with nhops = ndis = -1 for the query
 * and an error count instead of a hang. drm_search returns DRM_ERR_INTERNAL when the count
 * is non-zero; callers of the device entry points (drm_search_device[_ex]) read it here. Synchronizes the
 * device and resets the count. */
int drm_index_search_errors(drm_index *index, int64_t *count);

/* ---------------------------------------------------------------- fp32-L2 index (hnswlib)
 * The reference's hnswlib backend (BASELINE configs[1] "HIP L2 HNSW
 * search"): an hnswlib HierarchicalNSW<float> file searched with fp32 squared-L2 distances. */
typedef struct drm_flat_index drm_flat_index;

typedef struct {
    int32_t d;
    int64_t ntotal;
    int32_t M, maxM0, maxM; /* hnswlib M_, maxM0_ (level 0), maxM_ (levels >= 1) */
    int32_t max_level;
    uint32_t entry_point;
    int32_t efConstruction;
    int64_t device_bytes;
} drm_flat_index_info;

/* new hnswlib::HierarchicalNSW<float>(&space, index_file) (src/hnswlib_dir/test_search.cpp:33):
 * parses and validates an hnswlib saveIndex file, uploads it to `device`. DRM_ERR_UNSUPPORTED for a layout
 * the search kernel has no room for: d % 16 != 0, maxM0 or maxM > 4096, maxM > maxM0, 2^32 elements or more. */
int drm_flat_index_load(const char *path, int device, drm_flat_index **out);
int drm_flat_index_free(drm_flat_index *index);
int drm_flat_index_get_info(const drm_flat_index *index, drm_flat_index_info *info);

/* search(index, query_data, k, ef) (src/hnswlib_dir/search.cpp:7-52, includes/hnswlib_dir/search.hpp):
 * setEf(ef) then searchKnnCloserFirst(q, k) per query. x: [n][d] f32 host; outputs caller-owned
 * [n][k]: D = squared L2 ascending, labels = hnswlib labels (u64); a short result is padded with
 * (+inf, 2^64-1). Throws "Query data is empty" (-1) for n == 0 (search.cpp:20-23). */
int drm_flat_search(drm_flat_index *index, const float *x, int64_t n, int32_t d, int32_t k, int32_t ef, float *D,
                    uint64_t *labels, drm_search_stats *stats);
/* Same on device buffers, enqueued on `stream`; d_ndis/d_nhops [n] receive per-query counts,
 * d_nhops_upper [n] (may be NULL) the hops on levels >= 1 contained in nhops. */
int drm_flat_search_device(drm_flat_index *index, const float *d_x, int64_t n, int32_t k, int32_t ef, float *d_D,
                           uint64_t *d_labels, int32_t *d_ndis, int32_t *d_nhops, int32_t *d_nhops_upper,
                           void *stream);
/* Diagnostic: queries of the last search whose candidate_set outgrew the GPU heap (their outputs
 * are invalid; drm_flat_search reports it as an error). Synchronizes the device. */
int drm_flat_search_overflows(drm_flat_index *index, int64_t *count);
/* As drm_index_search_errors for the fp32 index (drm_flat_search returns DRM_ERR_INTERNAL on a non-zero count). */
int drm_flat_search_errors(drm_flat_index *index, int64_t *count);

/* ---------------------------------------------------------------- exhaustive k-NN scans (no graph)
 * Ground truth for recall figures (no counterpart in the ported back ends; the reference's BruteForce::search,
 * src/hnswm/bruteforce.cpp:27-86, plays this role in its own): every base row is scored and the k smallest under
 * the total order (distance, id) are returned, independent of tiling, grid and run.
 * Limits of all of them: 1 <= k <= 1024 (else DRM_ERR_UNSUPPORTED), n == 0 -> DRM_ERR_ARG "Query data is empty",
 * fewer than 2^31 base rows. */

/* The PQ-ADC scan over every code of a loaded index: dist(i) is the sequential fp32 sum of the query's distance-table
 * entries of code i, the same bits drm_search reports for id i. Host pointers: x [n x d] f32; D [n x k] f32 and
 * I [n x k] int64 filled as drm_search fills them (ascending distance, ties by ascending id, missing slots
 * (+inf, -1) when k > ntotal). d != the index dimension -> DRM_ERR_ARG. PQ 8 x 8 runs the tiled kernel; any other
 * shape drm_index_load accepts runs a plain one when its distance table is at most 64 KB (else
 * DRM_ERR_UNSUPPORTED). kernel_ms (may be NULL) receives the device time of the scan. */
int drm_exact_search(drm_index *index, const float *x, int64_t n, int32_t d, int32_t k, float *D, int64_t *I,
                     double *kernel_ms);
/* The same scan on device-resident buffers: enqueued on `stream` (a hipStream_t, NULL = default) and synchronised
 * (the workspace for the partial lists is allocated in the call and freed before it returns; the handle keeps no
 * state of it). */
int drm_exact_search_device(drm_index *index, const float *d_x, int64_t n, int32_t k, float *d_D, int64_t *d_I,
                            void *stream);
/* The fp32 scan over any device-resident row-major matrix d_base [n_base x d] (a flat index's vectors, the table
 * of drm_refs_embeddings, a builder's input), 16-byte aligned, d % 16 == 0 (else DRM_ERR_UNSUPPORTED): squared L2
 * in the order of drm_flat_search (hnswlib's L2SqrSIMD16ExtAVX: 8 accumulators over dims i, i + 8, ..., added left
 * to right; no FMA), the same bits for the same pair. d_D [n x k] f32, d_I [n x k] int64 row numbers, padding
 * (+inf, -1). Inputs are finite; NaN is not specified. Enqueued on `stream` and synchronised. */
int drm_exact_search_l2_device(const float *d_base, int64_t n_base, int32_t d, const float *d_x, int64_t n,
                               int32_t k, float *d_D, int64_t *d_I, void *stream);
/* The same with host pointers (base and x are uploaded to the current device). */
int drm_exact_search_l2(const float *base, int64_t n_base, int32_t d, const float *x, int64_t n, int32_t k, float *D,
                        int64_t *I, double *kernel_ms);
/* The fp32 scan over a flat index's own vectors: ties by internal id (file order), labels[n x k] receives the
 * hnswlib label of each internal id (padding 2^64-1, as drm_flat_search). Host pointers. */
int drm_flat_exact_search(drm_flat_index *index, const float *x, int64_t n, int32_t d, int32_t k, float *D,
                          uint64_t *labels, double *kernel_ms);
/* Tuning (process-wide; results do not depend on it): base rows per slice of the scans' grid, rounded up to a
 * multiple of 64 (and raised where more than 1024 slices would result); 0 = the default split. For the tests. */
int drm_exact_set_slice_rows(int64_t rows);
/* Queries per workgroup tile of the PQ 8 x 8 scan (for the tests' batch-edge cases). */
int drm_exact_query_tile(void);
/* Diagnostic: the plan a scan of n queries over n_base rows at k would run with under the current slice rows, from
 * the function the scans themselves use. kind: 0 = PQ 8 x 8 with 16-byte aligned queries, 1 = any other PQ scan,
 * 2 = fp32. out7 = {queries per tile, base rows per step, cap (survivor buffer entries per (query, slice)), rows per
 * slice, slices, queries per launch, launches}. Launches nothing. Arguments outside the scans' limits -> the scans'
 * errors. For the tests. */
int drm_debug_exact_plan(int32_t kind, int64_t n, int64_t n_base, int32_t k, int64_t *out7);

/* ---------------------------------------------------------------- Smith-Waterman rerank */
/* Batched calc_sw_score(seq1, seq2) (includes/utils/metrics.hpp:22, src/utils/metrics.cpp:10-45):
 * pair p scores s1[off1[p] .. +len1[p]) against s2[off2[p] .. +len2[p]). Host pointers. */
int drm_sw_scores(const uint8_t *s1, const int64_t *off1, const int32_t *len1, const uint8_t *s2,
                  const int64_t *off2, const int32_t *len2, int64_t npairs, int32_t *scores);

/* The static reference window table `ref_seqs` (read_file(ref, ref_len, 1, lookup=true),
 * src/main.cpp:190): n_ref windows of ref_len bytes, window r at windows[r*row_stride]. */
int drm_refs_create(const uint8_t *windows, int64_t n_ref, int32_t ref_len, int64_t row_stride, int device,
                    drm_refs **out);
int drm_refs_free(drm_refs *refs);
/* Dynamic lookup (pipeline's use_dynamic, src/main.cpp:182-185): the genome string itself
 * (extract_FASTA_sequence, src/utils/parse_inputs.cpp:174-220 -- drm_extract_fasta_sequence) on the
 * device instead of the 2*(L - ref_len + 1)-window table: window id w is genome[w/2 ..+ ref_len),
 * reverse-complemented (comp_table) when w is odd (find_sequence, src/utils/post_processor.cpp:47-64).
 * Genomes of up to 2^31 - 1 bases. */
int drm_refs_create_genome(const uint8_t *genome, int64_t len, int32_t ref_len, int device, drm_refs **out);
int drm_refs_is_genome(const drm_refs *refs, int *is_genome);
/* extract_FASTA_sequence: the file's first line is skipped, whitespace dropped, letters upper-cased
 * and only A/C/G/T/N kept (from every later line, headers included -- the reference's behaviour).
 * Two calls: *len receives the length (out may be NULL), then out[0 .. *len) the sequence. */
int drm_extract_fasta_sequence(const char *path, uint8_t *out, int64_t *len);
/* Shape and device of a window table (any out-pointer may be NULL). */
int drm_refs_get_info(const drm_refs *refs, int64_t *n_ref, int32_t *ref_len, int *device);
/* Opt-in banded Smith-Waterman for every rerank on this handle (an extension: the reference scores the full DP and
 * leaves banding as a TODO, includes/utils/reranker.hpp:12). band 0 = the full DP, bit-exact with calc_sw_score
 * (the default); band 8, 16 or 32 = only the cells with |i - j| <= band (row i over the window, column j over the
 * query, both 0-based), a cell outside the band being 0: the score is at most the full one and equal to it when the
 * best local alignment stays inside the band (NOT parity with the reference). Other values: DRM_ERR_ARG. A new handle
 * starts at $DRM_SW_BAND (unset: 0). Banded queries are limited to 256 bytes and 7 distinct byte values (otherwise
 * the rerank fails with DRM_ERR_UNSUPPORTED). */
int drm_refs_set_sw_band(drm_refs *refs, int32_t band);
int drm_refs_get_sw_band(const drm_refs *refs, int32_t *band);
/* How a Smith-Waterman rerank call on this handle splits its queries (results are the same bytes either way; queries
 * of up to 152 bytes on the full DP only): chunk 0 = one launch sequence on the caller's stream (scoring, re-scores,
 * top-k); chunk n > 0 = chunks of n queries, alternating between two streams the handle owns, so that a chunk's
 * top-k runs beside the next chunk's scoring; chunk -1 = the library's plan (chunks for large calls only). The call
 * stays ordered on the caller's stream in every mode. Below -1: DRM_ERR_ARG. A new handle starts at $DRM_SW_CHUNK
 * (read once per process; unset: -1). */
int drm_refs_set_sw_chunk(drm_refs *refs, int64_t chunk);
int drm_refs_get_sw_chunk(const drm_refs *refs, int64_t *chunk);

/* post_process_sw_static (src/utils/post_processor.cpp:454-549) -> find_sequences (static,
 * :204-336) -> sw_reranker (src/utils/reranker.cpp:3-51) -> calc_sw_score, for nq queries.
 *   neighbors [nq x kk] int64 faiss labels (-1 allowed), queries [nq x q_stride] bytes, q_len[nq]
 *   (the tagged "<"+read+">" strings of format_fastq, src/utils/parse_inputs.cpp:843-950).
 * Outputs [nq x k]: top_scores (SW score), top_ids (dense window id, size_t), counts[nq] (k, or 0
 * when the query had no candidate at all: reranker.cpp:10-11). Ordering among equal scores is
 * libstdc++ std::partial_sort's (reranker.cpp:38-40).
 * Errors: DRM_ERR_K (k > k_clusters*2*stride), DRM_ERR_CANDS (some query has 0 < n_cands < k;
 * *bad_query receives the first such query index when bad_query != NULL). Host pointers. */
int drm_post_process_sw_static(drm_refs *refs, const int64_t *neighbors, int64_t nq, int32_t kk,
                               const uint8_t *queries, const int32_t *q_len, int32_t q_stride, int64_t stride,
                               int32_t k, int32_t k_clusters, int32_t *top_scores, uint64_t *top_ids,
                               int32_t *counts, int64_t *bad_query);

/* Device-buffer form, enqueued on `stream`. d_status[nq] receives per-query status
 * (k or 0 = rows emitted, -1 = not enough candidates, -2 = more than 1024 candidates,
 * -3 = query longer than q_stride's SW build). Host must check d_status. */
int drm_post_process_sw_static_device(drm_refs *refs, const int64_t *d_neighbors, int64_t nq, int32_t kk,
                                      const uint8_t *d_queries, const int32_t *d_q_len, int32_t q_stride,
                                      int64_t stride, int32_t k, int32_t k_clusters, int32_t *d_top_scores,
                                      uint64_t *d_top_ids, int32_t *d_status, void *stream);

/* ---------------------------------------------------------------- Smith-Waterman alignment (traceback)
 * The alignment behind a rerank score, for real SAM fields (the reference's open "TODO: Implement real CIGAR -
 * from SW ranker", src/utils/utils.cpp:380-384, :478-482). The reference has no traceback, so this is the
 * definition. w = the window bytes of window_ids[p] exactly as the rerank reads them (table row; genome slice,
 * reverse-complemented for odd ids; empty for an id outside the table or a window past the genome end), rows
 * i = 1..n; q = the query bytes as passed (tags included), columns j = 1..m; equality is raw byte equality.
 *   H[i][j] = max(0, H[i-1][j-1] + s, H[i-1][j] - 1, H[i][j-1] - 1), s = +1 on equal bytes, else -1;
 *   score = max H = calc_sw_score(w, q). End cell: among H == score the smallest i, then the smallest j.
 *   Traceback from the end cell while H[i][j] > 0, the first true condition deciding the step:
 *     1. H[i][j] == H[i-1][j-1] + s -> M (both step back)   2. H[i][j] == H[i-1][j] - 1 -> D (a window byte)
 *     3. otherwise -> I (a query byte).
 *   ref_begin / q_begin: 0-based, inclusive, where the walk stopped; ref_end / q_end: the end cell's i / j
 *   (exclusive). nm = mismatching M columns + inserted + deleted bases. Operations in forward order, run-length
 *   encoded as BAM words (len << 4) | op, M = 0, I = 1, D = 2; no clip operations (they follow from q_begin / q_end).
 * status: 0 aligned; 1 no alignment (score 0: empty window, id outside the table / genome, pair_query outside
 * [0, nq) on the device entry point, nothing matches): every other field is 0; 2 aligned but n_ops > ops_stride:
 * the first ops_stride words are stored and n_ops is the full count (retry those pairs as a sub-list with a larger
 * stride; ops_stride = q_len + ref_len never overflows). */
typedef struct {
    int32_t score, ref_begin, ref_end, q_begin, q_end, nm, n_ops, status;
} drm_sw_alignment;
/* Pair p aligns window window_ids[p] with query pair_query[p] (queries [nq x q_stride] bytes, q_len[nq]); out[npairs],
 * ops [npairs x ops_stride]. Works on a window table and on a genome handle, always with the full DP (the handle's
 * sw_band is ignored). Queries and windows of up to 256 bytes (DRM_ERR_UNSUPPORTED beyond). Host pointers. */
int drm_sw_align(drm_refs *refs, const uint64_t *window_ids, const int64_t *pair_query, int64_t npairs,
                 const uint8_t *queries, const int32_t *q_len, int32_t q_stride, int64_t nq, drm_sw_alignment *out,
                 uint32_t *ops, int32_t ops_stride);
/* Device-buffer form, enqueued on `stream`; query lengths are bounded by q_stride (<= 256). */
int drm_sw_align_device(drm_refs *refs, const uint64_t *d_window_ids, const int64_t *d_pair_query, int64_t npairs,
                        const uint8_t *d_queries, const int32_t *d_q_len, int32_t q_stride, int64_t nq,
                        drm_sw_alignment *d_out, uint32_t *d_ops, int32_t ops_stride, void *stream);
/* Host only: SAM coordinates of one record (status 0, ops[0 .. n_ops) complete). The read is
 * q[tag_prefix : q_len - tag_postfix]; leading soft clip = q_begin - tag_prefix, trailing soft clip =
 * (q_len - tag_postfix) - q_end, a zero clip omitted. Even window_id: *pos1 = window_id / 2 + ref_begin + 1 and the
 * CIGAR is [lead S] ops [trail S]. Odd window_id (the window is the reverse complement of
 * genome[window_id / 2 ..+ ref_len)): *pos1 = window_id / 2 + (ref_len - ref_end) + 1 and the whole CIGAR is
 * reversed, clips included, i.e. it describes the reverse-complemented read on the forward strand.
 * DRM_ERR_ARG: status != 0, an alignment reaching into the tags, or cigar_cap too small for the string + NUL. */
int drm_sam_cigar(const drm_sw_alignment *a, const uint32_t *ops, int32_t q_len, int32_t tag_prefix,
                  int32_t tag_postfix, int32_t ref_len, uint64_t window_id, int64_t *pos1, char *cigar,
                  int32_t cigar_cap);

/* ---------------------------------------------------------------- Affine-gap alignment over a flanked region
 * A second definition beside drm_sw_align's, for the alignment that gets printed: gaps priced by open + extend, and on
 * a genome handle a target that reaches `flank` bases past either end of the window, so that neither the window grid
 * nor an indel clips the read. drm_sw_align and the rerank are untouched by it.
 * Scoring: mismatch, gap_open and gap_extend are penalties (positive numbers that get subtracted); a gap of L bases
 * costs gap_open + L * gap_extend. Accepted: match 1..31, mismatch 1..63, gap_open 0..63, gap_extend 1..63
 * (DRM_ERR_ARG otherwise); with a region of at most 256 rows every score fits the kernel's packed keys.
 * Target region of window id w, pos = w / 2, on a genome handle with flank >= 0 (DRM_ERR_ARG when negative):
 *   pos + ref_len > glen: empty (status 1), as the window is for drm_sw_align; otherwise genome[s, e) with
 *   s = max(0, pos - flank), e = min(glen, pos + ref_len + flank); for odd w the whole region is reverse-complemented
 *   with the reference's comp_table. On a window-table handle flank must be 0 (DRM_ERR_ARG) and the region is the
 *   table row (empty for an id outside the table). ref_len + 2 * flank > 256 or a query longer than 256 is
 *   DRM_ERR_UNSUPPORTED. Rows i = 1..n run over the region, columns j = 1..m over the query bytes as passed (tags
 *   included); equality is raw byte equality.
 * Recurrence (Gotoh), borders H = 0, E = F = -inf, open / ext = gap_open / gap_extend:
 *   F[i][j] = max(H[i-1][j] - open - ext, F[i-1][j] - ext)      (a run of region bytes: D)
 *   E[i][j] = max(H[i][j-1] - open - ext, E[i][j-1] - ext)      (a run of query bytes: I)
 *   H[i][j] = max(0, H[i-1][j-1] + s, F[i][j], E[i][j])         s = +match on equal bytes, else -mismatch
 *   score = max H. End cell: among H == score the smallest i, then the smallest j (drm_sw_align's rule).
 * Traceback from the end cell in state H:
 *   State H: stop when H[i][j] == 0, i == 0 or j == 0; otherwise the first true condition decides:
 *     1. H[i][j] == H[i-1][j-1] + s -> M, both step back   2. H[i][j] == F[i][j] -> state F at the same cell
 *     3. otherwise -> state E at the same cell.
 *   State F: emit D; if F[i][j] == H[i-1][j] - open - ext the next state is H (closing the gap wins a tie against
 *     extending it), otherwise it stays F; then i -= 1.
 *   State E: the same with I, H[i][j-1] and j -= 1.
 * The record is drm_sw_alignment's: ref_begin / ref_end are relative to the region, nm = mismatching M columns +
 * inserted + deleted bases, operation words and the status 2 rule as for drm_sw_align; ops_stride = q_len + region
 * length never overflows. With {1, 1, 0, 1} and flank 0 the result equals drm_sw_align's, record and words: at
 * open = 0 the closing move is always available, so the walk decides again with M first at every cell. */
typedef struct {
    int32_t match, mismatch, gap_open, gap_extend;
} drm_sw_scoring;
/* drm_sw_align's arguments after the scoring and the flank. Host pointers. */
int drm_sw_align_affine(drm_refs *refs, const drm_sw_scoring *scoring, int32_t flank, const uint64_t *window_ids,
                        const int64_t *pair_query, int64_t npairs, const uint8_t *queries, const int32_t *q_len,
                        int32_t q_stride, int64_t nq, drm_sw_alignment *out, uint32_t *ops, int32_t ops_stride);
/* Device-buffer form, enqueued on `stream`; query lengths are bounded by q_stride (<= 256). */
int drm_sw_align_affine_device(drm_refs *refs, const drm_sw_scoring *scoring, int32_t flank,
                               const uint64_t *d_window_ids, const int64_t *d_pair_query, int64_t npairs,
                               const uint8_t *d_queries, const int32_t *d_q_len, int32_t q_stride, int64_t nq,
                               drm_sw_alignment *d_out, uint32_t *d_ops, int32_t ops_stride, void *stream);
/* The clipping penalty (bwa-mem's -L): drm_sw_align_affine made aware of the read's two ends, so that an alignment
 * which stops short of an end pays a fixed price L and a mismatch a few bases from an end is aligned instead of
 * soft-clipped. The region, the query bytes (tags included), the raw byte equality, E and F, the record, the operation
 * words and the status 2 rule are drm_sw_align_affine's. Accepted: penalty 0..63, tag_prefix and tag_postfix >= 0
 * (DRM_ERR_ARG otherwise). For a pair with query length m let a = tag_prefix and b = m - tag_postfix: the read is
 * columns a + 1 .. b. A pair with b < a has status 1.
 *   floor(j) = 0 for j <= a, -L for j > a           (an alignment that starts inside the read has paid L)
 *   Borders: H[i][0] = 0, H[0][j] = floor(j), E = F = -inf.
 *   H[i][j] = max(floor(j), H[i-1][j-1] + s, F[i][j], E[i][j]); F and E by the recurrences above over this H.
 *   adj(i, j) = H[i][j] - (j == b ? 0 : L) for i >= 1, j >= 1   (an alignment that ends off the read's end pays L)
 *   End cell: the largest adj; among equals the smallest i, then the smallest j. No cell, or a largest adj <= 0, is
 *   status 1 with every other field 0.
 * Traceback: the one above, except that state H stops when i == 0, j == 0 or H[i][j] == floor(j), tested before the
 *   M / F / E conditions: a tie goes to stopping, as it does at 0.
 * score is the plain affine score of the walk that is printed, adj + L * [q_begin > a] + L * [q_end != b], so that
 *   replaying the operations under the scoring gives exactly score and AS:i stays comparable between reads.
 * At L = 0 this is drm_sw_align_affine for any tags, record and words. drm_sam_cigar_region, drm_sw_align_md and
 * drm_sam_md take the records as they are. */
typedef struct {
    int32_t penalty, tag_prefix, tag_postfix;
} drm_sw_clip;
/* drm_sw_align_affine's arguments and errors, with the clipping parameters after the scoring. Host pointers. */
int drm_sw_align_affine_clip(drm_refs *refs, const drm_sw_scoring *scoring, const drm_sw_clip *clip, int32_t flank,
                             const uint64_t *window_ids, const int64_t *pair_query, int64_t npairs,
                             const uint8_t *queries, const int32_t *q_len, int32_t q_stride, int64_t nq,
                             drm_sw_alignment *out, uint32_t *ops, int32_t ops_stride);
/* Device-buffer form, as drm_sw_align_affine_device. */
int drm_sw_align_affine_clip_device(drm_refs *refs, const drm_sw_scoring *scoring, const drm_sw_clip *clip,
                                    int32_t flank, const uint64_t *d_window_ids, const int64_t *d_pair_query,
                                    int64_t npairs, const uint8_t *d_queries, const int32_t *d_q_len, int32_t q_stride,
                                    int64_t nq, drm_sw_alignment *d_out, uint32_t *d_ops, int32_t ops_stride,
                                    void *stream);
/* Host only: the target region of one window id on a genome handle (DRM_ERR_ARG on a window table or a negative
 * flank, DRM_ERR_UNSUPPORTED when ref_len + 2 * flank > 256): genome[*start, *start + *len), *reverse = 1 when it is
 * reverse-complemented. A window past the genome end has *len = 0 (and *start = 0). */
int drm_sw_align_region(const drm_refs *refs, uint64_t window_id, int32_t flank, int64_t *start, int32_t *len,
                        int32_t *reverse);
/* Host only: drm_sam_cigar for a record whose ref_begin / ref_end are relative to a region: *pos1 = region_start +
 * (reverse ? region_len - ref_end : ref_begin) + 1, the CIGAR reversed, clips included, when reverse != 0.
 * drm_sam_cigar is the case (window_id / 2, ref_len, window_id & 1). The same errors. */
int drm_sam_cigar_region(const drm_sw_alignment *a, const uint32_t *ops, int32_t q_len, int32_t tag_prefix,
                         int32_t tag_postfix, int64_t region_start, int32_t region_len, int32_t reverse,
                         int64_t *pos1, char *cigar, int32_t cigar_cap);

/* ---------------------------------------------------------------- MD: the reference bases under an alignment
 * Which columns of an alignment differ and what the reference holds there, for the SAM MD:Z tag. The reference prints
 * no tags (src/utils/utils.cpp:380-384), so this text is the definition. It is computed for pair p from the pair
 * itself (window id, query index), its drm_sw_alignment record and its operation words, all as drm_sw_align or
 * drm_sw_align_affine left them.
 * Target bytes: the region exactly as drm_sw_align_affine defines it for (window id, flank): a table row, or
 *   genome[max(0, pos - flank), min(glen, pos + ref_len + flank)), reverse-complemented as a whole with comp_table for
 *   an odd id, empty past the genome end. With flank 0 this is drm_sw_align's window. Equality is raw byte equality
 *   between a region byte and a query byte, the aligners' own rule (N against N matches, a tag matches no base).
 * Walk the operations forward from (ref_begin, q_begin) with a counter `run` of matching columns, 0 at the start:
 *   M column, equal bytes:    run += 1.
 *   M column, unequal bytes:  emit the number run, run = 0, then emit one mismatch word with the region byte.
 *   I operation:              skip its query bytes, emit nothing: a run continues across an insertion.
 *   D operation of n bytes:   emit the number run (also when it is 0), run = 0, then n deleted-base words with the
 *                             region bytes.
 *   after the last operation: emit the number run.
 * Words are (value << 4) | kind: kind 0 a number (value = the run length), 1 a mismatch, 2 a deleted base (value = the
 * region byte). The stream starts and ends with a number, two numbers are never adjacent, and the word count is
 * 2 * mismatches + D operations + deleted bases + 1 (a number in front of every mismatch and every D operation, and
 * one at the end) <= 2 * region length + 1 <= 513. This is samtools calmd's token rule: D, I, D gives "^AC0^GT".
 * Per pair: n_words, the counts of matching and mismatching M columns, of inserted and of deleted bases, and status
 *   0 done;
 *   1 the record holds no alignment (its status is 1), or the region or the query is empty: every other field is 0;
 *   2 done, but n_words > md_stride: the first md_stride words are stored and n_words is the full count (retry those
 *     pairs as a sub-list with a larger stride; md_stride = 2 * (ref_len + 2 * flank) + 1 never overflows);
 *   3 the record and its words describe no walk inside this region and query: every other field is 0. Raised by a
 *     record status other than 0 and 1 (2: its words are incomplete), n_ops outside [1, 512], an operation kind above
 *     2 or a zero length, a negative ref_begin or q_begin, ref_begin > ref_end, ref_end past the region, q_end past
 *     the query, or the words' reference or query span differing from ref_end - ref_begin or q_end - q_begin.
 * Status 1 is decided before status 3. Whatever a record says, operation words are read only inside
 * ops[ops_off[p] .. + min(n_ops, 512)) and only when the record's status is 0, and no byte is read outside the region
 * and the query. For records the aligners produced, n_mismatch + n_ins + n_del == nm. */
typedef struct {
    int32_t n_words, n_match, n_mismatch, n_ins, n_del, status;
} drm_sw_md;
/* Pairs, queries, flank limits and argument errors as for drm_sw_align_affine (flank 0 on a window table; a region or
 * a query above 256 bytes is DRM_ERR_UNSUPPORTED; a negative flank, md_stride or ops_off[p] is DRM_ERR_ARG). rec[npairs];
 * pair p's words start at ops[ops_off[p]] (p * ops_stride for the aligner's strided buffer); out[npairs],
 * md [npairs x md_stride], words past n_words read as 0. Host pointers. */
int drm_sw_align_md(drm_refs *refs, int32_t flank, const uint64_t *window_ids, const int64_t *pair_query,
                    int64_t npairs, const uint8_t *queries, const int32_t *q_len, int32_t q_stride, int64_t nq,
                    const drm_sw_alignment *rec, const uint32_t *ops, const int64_t *ops_off, drm_sw_md *out,
                    uint32_t *md, int32_t md_stride);
/* Device-buffer form, enqueued on `stream`; query lengths are bounded by q_stride (<= 256), a pair_query outside
 * [0, nq) is an empty query (status 1), and ops_off is not checked. */
int drm_sw_align_md_device(drm_refs *refs, int32_t flank, const uint64_t *d_window_ids, const int64_t *d_pair_query,
                           int64_t npairs, const uint8_t *d_queries, const int32_t *d_q_len, int32_t q_stride,
                           int64_t nq, const drm_sw_alignment *d_rec, const uint32_t *d_ops, const int64_t *d_ops_off,
                           drm_sw_md *d_out, uint32_t *d_md, int32_t md_stride, void *stream);
/* Host only: the MD string of one pair (status 0, words[0 .. n_words) complete): numbers in decimal, a mismatch as its
 * letter, a run of consecutive deleted-base words as "^" and their letters. reverse != 0: the region was a reverse
 * complement, so the words are taken in reverse order and every base is complemented (A<->T, C<->G, N->N), which gives
 * MD on the forward strand as drm_sam_cigar_region gives the CIGAR.
 * DRM_ERR_ARG: status != 0, a kind above 2, a base that is not 'A'..'Z' after the complement, a stream that does not
 * start and end with a number or holds two adjacent numbers, or md_cap too small for the string + NUL. */
int drm_sam_md(const drm_sw_md *h, const uint32_t *words, int32_t reverse, char *md, int32_t md_cap);

/* ---------------------------------------------------------------- Mate pairing (paired-end reads)
 * Which hit of mate 1 and which hit of mate 2 belong to one fragment. The reference maps single reads only (its SAM
 * prints "* 0 0" in RNEXT / PNEXT / TLEN), so this text is the definition.
 * A hit is a row (w, s) of a read's rerank output (top_ids / top_scores): pos(w) = w >> 1 (int64), rev(w) = w & 1.
 * Only the first `count` rows of a list take part, a count outside [0, k] being clamped (a negative rerank status is
 * 0 rows), and of those only the live ones, s > 0: a zero-score row is an out-of-genome window. Row indices j always
 * refer to the original list. A mate's top hit is its live row of largest s, the smallest row among equals (the list
 * need not be sorted).
 * A proper combination (FR library orientation, the only one supported): row j1 of mate 1 with row j2 of mate 2 is
 * proper iff both rows are live, their rev differs, and with f the forward and r the reverse hit pos(f) <= pos(r) and
 * min_tlen <= T <= max_tlen (both inclusive), T = pos(r) + ref_len - pos(f) in 64-bit arithmetic: any u64 window id
 * is safe.
 * Choice: n_proper = the number of proper combinations (always reported). The best proper combination maximises
 * s1 + s2, then takes the smallest j1, then the smallest j2. With t1, t2 the mates' top hits:
 *   status 0: both mates live, a proper combination exists and best_sum >= s(t1) + s(t2) - unpaired_penalty:
 *             (j1, j2) = the best proper combination, score = its sum, tlen = its T;
 *   status 1: both mates live, otherwise: (j1, j2) = (t1, t2), score = s(t1) + s(t2), tlen = 0;
 *   status 2: only mate 1 live: j1 = t1, j2 = -1, score = s(t1), tlen = 0;
 *   status 3: only mate 2 live: j1 = -1, j2 = t2, score = s(t2), tlen = 0;
 *   status 4: neither live: j1 = j2 = -1, score = 0, tlen = 0.
 * Arguments: 0 <= k <= 1024 (beyond: DRM_ERR_UNSUPPORTED; 1024 is the rerank's candidate cap), 1 <= ref_len <= 2^20,
 * 0 <= min_tlen <= max_tlen <= 2^30, 0 <= unpaired_penalty <= 2^20, row_step >= 1, npairs >= 0 (DRM_ERR_ARG
 * otherwise). Scores of the counted rows must lie in [0, 2^20]: the host entry point checks it (DRM_ERR_ARG), for the
 * device form it is the caller's contract (the rerank's scores are at most the read length).
 * Layout: row_step is the number of list rows between consecutive pairs: pair p's mate-m list starts at
 * ids_m + p * row_step * k (scores_m likewise) and its count is cnt_m[p * row_step]. row_step = 1 takes two separate
 * arrays; row_step = 2 with ids2 = ids1 + k, scores2 = scores1 + k, cnt2 = cnt1 + 1 takes one interleaved batch
 * (read 2p is mate 1, read 2p + 1 mate 2). The device form consumes drm_post_process_sw_{static,dynamic}_device's
 * d_top_ids, d_top_scores and d_status unchanged. */
typedef struct {
    int32_t ref_len, min_tlen, max_tlen, unpaired_penalty;
} drm_pair_params;
typedef struct {
    int32_t j1, j2, score, tlen, n_proper, status;
} drm_pair_result;
/* Host pointers; runs on the current device. out[npairs]. */
int drm_pair_hits(const drm_pair_params *p, const uint64_t *ids1, const int32_t *scores1, const int32_t *cnt1,
                  const uint64_t *ids2, const int32_t *scores2, const int32_t *cnt2, int64_t npairs, int32_t k,
                  int64_t row_step, drm_pair_result *out);
/* Device-buffer form, enqueued on `stream`. Stateless: no handle, the current device. */
int drm_pair_hits_device(const drm_pair_params *p, const uint64_t *d_ids1, const int32_t *d_scores1,
                         const int32_t *d_cnt1, const uint64_t *d_ids2, const int32_t *d_scores2,
                         const int32_t *d_cnt2, int64_t npairs, int32_t k, int64_t row_step, drm_pair_result *d_out,
                         void *stream);
/* Host only: the SAM fields that relate the two lines of a pair. in[0] is mate 1, in[1] mate 2: mapped, reverse
 * (the strand of a mapped mate), pos1 (1-based leftmost position) and ref_span = ref_end - ref_begin of its alignment
 * record; the last three are ignored for an unmapped mate. proper != 0: the pairing chose a proper combination.
 * flag = 0x1 | 0x40 (mate 1) or 0x80 (mate 2) | 0x4 self unmapped | 0x8 mate unmapped | 0x10 self mapped and reverse |
 *        0x20 mate mapped and reverse | 0x2 iff proper and both mapped.
 * Both mapped: pos = the read's own pos1, pnext = the mate's, has_rname = 1; L = max(pos1 + ref_span - 1) -
 *   min(pos1) + 1 over the two; the mate with the smaller pos1 gets tlen = +L, the other -L, mate 1 gets +L when the
 *   pos1 are equal. One mapped: both lines carry the mapped mate's position in pos and pnext, tlen = 0, has_rname = 1.
 * None mapped: has_rname = 0 and pos = pnext = tlen = 0.
 * DRM_ERR_ARG: a null pointer, or a mapped mate with pos1 < 1 or ref_span < 1. */
typedef struct {
    int32_t mapped, reverse;
    int64_t pos1;
    int32_t ref_span;
} drm_sam_mate;
typedef struct {
    int32_t flag, has_rname;
    int64_t pos, pnext, tlen;
} drm_sam_mate_fields;
int drm_sam_pair_fields(const drm_sam_mate in[2], int proper, drm_sam_mate_fields out[2]);

/* ---------------------------------------------------------------- Mate rescue (paired-end reads)
 * A pair is proper only when both mates' true windows come through the embedding search and the rerank. Where one
 * did not (a repeat, a long indel, a burst of errors, a hit outside the top k), the mate that did map is taken as an
 * anchor and the other read is aligned, score only, against the stretch of genome in which the template length says
 * it must lie. The reference has no paired mode, so this text is the definition.
 * Region of a task with anchor id w, a = w >> 1, all arithmetic in 64 bits, dlo = max(0, min_tlen - ref_len) and
 * dhi = max_tlen - ref_len (drm_pair_hits' range of pos(r) - pos(f)), glen the genome length:
 *   a + ref_len > glen, or dhi < dlo: empty.
 *   w even (the anchor is the forward hit; the mate is a reverse hit at a position in [a + dlo, a + dhi]):
 *     genome[s, e) with s = min(glen, a + dlo), e = min(glen, a + dhi + ref_len), reverse-complemented as a whole with
 *     the reference's comp_table; reverse = 1.
 *   w odd (the anchor is the reverse hit; the mate is a forward hit at a position in [a - dhi, a - dlo]):
 *     genome[s, e) with s = max(0, a - dhi), e = min(glen, a - dlo + ref_len), as it stands; reverse = 0.
 *   e <= s: empty. An empty region is reported as region_start = 0, region_len = 0, reverse as above.
 * dhi - dlo + ref_len > 2048 is DRM_ERR_UNSUPPORTED, decided from the parameters alone (the default 0,1000 template
 * length gives 1,000 rows): with scores below 2^13, 11 bits of row and 8 of column the kernel's best-cell key fits
 * 32 bits.
 * Recurrence and end cell are drm_sw_align_affine's, word for word: Gotoh's H / E / F with the caller's scoring (the
 * same accepted ranges), rows i = 1..n over the region as oriented, columns j = 1..m over the query bytes as passed
 * (tags included, up to 256 bytes, DRM_ERR_UNSUPPORTED beyond), raw byte equality; score = max H, the end cell is,
 * among the cells with H == score, the one of smallest i, then smallest j. There is no traceback.
 * Record: region_start / region_len / reverse as above; score; ref_end / q_end = the end cell's i / j (exclusive
 * ends, ref_end relative to the oriented region); status 0 = found, 1 = nothing (an empty region, score 0, or
 * task_query outside [0, nq) on the device entry point): every field but the region's three is 0.
 * Arguments: a genome handle (a window table: DRM_ERR_ARG); the pair parameters' ranges are drm_pair_hits', and
 * ref_len must equal the handle's (DRM_ERR_ARG); unpaired_penalty is not used. The host form checks task_query and
 * q_len as drm_sw_align does.
 * Scores are comparable with the rerank's only under the rerank's scoring {1, 1, 0, 1}: a caller that weighs a rescued
 * mate against reranked hits (drm_pair_rescue_choose) rescues with it. The scan visits every offset of the region, not
 * only the stride grid of the window ids the search returns, so a rescued score can exceed the score of the best grid
 * window over the same bases by the few columns the grid cuts off: this favours the rescued mate slightly. */
typedef struct {
    int64_t region_start;
    int32_t region_len, reverse, score, ref_end, q_end, status;
} drm_rescue_result;
/* Task t aligns query task_query[t] (queries [nq x q_stride] bytes, q_len[nq]) against the region of anchor_ids[t];
 * out[ntasks]. Host pointers. */
int drm_mate_rescue(drm_refs *refs, const drm_sw_scoring *scoring, const drm_pair_params *p,
                    const uint64_t *anchor_ids, const int64_t *task_query, int64_t ntasks, const uint8_t *queries,
                    const int32_t *q_len, int32_t q_stride, int64_t nq, drm_rescue_result *out);
/* Device-buffer form, enqueued on `stream`; query lengths are bounded by q_stride (<= 256). */
int drm_mate_rescue_device(drm_refs *refs, const drm_sw_scoring *scoring, const drm_pair_params *p,
                           const uint64_t *d_anchor_ids, const int64_t *d_task_query, int64_t ntasks,
                           const uint8_t *d_queries, const int32_t *d_q_len, int32_t q_stride, int64_t nq,
                           drm_rescue_result *d_out, void *stream);
/* Host only, no device: the region of one anchor on a genome of glen bases (glen >= 0; the parameter errors are
 * drm_mate_rescue's, the 2,048-row cap included). */
int drm_mate_rescue_region(const drm_pair_params *p, int64_t glen, uint64_t anchor_id, int64_t *start, int32_t *len,
                           int32_t *reverse);
/* Host only: the window id under which drm_sw_align / drm_sw_align_affine find a rescued hit (status 0, DRM_ERR_ARG
 * otherwise, also for glen < ref_len, ref_len < 1, a region outside [0, glen) or ref_end outside [1, region_len]):
 * p =region_start + ref_end - ref_len for a forward region,
 * p = region_start + region_len - ref_end for a reversed one, clamped to [0, glen - ref_len]; *window_id =
 * 2 * p + reverse. In both orientations the alignment's last row is the window's last row, or lies inside the window
 * after clamping, so drm_sw_align_affine(*window_id, flank F) contains the whole alignment whenever it deletes at
 * most F genome bases. */
int drm_mate_rescue_window(const drm_rescue_result *r, int32_t ref_len, int64_t glen, uint64_t *window_id);
/* Host only: whether a rescued mate replaces what drm_pair_hits chose for a pair. s1 / s2 are the scores of the
 * pair's chosen rows (0 for j = -1), anchor1 / anchor2 their window ids. rA is the rescue of mate 2 anchored on mate
 * 1's chosen hit, rB the rescue of mate 1 anchored on mate 2's; NULL = no task. A record is valid when its status is
 * 0 and its score >= min_score; sumA = s1 + rA->score, sumB = rB->score + s2.
 *   pair status 0 or 4: unchanged.
 *   pair status 1: a valid candidate qualifies when its sum >= s1 + s2 - unpaired_penalty, drm_pair_hits' test for a
 *                  proper combination; the larger sum wins, rA on a tie.
 *   pair status 2: rA qualifies when valid.     pair status 3: rB qualifies when valid.
 * A winner: *out = the pair with status 5 (mate 2 rescued; j2 = -1) or 6 (mate 1 rescued; j1 = -1), score = the sum,
 * tlen = pos(r) + ref_len - pos(f) from the anchor and the rescued window id w_r (drm_mate_rescue_window), which is
 * returned in *rescued_id; j of the other mate and n_proper are kept. Otherwise *out = *pair and *rescued_id = 0.
 * DRM_ERR_ARG: a null pair / out / rescued_id, a pair status outside [0, 4], or a winner that
 * drm_mate_rescue_window rejects. */
int drm_pair_rescue_choose(const drm_pair_result *pair, int32_t s1, int32_t s2, uint64_t anchor1, uint64_t anchor2,
                           const drm_rescue_result *rA, const drm_rescue_result *rB, int32_t ref_len, int64_t glen,
                           int32_t unpaired_penalty, int32_t min_score, drm_pair_result *out, uint64_t *rescued_id);

/* ---------------------------------------------------------------- Mapping quality (MAPQ)
 * How certain a read's chosen hit is, from the hits that compete with it. The reference prints MAPQ 60 on every line
 * and has no such step, so this text is the definition.
 * Hit model (drm_pair_hits', word for word): a hit is a row (w, s) of a read's rerank output, pos(w) = w >> 1 (int64),
 * rev(w) = w & 1. Only the first `count` rows of a list take part, a count outside [0, k] being clamped, and of those
 * only the live ones, s > 0. Row indices always refer to the original list. The top of a set of rows is the row of
 * largest s, the smallest row among equals. 0 <= k <= 1024 (beyond: DRM_ERR_UNSUPPORTED). Scores of the counted rows
 * must lie in [0, 2^20]: the host forms check it (DRM_ERR_ARG), for the device forms it is the caller's contract.
 * Parameters (DRM_ERR_ARG outside): 1 <= ref_len <= 2^20, 1 <= locus_span <= 2^20, 0 <= min_score <= 2^20,
 * 0 <= sub_band <= 2^20.
 * Same locus: rows a and b are in the same locus iff rev(a) == rev(b) and |pos(a) - pos(b)| < locus_span, in 64-bit
 * arithmetic (positions are below 2^63: any u64 id is safe). At stride 1 the windows beside the true one overlap it
 * and score almost as high; they are one locus, not competitors.
 * The locus scan of one list with head row h (h = -1: the list's top hit; a given h must be a live counted row,
 * otherwise the record is the "nothing" record):
 *   1. locus 0 = every live row in the same locus as h, h included; locus_rows = their number, best = h,
 *      best_score = s(h);
 *   2. locus 0 is removed. sub_row = the top of what remains, or -1; sub_score = s(sub_row), or 0;
 *   3. n_sub counts greedily: take the top t of what remains; stop when nothing remains or
 *      s(t) < sub_score - sub_band; otherwise count one, remove every remaining row in the same locus as t, repeat.
 *      So n_sub >= 1 exactly when sub_score > 0.
 * The suppression is greedy, not transitive: rows at positions 0, 100, 200 of one strand with scores 100, 90, 80 and a
 * span of 150 give locus 0 = {0, 100} and the row at 200 as the competitor.
 * Record: status 0 = a head exists; status 1 = nothing: best = sub_row = -1, every other field 0.
 * mapq = drm_mapq_value(best_score, sub_score, n_sub, full, min_score), a pure function in int64:
 *   1. 0 if s1 <= 0 or full <= 0;
 *   2. c = min(s1, full), s2 = max(sub, min_score);
 *   3. 0 if c <= s2;
 *   4. q = floor(60 * (c - s2) * c / ((c - min_score) * full)): the divisor is positive because c > s2 >= min_score,
 *      and q <= 60 because c - s2 <= c - min_score and c <= full;
 *   5. q -= 3 * floor(log2(n_sub + 1));
 *   6. clamped to [0, 60].
 * `full` is the score of the read against itself under the rerank's scoring {1, 1, 0, 1}: its length without tags.
 * A perfect unique read gets 60, a unique read at 130 of 150 gets 52, a read whose competitor scores the
 * same gets 0. */
typedef struct {
    int32_t ref_len, locus_span, min_score, sub_band;
} drm_mapq_params;
typedef struct {
    int32_t best, best_score, locus_rows, sub_row, sub_score, n_sub, mapq, status;
} drm_mapq_result;
/* Read r's list is ids / scores + r * k with the count cnt[r]; head[r] its head row (head == NULL: -1 for every
 * read), full[r] its self score. out[nreads]. Host pointers; runs on the current device. */
int drm_hit_mapq(const drm_mapq_params *p, const uint64_t *ids, const int32_t *scores, const int32_t *cnt,
                 const int32_t *head, const int32_t *full, int64_t nreads, int32_t k, drm_mapq_result *out);
/* Device-buffer form, enqueued on `stream`. Stateless: no handle, the current device. It consumes
 * drm_post_process_sw_{static,dynamic}_device's d_top_ids, d_top_scores and d_status unchanged. */
int drm_hit_mapq_device(const drm_mapq_params *p, const uint64_t *d_ids, const int32_t *d_scores, const int32_t *d_cnt,
                        const int32_t *d_head, const int32_t *d_full, int64_t nreads, int32_t k,
                        drm_mapq_result *d_out, void *stream);
/* Host only, no device: drm_mapq_value as defined above. DRM_ERR_ARG: a null mapq, n_sub < 0, min_score outside
 * [0, 2^20], or |s1|, |sub|, n_sub or |full| beyond 2^20 (the products stay far inside int64). */
int drm_mapq_value(int64_t s1, int64_t sub, int64_t n_sub, int64_t full, int64_t min_score, int32_t *mapq);
/* Pair MAPQ. The two lists in drm_pair_hits' layout (row_step included), full_m indexed like cnt_m
 * (full_m[p * row_step]), pairs[npairs] the records of drm_pair_hits on the same lists and pair parameters, whose
 * statuses must be 0 to 4 (the host form: DRM_ERR_ARG; a device record outside gives the all-zero record). For pair p:
 *   1. q_se_m = the locus scan's mapq of mate m's list with head = the pair's chosen row j_m; 0 for j_m = -1;
 *   2. status 0 only: sub_pair = the largest s1 + s2 over the proper combinations (j1', j2') (drm_pair_hits'
 *      definition of proper), except those where j1' is in the chosen j1's locus AND j2' is in the chosen j2's locus
 *      (locus 0 of the two scans); 0 if none remain;
 *   3. with t1, t2 the mates' top hits, subo = max(sub_pair, s(t1) + s(t2) - unpaired_penalty);
 *   4. q_pe = clamp(6 * (score - subo), 0, 60), score the record's;
 *   5. mapq_m = q_se_m if q_se_m > q_pe, otherwise min(q_pe, q_se_m + 40): bwa-mem's rule for letting a confident pair
 *      lift an ambiguous mate;
 *   6. statuses 1 to 3: mapq_m = q_se_m, q_pe = 0, sub_pair = 0;
 *   7. status 4: every field 0. */
typedef struct {
    int32_t mapq1, mapq2, q_se1, q_se2, q_pe, sub_pair;
} drm_pair_mapq_result;
int drm_pair_mapq(const drm_pair_params *pp, const drm_mapq_params *mp, const uint64_t *ids1, const int32_t *scores1,
                  const int32_t *cnt1, const uint64_t *ids2, const int32_t *scores2, const int32_t *cnt2,
                  const int32_t *full1, const int32_t *full2, const drm_pair_result *pairs, int64_t npairs, int32_t k,
                  int64_t row_step, drm_pair_mapq_result *out);
int drm_pair_mapq_device(const drm_pair_params *pp, const drm_mapq_params *mp, const uint64_t *d_ids1,
                         const int32_t *d_scores1, const int32_t *d_cnt1, const uint64_t *d_ids2,
                         const int32_t *d_scores2, const int32_t *d_cnt2, const int32_t *d_full1,
                         const int32_t *d_full2, const drm_pair_result *d_pairs, int64_t npairs, int32_t k,
                         int64_t row_step, drm_pair_mapq_result *d_out, void *stream);
/* Host only, plain loops: the MAPQ of rescued pairs. pairs[npairs] are the records after drm_pair_rescue_choose
 * (statuses 0 to 6, DRM_ERR_ARG otherwise), inout[npairs] the drm_pair_mapq records of the pre-rescue pairs. A pair of
 * status 5 (mate 2 rescued, mate 1 the anchor) keeps mapq1 and gets
 * mapq2 = min(mapq1, drm_mapq_value(rescue_score[p], 0, 0, full2[p * row_step], min_score)); status 6 the mirror image
 * with full1[p * row_step] (full_m indexed as in drm_pair_mapq): a rescued placement is never more certain than its
 * anchor. rescue_score[p] is the rescued mate's own score (the record's sum minus the anchor's score). Every other
 * field and every other pair is left as it is; rescue_score / full of an unrescued pair are not read. */
int drm_pair_mapq_rescued(const drm_mapq_params *mp, const drm_pair_result *pairs, const int32_t *rescue_score,
                          const int32_t *full1, const int32_t *full2, int64_t npairs, int64_t row_step,
                          drm_pair_mapq_result *inout);

/* ---------------------------------------------------------------- Locus list
 * The distinct loci of a read's hit list: the placements a SAM writer prints as the primary line and its secondary
 * lines or XA entries. The reference has no such step, so this text is the definition. The hit model, "same locus",
 * "top of a set" and the head rule are drm_hit_mapq's, word for word, and so are the lists, counts, heads, self
 * scores, their argument ranges and the host form's score check. New parameters: 1 <= max_loci <= 64 (0 or less:
 * DRM_ERR_ARG; beyond 64: DRM_ERR_UNSUPPORTED) and 0 <= drop_pct <= 100 (DRM_ERR_ARG outside).
 * With head row h (h = -1: the list's top hit) the enumeration of one list runs as follows:
 *   1. There is no head (h = -1 with no live row, or a given h that is not a live counted row): the MAPQ record is the
 *      "nothing" record (status 1), n_loci = n_pass = 0 and every slot is empty.
 *   2. Locus 0 = every live row in the same locus as h. It is always recorded, in slot 0, with id(h), s(h), row h and
 *      size = its number of rows, and it counts in n_pass. best_score = s(h). Locus 0 is removed.
 *   3. Repeat with t = the top of what remains and s = s(t); stop when nothing remains.
 *        counts_sub = s >= sub_score - sub_band, sub_score being s of the first t, as in drm_hit_mapq;
 *        passes     = s >= min_score and 100 * s >= drop_pct * best_score.
 *      Neither holds: stop. counts_sub: n_sub += 1. passes: n_pass += 1, and if n_loci < max_loci the locus is recorded
 *      in the next slot as (id(t), s, row t, size = the rows removed in this step). Then every remaining row in the
 *      same locus as t is removed.
 *      The tops come in non-increasing score, so both tests are monotone and n_sub equals drm_hit_mapq's.
 * Example: rows at positions 0, 100, 200 of one strand with scores 100, 90, 80, a span of 150, min_score 39 and
 * drop_pct 80 give slot 0 = {row 0, score 100, size 2} and slot 1 = {row 2, score 80, size 1}; with drop_pct 81 the
 * second locus no longer passes, and n_loci = n_pass = 1.
 * Outputs per read r: out[r], byte for byte drm_hit_mapq's record for the same list, head, full and parameters;
 * n_loci[r], the slots recorded; n_pass[r], the loci that pass in the whole list (n_pass > n_loci: the list was
 * truncated at max_loci); and slot j of the read at index r * max_loci + j of loci_ids (u64), loci_scores, loci_rows
 * and loci_size (i32). A slot at or beyond n_loci[r] holds id ~0, score 0, row -1, size 0, so every byte of the
 * outputs is defined. loci_ids / loci_scores / n_loci have the rerank's layout (ids[r * width + j], cnt[r]) with
 * width = max_loci: drm_sw_align*, drm_sw_align_md and a SAM writer consume them unchanged. nreads == 0 is DRM_OK and
 * touches nothing. */
typedef struct {
    int32_t max_loci, drop_pct;
} drm_loci_params;
int drm_hit_loci(const drm_mapq_params *mp, const drm_loci_params *lp, const uint64_t *ids, const int32_t *scores,
                 const int32_t *cnt, const int32_t *head, const int32_t *full, int64_t nreads, int32_t k,
                 drm_mapq_result *out, int32_t *n_loci, int32_t *n_pass, uint64_t *loci_ids, int32_t *loci_scores,
                 int32_t *loci_rows, int32_t *loci_size);
/* Device-buffer form, enqueued on `stream`. Stateless: no handle, the current device. */
int drm_hit_loci_device(const drm_mapq_params *mp, const drm_loci_params *lp, const uint64_t *d_ids,
                        const int32_t *d_scores, const int32_t *d_cnt, const int32_t *d_head, const int32_t *d_full,
                        int64_t nreads, int32_t k, drm_mapq_result *d_out, int32_t *d_n_loci, int32_t *d_n_pass,
                        uint64_t *d_loci_ids, int32_t *d_loci_scores, int32_t *d_loci_rows, int32_t *d_loci_size,
                        void *stream);

/* ---------------------------------------------------------------- Template-length window from the reads
 * drm_pair_hits, drm_mate_rescue and drm_pair_mapq all take the window [min_tlen, max_tlen] a proper pair's template
 * length must lie in. It is a property of the sequenced library, so it is estimated from the batch being mapped, as
 * bwa-mem does in mem_pestat: the pairs whose two mates each map uniquely on their own are turned into a histogram of
 * template lengths (drm_tlen_scan), and the window is read off the histogram (drm_tlen_estimate). The reference has no
 * paired mode, so this text is the definition.
 * Scan. Lists, counts, row_step, the indexing of full_m and the hit model are drm_pair_mapq's, word for word; the
 * argument ranges are drm_hit_mapq's (0 <= k <= 1024, beyond: DRM_ERR_UNSUPPORTED; scores of the counted rows in
 * [0, 2^20]: the host form checks them, DRM_ERR_ARG, for the device form they are the caller's contract), with
 * 0 <= min_mapq <= 60 and ref_len <= max_scan <= 2^16 (DRM_ERR_ARG outside). For pair p:
 *   1. mapq_m = the mapq field of drm_hit_mapq's record of mate m's list with head -1 and self score full_m; 0 when
 *      that record's status is 1. mapq1 and mapq2 are always reported.
 *   2. Mate m is confident iff mapq_m >= min_mapq and its record's status is 0. Not both confident: cls = 0, tlen = 0.
 *   3. Otherwise w1, w2 = the ids of the two records' `best` rows, and in 64-bit arithmetic (any u64 id is safe):
 *        rev(w1) == rev(w2):  cls = 3 (same strand), T = |pos(w1) - pos(w2)| + ref_len;
 *        otherwise, with f the forward hit, r the reverse hit and d = pos(r) - pos(f):
 *          d >= 0: cls = 1 (FR), T = d + ref_len -- drm_pair_hits' T;
 *          d < 0:  cls = 2 (RF), T = -d + ref_len;
 *        T > max_scan: cls = 4 (far), tlen = 0; otherwise tlen = T.
 * Histogram: hist[(cls - 1) * (max_scan + 1) + T] += 1 for cls 1 to 3, three rows of max_scan + 1 bins. The host form
 * zeroes hist first; the device form ADDS into d_hist, which the caller zeroes and may accumulate over several calls.
 * The counts are integers: the result does not depend on the order in which the pairs finish. samples / d_samples
 * [npairs] may be NULL. */
typedef struct {
    int32_t min_mapq, max_scan;
} drm_tlen_params;
typedef struct {
    int32_t cls, tlen, mapq1, mapq2;
} drm_tlen_sample;
int drm_tlen_scan(const drm_mapq_params *mp, const drm_tlen_params *tp, const uint64_t *ids1, const int32_t *scores1,
                  const int32_t *cnt1, const uint64_t *ids2, const int32_t *scores2, const int32_t *cnt2,
                  const int32_t *full1, const int32_t *full2, int64_t npairs, int32_t k, int64_t row_step,
                  drm_tlen_sample *samples, uint32_t *hist);
/* Device-buffer form, enqueued on `stream`. Stateless: no handle, the current device. It consumes
 * drm_post_process_sw_{static,dynamic}_device's d_top_ids, d_top_scores and d_status unchanged. */
int drm_tlen_scan_device(const drm_mapq_params *mp, const drm_tlen_params *tp, const uint64_t *d_ids1,
                         const int32_t *d_scores1, const int32_t *d_cnt1, const uint64_t *d_ids2,
                         const int32_t *d_scores2, const int32_t *d_cnt2, const int32_t *d_full1,
                         const int32_t *d_full2, int64_t npairs, int32_t k, int64_t row_step,
                         drm_tlen_sample *d_samples, uint32_t *d_hist, void *stream);
/* Host only, no device, integers throughout: the window of one histogram row, hist_row[nbins] with bin T the number
 * of samples of template length T. The steps are bwa-mem's mem_pestat (outliers beyond 2 IQR, mapping bound 3 IQR,
 * 4 standard deviations) restated on a histogram:
 *   1. n = the sum of hist_row[T] over T in [1, nbins). n < min_samples: status 1, every other field 0. Otherwise
 *      status 0.
 *   2. With a[0..n) the samples in ascending order, p25, p50, p75 = a[min(n - 1, floor(q * n / 4))], q = 1, 2, 3.
 *   3. iqr = p75 - p25; trim_lo = max(1, p25 - 2 * iqr); trim_hi = min(nbins - 1, p75 + 2 * iqr).
 *   4. Over the samples in [trim_lo, trim_hi]: x = n_trim their number (>= 1), S1 = sum T, S2 = sum T^2, both exact
 *      (128 bits); V = x * S2 - S1^2 (>= 0); R = floor(sqrt(V)), an integer square root.
 *   5. mean = floor((2 * S1 + x) / (2 * x)); sd = floor((2 * R + x) / (2 * x)): both rounded half up.
 *   6. low = max(1, min(p25 - 3 * iqr, floor((S1 - 4 * R) / x))), the division flooring toward minus infinity.
 *   7. high = max(p75 + 3 * iqr, ceil((S1 + 4 * R) / x)).
 * DRM_ERR_ARG: a null pointer, nbins outside [2, 2^16 + 1], min_samples < 1. */
typedef struct {
    int64_t n, n_trim;
    int32_t p25, p50, p75, trim_lo, trim_hi, mean, sd, low, high, status;
} drm_tlen_estimate_t;
int drm_tlen_estimate(const uint32_t *hist_row, int32_t nbins, int32_t min_samples, drm_tlen_estimate_t *out);

/* ---------------------------------------------------------------- Multi-contig references
 * A FASTA of several sequences is mapped through the one string g that drm_extract_fasta_sequence returns for it, and a
 * contig table says which stretches of g are contigs. The reference treats every FASTA as one sequence, so this text is
 * the definition.
 * Contig table of a FASTA. Lines end at '\n'. The first line must start with '>': it is contig 0's header and adds
 * nothing to g. Every later line whose first byte is '>' is a header too; its A/C/G/T/N letters (either case) are part
 * of g, as drm_extract_fasta_sequence keeps them, and form a gap that belongs to no contig: the next contig starts at
 * the length of g after them. A contig's len is the number of letters appended to g from its header to the next header
 * or the end of the file; its name is the header after '>', up to the first white-space byte. So
 * g[start, start + len) is exactly the contig's sequence, and the table is ascending and disjoint.
 * DRM_ERR_FORMAT, the message naming the contig by index and name: a first line without '>', an empty or a duplicate
 * name, a contig of length 0, and a sequence line holding a non-space byte that drm_extract_fasta_sequence drops
 * (IUPAC R or Y, say: it would shift every later coordinate against the FASTA's own).
 * Two calls: with starts == NULL, *n receives the number of contigs and *names_bytes the size of the names, each
 * followed by a NUL; then, with *n and *names_bytes the capacities (DRM_ERR_ARG when too small), starts[*n], lens[*n]
 * and names[*names_bytes] are filled (lens and names may be NULL). */
int drm_fasta_contigs(const char *path, int64_t *n, int64_t *starts, int64_t *lens, char *names, int64_t *names_bytes);
/* A contig table for `device`: 1 <= n <= 2^20 contigs, starts ascending, lens >= 1, start + len <= the next start and
 * <= 2^40 (DRM_ERR_ARG otherwise). Host pointers. Where `device` exists the table is copied to it here, synchronously,
 * and the caller's current device is left as it was. Without a device the handle still serves drm_contigs_find, and
 * the copy is made by the first drm_contig_hits[_device] that has reads to process: that one call then allocates and
 * copies synchronously before it enqueues, so it must not run inside a stream capture. */
typedef struct drm_contigs drm_contigs;
int drm_contigs_create(const int64_t *starts, const int64_t *lens, int64_t n, int device, drm_contigs **out);
int drm_contigs_free(drm_contigs *c);
/* Host only: *contig = the contig t with start_t <= pos and pos + span <= start_t + len_t, or -1 (pos < 0, span < 0
 * or a sum beyond int64: -1). Of two adjoining contigs an empty span at their seam belongs to the later one: t is the
 * last contig that starts at or before pos, as in the contig stage. */
int drm_contigs_find(const drm_contigs *c, int64_t pos, int64_t span, int32_t *contig);
/* The largest table the contig stage searches in LDS; a larger one is searched in global memory (L2). */
int drm_contig_lds_max(void);
/* The contig stage: the step between the rerank and everything that consumes its rows. ids / scores [nreads x k] and
 * cnt[nreads] are a rerank's outputs, a count outside [0, k] being clamped as everywhere. For read r, over its counted
 * rows in order, with p = id >> 1 compared in unsigned 64-bit arithmetic: a row is kept iff some contig t has
 * start_t <= p and p + ref_len <= start_t + len_t, i.e. its window lies wholly inside one contig. The score does not
 * decide: a dead row (score 0) inside a contig stays. The kept rows are written in their original order to rows
 * 0 .. m - 1 of out_ids = id, out_spread = id + (t << 33), out_scores = score, out_contig = t, and out_cnt[r] = m;
 * rows m .. k - 1 get ids and spread ids 2^64 - 1, score 0 and contig -1.
 * A spread id is the position shifted by t * 2^32. drm_pair_hits, drm_hit_mapq, drm_pair_mapq and drm_tlen_scan accept
 * any u64 id and their distances (max_tlen <= 2^30, locus_span <= 2^20, max_scan <= 2^16) are below 2^32, while the
 * table is ascending, so that two rows of different contigs lie at least 2^32 apart: fed spread ids they never pair,
 * merge or measure across a contig boundary, and inside one contig they see the differences they see with the real
 * ids. Spread positions stay below 2^20 * 2^32 + 2^40 < 2^63.
 * Arguments: 0 <= k <= 1024 (beyond: DRM_ERR_UNSUPPORTED), 1 <= ref_len <= 2^20, nreads >= 0, no null pointer, and
 * no output overlapping an input or another output (DRM_ERR_ARG otherwise). Runs on the table's device.
 * Host pointers; out arrays [nreads x k], out_cnt[nreads]. */
int drm_contig_hits(const drm_contigs *c, int32_t ref_len, const uint64_t *ids, const int32_t *scores,
                    const int32_t *cnt, int64_t nreads, int32_t k, uint64_t *out_ids, uint64_t *out_spread,
                    int32_t *out_scores, int32_t *out_contig, int32_t *out_cnt);
/* Device-buffer form, enqueued on `stream`. It consumes drm_post_process_sw_{static,dynamic}_device's d_top_ids,
 * d_top_scores and d_status unchanged, and its outputs feed the device forms of drm_pair_hits, drm_hit_mapq,
 * drm_pair_mapq and drm_tlen_scan unchanged. Like every handle-based call it makes the handle's device the current
 * one and leaves it so. */
int drm_contig_hits_device(const drm_contigs *c, int32_t ref_len, const uint64_t *d_ids, const int32_t *d_scores,
                           const int32_t *d_cnt, int64_t nreads, int32_t k, uint64_t *d_out_ids,
                           uint64_t *d_out_spread, int32_t *d_out_scores, int32_t *d_out_contig, int32_t *d_out_cnt,
                           void *stream);

/* ---------------------------------------------------------------- Duplicate marking (a first-seen set)
 * A template (a read, or a pair) is a duplicate when an earlier template of the run has the same unclipped 5' ends on
 * the same strands; the first one seen stays unmarked, as in samblaster. No sort is needed: the ends of every template
 * so far live in a hash set on the device. The reference has no such step, so this text is the definition.
 *
 * drm_sam_end5 (host only): *end5 = the 0-based forward-strand coordinate under the read's first sequenced base, were
 * its leading clip aligned without gaps. With lead = a->q_begin - tag_prefix:
 *   forward (reverse == 0):  region_start + a->ref_begin - lead
 *   reverse:                 region_start + region_len - 1 - a->ref_begin + lead
 * the record being relative to the region genome[region_start ..+ region_len) as in drm_sam_cigar_region; for a window
 * record (drm_sw_align) the region is (window_id / 2, ref_len, window_id & 1), as in drm_sam_cigar. It may be negative,
 * by at most the query length. It is the unclipped 5' end that samtools or Picard derive from the printed line: forward,
 * 1-based, POS minus the leading S; reverse, POS + reference span - 1 + the trailing S of the printed (reversed) CIGAR.
 * Under a contig table the coordinate is that of the one genome string, so contigs need no key bits of their own; a
 * clip that reaches past a contig's end is keyed where it would lie in that string.
 * Examples: q_begin 4, tag_prefix 1, ref_begin 5, region (92, 166): forward 92 + 5 - 3 = 94; reverse 92 + 165 - 5 + 3 =
 * 255. DRM_ERR_ARG: a null pointer, a->status != 0, tag_prefix < 0 or q_begin < tag_prefix (the alignment reaches into
 * the prefix tag). */
int drm_sam_end5(const drm_sw_alignment *a, int32_t tag_prefix, int64_t region_start, int32_t region_len,
                 int32_t reverse, int64_t *end5);
/* The end word of one mapped mate (host only): *word = (((uint64_t)(end5 + 2^20) << 1) | (reverse != 0)) + 1, for
 * -2^20 <= end5 < 2^61 (DRM_ERR_ARG outside, or a null pointer). Word 0 means "this mate is unmapped".
 * Examples: (0, 0) -> 2^21 + 1; (-2^20, 1) -> 2; (94, 1) -> ((2^20 + 94) << 1) + 2. */
int drm_dup_end_word(int64_t end5, int32_t reverse, uint64_t *word);
/* The key of an item with the end words (e1, e2) is the unordered pair lo = min(e1, e2), hi = max(e1, e2): which mate
 * is mate 1 does not matter, F1R2 and F2R1 over the same ends are duplicates, as in Picard. A single read is the item
 * (e, 0), and so is a pair with one unmapped mate. An item with hi == 0 has no key and is never a duplicate of anything.
 *
 * The set. Items are numbered over the whole run; a call marks items first_item .. first_item + n, where first_item must
 * be >= the set's next_item (a gap is allowed) and first_item + n <= max_items; the call then sets next_item =
 * first_item + n. first[i] is the smallest item index, over all calls so far including this one, that has item i's
 * key, and -1 for an item without a key; item i is a duplicate iff 0 <= first[i] != first_item + i. Earlier calls hold
 * smaller indices, so "smallest index" is "first seen", and the answers do not depend on how the run is cut into calls.
 * n == 0 is DRM_OK and touches nothing. DRM_ERR_ARG, nothing touched: a null pointer (with n > 0), n < 0, first_item <
 * next_item, first_item + n > max_items. Limits: 1 <= max_items <= 2^31.
 * The handle owns keys[max_items] (16 bytes each: lo, hi) and slots, the smallest power of two >= 2 * max_items of
 * 8 bytes each, a slot holding 0 or item index + 1: 32 to 48 bytes of device memory per item of capacity. The home slot
 * of a key is
 *   z = lo ^ rotl64(hi, 32); z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9; z = (z ^ (z >> 27)) * 0x94D049BB133111EB;
 *   slot = (z ^ (z >> 31)) & (slots - 1)
 * (splitmix64's finaliser) and a key lives in the first slot from there, wrapping at the end, that was empty when its
 * first item arrived (linear probing). Results never depend on the hash; drm_dup_slot (host only)
 * returns the home slot so that a test can restate the probing. slots must be a power of two in [1, 2^32].
 * Like the other handles a set is single-stream: calls on one set must be serialised in stream order.
 * drm_dupset_mark: host pointers, ends [n x 2], first [n]; runs on the set's device and returns when done.
 * drm_dupset_mark_device: device pointers on the set's device, enqueued on `stream`; it makes the set's device the
 * current one and leaves it so. */
int drm_dup_slot(uint64_t lo, uint64_t hi, int64_t slots, int64_t *slot);
typedef struct drm_dupset drm_dupset;
int drm_dupset_create(int64_t max_items, int device, drm_dupset **out);
int drm_dupset_free(drm_dupset *s);
int drm_dupset_get_info(const drm_dupset *s, int64_t *max_items, int64_t *slots, int64_t *next_item);
int drm_dupset_mark(drm_dupset *s, const uint64_t *ends, int64_t n, int64_t first_item, int64_t *first);
int drm_dupset_mark_device(drm_dupset *s, const uint64_t *d_ends, int64_t n, int64_t first_item, int64_t *d_first,
                           void *stream);

/* ---------------------------------------------------------------- Coordinate order (a stable GPU radix sort)
 * bin/pipeline's DRM_SAM_SORT=coordinate writes the SAM lines in samtools sort's order: by the index of RNAME among the
 * @SQ lines, then POS, then forward before reverse; lines whose RNAME is "*" last; lines of equal key in the order in
 * which the unsorted file has them. The reference has no such step, so this text is the definition.
 *
 * drm_sam_sort_key (host only): the key of one line. tid = the index of the line's RNAME among the @SQ lines (0
 * without a contig table), -1 for RNAME "*"; pos = the POS column as printed (1-based, 0 allowed); reverse = flag & 16.
 *   tid == -1:  *key = 2^64 - 1
 *   otherwise:  *key = (((uint64_t)tid << 33 | pos) << 1) | (reverse != 0),  0 <= tid < 2^29, 0 <= pos < 2^33
 * DRM_ERR_ARG: a null pointer, tid < -1 or >= 2^29, pos < 0 or >= 2^33 (with tid == -1 pos and reverse are not looked
 * at). The key is strictly increasing in (tid, pos, reverse) taken lexicographically, and 2^64 - 1 is above all of them.
 * An unmapped mate that carries its mate's RNAME and POS gets that key and so sorts beside its mate; a secondary line
 * sorts by its own position. Examples: (0, 1, 0) -> 2; (0, 1, 1) -> 3; (2, 100, 1) -> ((2 * 2^33 + 100) << 1) + 1. */
int drm_sam_sort_key(int64_t tid, int64_t pos, int32_t reverse, uint64_t *key);
/* The sort. order[i] = the input index of the key that comes i-th in ascending order; among equal keys the smaller
 * index comes first (a stable sort: the result is the one permutation np.argsort(keys, kind="stable") gives, in every
 * run). keys is not modified. n == 0 is DRM_OK before any device call; n >= 2^31 is DRM_ERR_UNSUPPORTED; n < 0, a null
 * pointer with n > 0, a negative device, or (device form) a null or too small workspace is DRM_ERR_ARG; in all of these
 * nothing is launched.
 * A least-significant-digit radix sort over the keys' eight bytes with the index as 32-bit payload (DESIGN.md sec.
 * 4.19): one pass over the keys counts every byte's values; a byte that is the same in every key costs nothing more,
 * nor does a byte that only tells the all-ones keys from the rest when a lower byte does the same;
 * every other byte costs a count, a scan and a scatter in which wave64 ballots place each key. No atomic decides a
 * destination. drm_sort_tile returns the keys one block scatters (a tile), drm_sort_scan_tiles the tiles one step of
 * the scan covers; both are there so that a test can aim at the boundaries.
 * drm_sort_order: host arrays in and out; runs on `device` and returns when done.
 * drm_sort_order_device: device memory on the current device, enqueued on `stream` (a hipStream_t, null = the default
 * stream); nothing is copied back to the host in between, so the call returns before the sort ran. d_work is scratch
 * memory of at least *bytes of drm_sort_order_workspace(n) (about 20 bytes per key, plus 1 KiB per tile); its content
 * before and after the call means nothing. d_keys, d_order and d_work must not overlap. */
int drm_sort_tile(void);
int drm_sort_scan_tiles(void);
int drm_sort_order(const uint64_t *keys, int64_t n, int device, uint32_t *order);
int drm_sort_order_workspace(int64_t n, size_t *bytes);
int drm_sort_order_device(const uint64_t *d_keys, int64_t n, uint32_t *d_order, void *d_work, size_t work_bytes,
                          void *stream);

/* ---------------------------------------------------------------- BAM output (BGZF on the GPU, the record encoder)
 * bin/pipeline's DRM_SAM_FORMAT=bam writes results.bam instead of results.sam: the BAM header, one alignment record per
 * line the SAM would have held, in the same order, compressed as BGZF, closed by the empty EOF member. The reference has
 * no BAM output, so this text, SAMv1 sec. 4 and RFC 1951 / 1952 are the definition.
 *
 * BGZF. Input byte i belongs to block i / 65280 (drm_bgzf_block, htslib's BGZF_BLOCK_SIZE). Every block becomes one gzip
 * member, and the members follow each other without gaps:
 *   1f 8b 08 04 | 00 00 00 00 | 00 ff | 06 00 | 42 43 02 00 | BSIZE-1 (u16 LE)
 *   raw DEFLATE payload: one block with BFINAL = 1
 *   CRC-32 of the block's bytes (u32 LE) | ISIZE = the block's length (u32 LE)
 * BSIZE is the member's length. The payload is fixed Huffman (BTYPE = 01: LZ77 matches of length 4 .. 258 at distance
 * 1 .. 32768 that neither start before the block's first byte nor end after its last, the codes of RFC 1951 sec. 3.2.6,
 * end of block, zero bits up to a byte) unless that would be longer than len + 5 bytes; then it is stored (BTYPE = 00:
 * 01 | LEN | ~LEN | the bytes). A member is therefore at most len + 31 bytes, drm_bgzf_bound(n) = n + 31 * ceil(n /
 * 65280) bounds a stream, and every member can be inflated on its own. No dynamic Huffman tables.
 * A member is a function of its block's bytes alone: the same in every run, wherever the block sits in a call, whatever
 * else the device does (bgzf.hip: the match candidates come from LDS atomicMax / atomicMin updates, which do not depend
 * on their order, and the greedy parse is resolved by pointer jumping). So compress(A || B) = compress(A) || compress(B)
 * whenever |A| is a multiple of 65280.
 * drm_bgzf_eof: the 28 bytes of the empty member that ends a BGZF file,
 *   1f 8b 08 04 00 00 00 00 00 ff 06 00 42 43 02 00 1b 00 03 00 00 00 00 00 00 00 00 00.
 * drm_bgzf_compress: host memory in and out; runs on `device`, on a stream of its own that it alone waits for (a thread
 * may call it while another drives other streams), with stream-ordered copies through pinned staging, in rounds of 256
 * blocks (the environment variable DRM_BGZF_ROUND, read at every call, sets another number in [1, 2^20], anything else
 * being DRM_ERR_ARG; the stream does not depend on it). *bytes gets the stream's length. n == 0 is DRM_OK with 0 bytes before any device call; n < 0, a null pointer with n > 0, a negative
 * device or cap < drm_bgzf_bound(n) is DRM_ERR_ARG with nothing launched. Calls are serialised inside.
 * drm_bgzf_compress_device: device memory on the current device, enqueued on `stream` (a hipStream_t, null = the default
 * stream); nothing is copied back in between, so the call returns before the kernels ran. d_sizes [ceil(n / 65280)] gets
 * every member's length, the packed stream starts at d_out, which holds drm_bgzf_bound(n) bytes; d_work is scratch of at
 * least *bytes of drm_bgzf_workspace(n) (64 KiB per block, plus 255 KiB for each of up to 512 workgroups). d_data, d_out,
 * d_sizes and d_work must not overlap. The same argument errors, plus a null or too small workspace. */
int drm_bgzf_block(void);
int drm_bgzf_bound(int64_t n, size_t *bytes);
int drm_bgzf_eof(uint8_t out[28]);
int drm_bgzf_compress(const uint8_t *data, int64_t n, int device, uint8_t *out, size_t cap, size_t *bytes);
int drm_bgzf_workspace(int64_t n, size_t *bytes);
int drm_bgzf_compress_device(const uint8_t *d_data, int64_t n, uint8_t *d_out, uint32_t *d_sizes, void *d_work,
                             size_t work_bytes, void *stream);
/* The BAM bytes in front of compression (host only; SAMv1 sec. 4.2). Both write *bytes = the length even when cap is too
 * small, which is DRM_ERR_ARG, as is a null pointer.
 * drm_bam_header: "BAM\1", l_text, the text as given, n_ref, and for every line of the text that starts with "@SQ\t", in
 * order, l_name (counting the NUL), the name from SN:, NUL, l_ref from LN:. An @SQ line without SN or LN: DRM_ERR_ARG.
 * drm_bam_record: one SAM text line (a trailing newline is allowed) as one alignment record, block_size first.
 *   refID, next_refID  the index of RNAME / RNEXT in ref_names; "*" gives -1, RNEXT "=" the line's own refID
 *   pos, next_pos      POS - 1, PNEXT - 1 (0 in the text becomes -1)
 *   bin                reg2bin(pos, pos + max(1, reference bases of the CIGAR)) of SAMv1 sec. 5.3 with arithmetic shifts
 *                      (4680 for pos = -1), its low 16 bits
 *   l_read_name        counts the NUL; a QNAME over 254 bytes is DRM_ERR_UNSUPPORTED
 *   cigar              len << 4 | op over MIDNSHP=X; "*" = none
 *   seq                4 bits a base over =ACMGRSVTWYHKDBN, high nibble first, any other character 15; "*" = l_seq 0
 *   qual               the character minus 33; "*" = 0xFF for every base
 *   tags               i: the smallest of C S I that holds a value >= 0, of c s i for a negative one (samtools' rule);
 *                      Z: the text and a NUL; A: one byte; any other type is DRM_ERR_UNSUPPORTED
 * DRM_ERR_ARG: fewer than eleven columns, a FLAG, POS, MAPQ, PNEXT, TLEN or i tag that is no number (or outside its
 * field), a CIGAR that does not parse, a QUAL of another length than SEQ, an RNAME or RNEXT that is not among the names, a
 * tag that is not XX:T:value. The SAM writers feed the same encoder the line they built, not its text. */
int drm_bam_header(const char *sam_header_text, size_t len, uint8_t *out, size_t cap, size_t *bytes);
int drm_bam_record(const char *line, size_t len, const char *const *ref_names, int32_t n_ref, uint8_t *out, size_t cap,
                   size_t *bytes);

/* ---------------------------------------------------------------- L2 rerank (the reference's live path)
 * post_process_l2_static (src/utils/post_processor.cpp:1023-1162, called at src/main.cpp:330) ->
 * find_sequences (static) -> Vectorizer::vectorize of the candidate windows -> batch_reranker(k = k_clusters)
 * (src/utils/reranker.cpp:98-195) -> calc_l2_dist (src/utils/metrics.cpp:48-61).
 * drm_refs_embed fills a device table of every window's embedding with the read encoder (the reference
 * re-embeds each candidate window per run; the encoder is a deterministic function of the window, so the
 * table row is the same vector) -- n_ref x 128 f32 of HBM, synchronous on `stream`. Encoder and window
 * table must be on the same device. drm_refs_embeddings returns the table's device pointer (NULL before
 * drm_refs_embed) and its width. */
int drm_refs_embed(drm_refs *refs, drm_encoder *enc, void *stream);
int drm_refs_embeddings(drm_refs *refs, const float **d_emb, int32_t *dim);
/* neighbors [nq x kk] (every label is a candidate, as in the reference), query_emb [nq x d] f32 (the search's
 * query embeddings). Outputs [nq x k_clusters]: top_dists (sqrtf of the rounded squares summed in index order, ascending,
 * libstdc++ std::partial_sort's order among ties), top_ids (window ids), counts[nq] (k_clusters, or 0 for
 * kk == 0). stride > 1 reproduces the reference's global expansion stream (query q reranks stream entries
 * [q*kk*stride, (q+1)*kk*stride) of the whole call), so such a call must not be split into batches.
 * Errors: DRM_ERR_ARG "Invalid mapping index in expansion" (a label outside the table, or a range past the
 * stream: the reference throws or reads out of bounds), DRM_ERR_CANDS (kk*stride < k_clusters); *bad_query
 * receives the first offending query. Host pointers. */
int drm_post_process_l2_static(drm_refs *refs, const int64_t *neighbors, int64_t nq, int32_t kk,
                               const float *query_emb, int32_t d, int64_t stride, int32_t k_clusters,
                               float *top_dists, uint64_t *top_ids, int32_t *counts, int64_t *bad_query);
/* Device-buffer form on `stream`; d_status[nq]: k_clusters or 0 = rows emitted, -1 = not enough candidates,
 * -4 = invalid label / range past the stream. */
int drm_post_process_l2_static_device(drm_refs *refs, const int64_t *d_neighbors, int64_t nq, int32_t kk,
                                      const float *d_query_emb, int32_t d, int64_t stride, int32_t k_clusters,
                                      float *d_top_dists, uint64_t *d_top_ids, int32_t *d_status, void *stream);
/* post_process_l2_dynamic / post_process_l2_dynamic_streaming's rerank (src/utils/post_processor.cpp:553-750,
 * :752-1021) on a genome handle embedded with drm_refs_embed (a genome handle embeds windows [0, glen): the
 * positions the sparse expansion can reach, window w = genome[w/2 ..+ ref_len), reverse-complemented for odd
 * w). stride > 1 only -- at stride 1 the reference reranks nothing and returns the first min(k, k_clusters)
 * search neighbours with their search distances (DRM_ERR_ARG here). Each query contributes its first
 * min(k_clusters, kk) labels to one global expansion stream (positions checked against the genome length)
 * and reranks the stream entries [q*nc, (q+1)*nc), nc = min(k_clusters, kk) * (2*stride - 1), keeping k rows
 * ([nq x k] outputs). Errors as drm_post_process_l2_static, plus DRM_ERR_K (k > k_clusters*2*stride). */
int drm_post_process_l2_dynamic(drm_refs *refs, const int64_t *neighbors, int64_t nq, int32_t kk,
                                const float *query_emb, int32_t d, int64_t stride, int32_t k, int32_t k_clusters,
                                float *top_dists, uint64_t *top_ids, int32_t *counts, int64_t *bad_query);
int drm_post_process_l2_dynamic_device(drm_refs *refs, const int64_t *d_neighbors, int64_t nq, int32_t kk,
                                       const float *d_query_emb, int32_t d, int64_t stride, int32_t k,
                                       int32_t k_clusters, float *d_top_dists, uint64_t *d_top_ids, int32_t *d_status,
                                       void *stream);

/* ---------------------------------------------------------------- batch executor (exec.cpp)
 * Pinned host memory: buffers from drm_host_alloc make the executor's host <-> device copies DMA
 * transfers that overlap the kernels; ordinary (pageable) buffers work too, staged by the runtime. */
int drm_host_alloc(void **ptr, size_t bytes);
int drm_host_free(void *ptr);

/* The fused search -> SW rerank of one batch driver pass (SURVEY.md sec. 8b `drm_search_rerank`): the
 * reference's faiss_search(index, emb, k_clusters, ef) followed by post_process_sw_static(neighbors,
 * distances, ref_seqs, query_seqs, ref_len, stride, k, k_clusters) (src/main.cpp:278, :333-341), run as
 * batches streamed through the device (host->device copies, kernels and device->host copies of
 * consecutive batches overlap on two streams; batch size DRM_BATCH, default 262144 queries).
 * Host pointers throughout:
 *   x [n x d] f32 -> D [n x k_clusters] f32, I [n x k_clusters] int64 (drm_search's outputs);
 *   refs == NULL: search only (queries ... status ignored); a genome handle (drm_refs_create_genome)
 *   reranks with the dynamic lookup (post_process_sw_dynamic), a window table with the static one;
 *   else queries [n x q_stride] bytes with q_len[n] -> sw_scores / sw_ids [n x k] and status[n]
 *   (drm_post_process_sw_static_device's per-query status: k or 0 rows emitted, -1 not enough
 *   candidates, -2 / -3 candidate or length limits).
 * Errors: those of drm_search, plus DRM_ERR_K / DRM_ERR_CANDS / DRM_ERR_UNSUPPORTED as
 * drm_post_process_sw_static reports them (the outputs of the other queries are still written).
 * stats->kernel_ms is the device span of the compute stream. */
int drm_search_rerank(drm_index *index, drm_refs *refs, const float *x, int64_t n, int32_t d, int32_t k_clusters,
                      int32_t ef, const uint8_t *queries, const int32_t *q_len, int32_t q_stride, int64_t stride,
                      int32_t k, float *D, int64_t *I, int32_t *sw_scores, uint64_t *sw_ids, int32_t *status,
                      drm_search_stats *stats);

/* The same search -> SW rerank on DEVICE-resident buffers (shapes as drm_search_rerank; d_ndis, d_nhops,
 * d_nhops_upper may be NULL), enqueued on `stream`: the search, then the rerank, each with the whole chip
 * (co-scheduling them on shared CUs measured slower at C5 and was removed in round 5). The
 * outputs equal those of drm_search_device + drm_post_process_sw_static_device (or _dynamic_device for a genome
 * handle). d_status must be checked by the caller, and search errors read with drm_index_search_errors. stats
 * (may be NULL) makes the call synchronous and returns the device span and the search / rerank spans
 * (n_batches = 1; first_search_ms = search_ms, last_sw_ms = sw_ms). */
typedef struct {
    int64_t nq;
    int32_t n_batches;
    double kernel_ms;       /* device span: first search start -> last rerank end */
    double search_ms;       /* the search's span */
    double sw_ms;           /* the rerank's span */
    double first_search_ms; /* = search_ms (one batch) */
    double last_sw_ms;      /* = sw_ms (one batch) */
} drm_pipeline_stats;
int drm_search_rerank_device(drm_index *index, drm_refs *refs, const float *d_x, int64_t n, int32_t k_clusters,
                             int32_t ef, const uint8_t *d_queries, const int32_t *d_q_len, int32_t q_stride,
                             int64_t stride, int32_t k, float *d_D, int64_t *d_I, int32_t *d_ndis, int32_t *d_nhops,
                             int32_t *d_nhops_upper, int32_t *d_sw_scores, uint64_t *d_sw_ids, int32_t *d_status,
                             void *stream, drm_pipeline_stats *stats);

/* Optional: set up drm_search_rerank's streams and device buffers for a batch of n queries ahead of the
 * call (q_stride = 0: search only), and do the first-use work there (the copy engines' first DMA, the
 * search kernel's first launch), so the call itself only streams data and runs kernels. */
int drm_search_rerank_prepare(drm_index *index, int64_t n, int32_t d, int32_t k_clusters, int32_t k, int32_t q_stride);

/* ---------------------------------------------------------------- multi-GPU fan-out
 * One index replica (and window table, when windows != NULL) per entry of devices[ndev] -- the same
 * device may appear more than once. drm_multi_search_rerank splits the n queries into contiguous
 * shards [r*n/ndev, (r+1)*n/ndev), runs drm_search_rerank for shard r on devices[r] from its own host
 * thread, and writes every shard straight into the caller's outputs (same arguments and outputs as
 * drm_search_rerank; stats summed, kernel_ms the slowest shard). Outputs are byte-identical to a
 * one-device run: queries are independent (src/utils/post_processor.cpp:491). */
typedef struct drm_multi drm_multi;
int drm_multi_create(const char *index_path, const int *devices, int ndev, const uint8_t *windows, int64_t n_ref,
                     int32_t ref_len, int64_t row_stride, drm_multi **out);
/* The same with the dynamic lookup: a genome handle per device (drm_refs_create_genome). */
int drm_multi_create_genome(const char *index_path, const int *devices, int ndev, const uint8_t *genome, int64_t len,
                            int32_t ref_len, drm_multi **out);
int drm_multi_free(drm_multi *m);
int drm_multi_get_index_info(const drm_multi *m, drm_index_info *info); /* replica 0's info */
int drm_multi_search_rerank(drm_multi *m, const float *x, int64_t n, int32_t d, int32_t k_clusters, int32_t ef,
                            const uint8_t *queries, const int32_t *q_len, int32_t q_stride, int64_t stride, int32_t k,
                            float *D, int64_t *I, int32_t *sw_scores, uint64_t *sw_ids, int32_t *status,
                            drm_search_stats *stats);

/* ---------------------------------------------------------------- RCCL result gather (one process per GPU)
 * A communicator over the nranks processes of a job (rank 0 creates the id with drm_comm_unique_id and
 * hands it to the others out of band, e.g. over the job's gloo/TCP control plane).
 * drm_comm_gather_rows: rank r holds rows [r*n_total/nranks, (r+1)*n_total/nranks) of a row-major
 * [n_total x row_bytes] result in d_send (device memory); the root receives all n_total rows in d_recv
 * over RCCL point-to-point transfers (xGMI), enqueued on `stream`. */
#define DRM_COMM_ID_BYTES 128
typedef struct drm_comm drm_comm;
int drm_comm_unique_id(uint8_t *id);
int drm_comm_init(const uint8_t *id, int nranks, int rank, int device, drm_comm **out);
int drm_comm_free(drm_comm *comm);
int drm_comm_gather_rows(drm_comm *comm, const void *d_send, int64_t n_total, int64_t row_bytes, void *d_recv, int root,
                         void *stream);
/* drm_index_broadcast: the index replicated from one GPU to every rank over RCCL ("index
 * broadcast from GPU0"), in place of every rank parsing the IHNp file (drm_index_load; src/main.cpp:236-237 is
 * the load it replaces on ranks != root). Collective: every rank of `comm` calls it, on the communicator's device.
 * The root passes its loaded index in root_index (other ranks pass NULL); every other rank receives a new index in
 * *out. At the root `out` may be NULL (its index is the replica) or non-NULL for a separate copy (what a
 * one-rank job uses to exercise the receive side). The header goes first (shape, levels, entry point, kept
 * metadata, and the root's checksum of each buffer), then the PQ centroids, codes, level-0 rows and upper-level
 * lists in one grouped ncclBroadcast; each receiver checks the checksums, derives the lean kernel's inline rows
 * itself and applies its own DRM_SEARCH_* load-time knobs. An argument, allocation or checksum failure on any rank
 * fails the call on every rank (an agreement step precedes each transfer, so none is left waiting). Synchronous. */
int drm_index_broadcast(drm_comm *comm, drm_index *root_index, int root, drm_index **out);

/* post_process_sw_dynamic (src/utils/post_processor.cpp:357-452) on a genome handle: the same
 * contract as drm_post_process_sw_static, with find_sequences' dynamic candidate rules (dense: every
 * one of the first min(k_clusters, kk) ids, an out-of-genome window scoring 0 and keeping its id;
 * sparse: the expansion checked against the genome length). */
int drm_post_process_sw_dynamic(drm_refs *refs, const int64_t *neighbors, int64_t nq, int32_t kk,
                                const uint8_t *queries, const int32_t *q_len, int32_t q_stride, int64_t stride,
                                int32_t k, int32_t k_clusters, int32_t *top_scores, uint64_t *top_ids,
                                int32_t *counts, int64_t *bad_query);
int drm_post_process_sw_dynamic_device(drm_refs *refs, const int64_t *d_neighbors, int64_t nq, int32_t kk,
                                       const uint8_t *d_queries, const int32_t *d_q_len, int32_t q_stride,
                                       int64_t stride, int32_t k, int32_t k_clusters, int32_t *d_top_scores,
                                       uint64_t *d_top_ids, int32_t *d_status, void *stream);

/* ---------------------------------------------------------------- index build (hnswpq_index)
 * build_faiss_index (src/hnswpq/index.cpp:86-193): trains PQ on an evenly spaced sample of
 * sample_rate*n vectors (create_training_set :57-84, Config::Build::SAMPLE_RATE = 0.5), builds the
 * HNSW graph (M_hnsw, efConstruction) with PQ-ADC distances and writes a faiss "IHNp" file.
 * nthreads <= 0 -> all cores; nthreads == 1 gives a deterministic graph. */
int drm_build_hnswpq(const float *x, int64_t n, int32_t d, int32_t M_pq, int32_t nbits, int32_t M_hnsw,
                     int32_t efConstruction, double sample_rate, int32_t nthreads, uint64_t seed,
                     const char *index_path);

/* The same build on one GPU (builder_gpu.hip), from DEVICE-resident vectors d_x [n x d] f32 (d = 128,
 * M_pq = 8, nbits = 8): PQ trained on the host on the same sample as drm_build_hnswpq, codes and the
 * graph built on `device` (batched insertion, ef = min(efConstruction, 256) beams, closest-first
 * neighbour selection), written as the same faiss "IHNp" file. For the 10M-50M synthetic configurations
 * (BASELINE.json configs[3..4]) that the host builder cannot produce inside a run. */
int drm_build_hnswpq_device(const float *d_x, int64_t n, int32_t d, int32_t M_pq, int32_t nbits, int32_t M_hnsw,
                            int32_t efConstruction, double sample_rate, uint64_t seed, int device,
                            const char *index_path);

/* build_index (src/hnswlib_dir/index.cpp:3-49): hnswlib HierarchicalNSW<float>(L2Space(d), n, M,
 * efConstruction), addPoint(x[i], label i) for all i, saveIndex -> an hnswlib file (the reference's
 * defaults: M = Config::Build::GPH_DEG = 64, EFC = 128, includes/utils/config.hpp:30-31). The graph
 * follows hnswlib's construction algorithm; it need not equal hnswlib's bit for bit. */
int drm_build_hnsw_flat(const float *x, int64_t n, int32_t d, int32_t M, int32_t efConstruction, int32_t nthreads,
                        uint64_t seed, const char *index_path);

/* ---------------------------------------------------------------- synthetic embedder
 * Stand-in for the OpenVINO read encoder (Vectorizer::vectorize, src/inference/vectorize.cpp:34-141,
 * OUT OF SCOPE): e(s) = normalize(sum_t R[3-mer(s, t)]) over ACGT 3-mers, R a [64 x dim] N(0,1)
 * matrix drawn from splitmix64(seed). Deterministic; used by the CLIs and the synthetic workloads so
 * that reads land near their source windows. seqs: n strings at seqs[off[i] .. +len[i]). */
int drm_embed_kmer3(const uint8_t *seqs, const int64_t *off, const int32_t *len, int64_t n, int32_t dim,
                    uint64_t seed, float *out);

/* drm_embed_kmer3 on the device for n fixed-length rows (d_rows[i * row_stride .. + len), len <= 512,
 * dim = 128), enqueued on `stream` and synchronised; bit-identical to drm_embed_kmer3. */
int drm_embed_kmer3_device(const uint8_t *d_rows, int64_t n, int32_t len, int64_t row_stride, int32_t dim,
                           uint64_t seed, float *d_out, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Read encoder: Vectorizer (src/inference/vectorize.cpp:4-141) =
 * Preprocessor::preprocess tokens (src/inference/preprocess.cpp:20-42) + the OpenVINO GRU model
 * (src/inference/fast_model.cpp:3-68, models/finetuned_sgn33-new-a-Apr6.xml) on the GPU.
 * -------------------------------------------------------------------------------------------*/
typedef struct {
    int32_t hidden, emb_dim, max_len, out_dim; /* 64, 64, 123 (config.hpp:21), 128 (config.hpp:22) */
    int32_t n_token_rows;                     /* 97: padding + the 96 _Tok2Index tokens */
    int32_t device;
    float h0;
    int64_t device_bytes;
} drm_encoder_info;

/* model_path: the reference's IR (.xml; weights from the sibling .bin, as core.read_model does,
 * fast_model.cpp:15) or a .drmenc file written by drm_encoder_export. DRM_ERR_UNSUPPORTED for any
 * graph other than embedding -> 2 x bidirectional GRU(64, linear_before_reset) with f16 weights. */
int drm_encoder_load(const char *model_path, int device, drm_encoder **out);
int drm_encoder_export(const char *model_path, const char *out_path); /* host only */
int drm_encoder_free(drm_encoder *enc);
int drm_encoder_get_info(const drm_encoder *enc, drm_encoder_info *info);
/* Preprocessor::preprocess + prepareBatch padding: tokens [n][max_len] model-input vocabulary ids
 * (0 = padding; -1 where the reference's hashToken indexes past its 96-entry table, which is
 * undefined behaviour there). seqs: n rows of `stride` bytes, lens[i] >= 2 (DRM_ERR_ARG otherwise). */
int drm_tokenize(drm_encoder *enc, const uint8_t *seqs, const int32_t *lens, int64_t n, int64_t stride, int32_t *tokens);
/* Vectorizer::vectorize: out [n][128] f32. n_undefined (optional): tokens that hit the reference's
 * undefined table read (encoded with the padding row). */
int drm_vectorize(drm_encoder *enc, const uint8_t *seqs, const int32_t *lens, int64_t n, int64_t stride, float *out,
                  int64_t *n_undefined);
/* device buffers + stream, asynchronous; lens must be >= 2 (shorter sequences encode as padding and
 * are counted by drm_encoder_flags). Like the index handles, an encoder handle is single-stream: its
 * layer-1 workspace is reused by every call, so calls must be serialised in stream order. */
int drm_vectorize_device(drm_encoder *enc, const uint8_t *d_seqs, const int32_t *d_lens, int64_t n, int64_t stride,
                         float *d_out, void *stream);
/* counters accumulated by drm_vectorize_device since the last call (synchronises the device) */
int drm_encoder_flags(drm_encoder *enc, int64_t *n_undefined, int64_t *n_short);

#ifdef __cplusplus
}
#endif
#endif
