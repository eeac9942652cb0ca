/*
 * quake_hip.h -- C ABI of libquake_hip.so: the MI355X (gfx950) implementation of Quake's
 * search / k-means hot path.
 *
 * The reference (marius-team/quake @ 2025-05-23) has NO C ABI or plugin registry: its boundary is the
 * C++ class API + pybind11.  These entry points are what the bodies of the
 * reference's C++ methods would bind when the hot path is delegated to the GPU; each one cites the
 * reference interface it replaces (paths relative to the reference checkout).  The host-side mirror of
 * the C++/Python surface (quake_amd/) is written against exactly this header.
 *
 * Conventions
 *   - plain pointers + sizes, no torch / C++ types; every function returns a qk_status (0 = ok) and
 *     records a message retrievable with qk_last_error() (the C++ side turns it into
 *     std::runtime_error / std::invalid_argument like the reference's throws).
 *   - `mem` says where the caller's data pointers live: QK_MEM_HOST (pageable or pinned host memory,
 *     what the reference's CPU tensors are) or QK_MEM_DEVICE (HBM of the context's device).
 *   - metric codes are faiss::MetricType's: 0 = inner product, 1 = L2 (common.h:145-156).
 *   - L2 results are sqrt distances, like the reference (list_scanning.h:260,286,353-357).
 *   - fewer than k results: ids -1, distances +inf (L2) / -inf (IP) (query_coordinator.cpp:589-601,774-788).
 *   - ordering is the total order (key, id) -- DESIGN.md section 3.
 *   - non-finite values: a (query, row) pair whose canonical float32 value -- the k-ordered fmaf chain; for L2 the
 *     expanded form with the clamp -- is NaN is NEVER a candidate: in qk_search, qk_scan, their filtered / per-query-filtered /
 *     tracked forms, wide rows, k > QK_MAX_K and qk_range_*, whatever the NaN's sign or payload, the row's position or the scan form.
 *     qk_coarse follows it: a NaN centroid is never probed, and the row is padded with -1 when fewer than kk centroids remain.
 *     +-inf are ordinary values, ordered as floats: a row at +inf (L2) / -inf (IP) is returned with its own id in front of the
 *     padding.  -0.0 and +0.0 tie and the lower id goes first; which sign a returned zero carries is unspecified.  Outside this
 *     rule: k-means on non-finite input (qk_kmeans*), qk_search_aps and the device group.
 *   - all work is enqueued on the context's HIP stream; host-memory outputs are complete on return,
 *     device-memory outputs are complete after qk_ctx_synchronize() (or stream order).
 */
#ifndef QUAKE_HIP_H
#define QUAKE_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define QK_API __attribute__((visibility("default")))

typedef enum {
    QK_OK = 0,
    QK_ERR_INVALID = 1,     /* bad argument (std::invalid_argument in the reference) */
    QK_ERR_NOT_FOUND = 2,   /* "List does not exist" (dynamic_inverted_list.cpp:71,79,87) */
    QK_ERR_HIP = 3,         /* HIP runtime error; also: a scan launched earlier on the context had to drop result records
                             * (its record buffer is sized by a host-side upper bound; the kernels raise a host-visible
                             * flag if that bound is ever wrong) -- reported by the call that synchronises, or the next call */
    QK_ERR_UNSUPPORTED = 4, /* outside the implemented envelope (e.g. k > QK_MAX_K) */
    QK_ERR_OOM = 5
} qk_status;

#define QK_METRIC_IP 0
#define QK_METRIC_L2 1
#define QK_MEM_HOST 0
#define QK_MEM_DEVICE 1
#define QK_MAX_K 448 /* largest k of the fused LDS top-k (pool capacity k+64 <= 512).  Larger k, up to 8192 -- the capacity
                      * of the reference's buffer (list_scanning.h:39) -- is served by emitting every key and selecting afterwards
                      * (slower, exact) */
#define QK_MAX_NPROBE 8192 /* largest nprobe / number of APS candidate partitions: the coarse step selects them with a
                              * bisection select + sort beyond QK_MAX_K (flat parent index) */
#define QK_MAX_D 8192 /* largest dimension, for every entry point and every k.  Up to d ~ 2500 (less with large k) the scan,
                       * dense and k-means kernels stage their 16-query tile in LDS; wider rows go to the wide-row siblings,
                       * which read the queries from global memory (same bits).  Larger d: QK_ERR_UNSUPPORTED */

typedef struct qk_ctx qk_ctx;     /* device + stream + scratch workspace                     */
typedef struct qk_store qk_store; /* device mirror of faiss::DynamicInvertedLists (one level) */

/* Per-call timing, filled from HIP events; mirrors the fields of SearchTimingInfo (common.h:214-228)
 * that still mean something on a GPU. */
typedef struct {
    float coarse_ms;  /* parent search (query_coordinator.cpp:644)            */
    float group_ms;   /* partition -> query grouping (query_coordinator.cpp:707-721) */
    float scan_ms;    /* partition scan kernel(s)                               */
    float merge_ms;   /* per-query merge + output                               */
    float total_ms;
    int64_t n_items;          /* work items scanned                              */
    int64_t scan_bytes;       /* algorithmic bytes of the scan: sum over unique probed partitions n_p*d*4 */
    int64_t partitions_scanned; /* (query, partition) pairs scanned              */
} qk_timing;

/* ---- errors ------------------------------------------------------------------------------------ */
QK_API const char *qk_last_error(void);
QK_API const char *qk_version(void);

/* ---- context ----------------------------------------------------------------------------------- */
/* device: HIP ordinal.  Creates a private non-blocking stream. */
QK_API int qk_ctx_create(int device, qk_ctx **out);
QK_API int qk_ctx_destroy(qk_ctx *ctx);
/* Run on a caller-owned hipStream_t instead (e.g. torch's current stream); NULL restores the private one. */
QK_API int qk_ctx_set_stream(qk_ctx *ctx, void *hip_stream);
/* Run on the device's NULL (legacy default) stream -- torch's default stream has the handle 0, which qk_ctx_set_stream reads
 * as "restore the private stream". */
QK_API int qk_ctx_set_null_stream(qk_ctx *ctx);
/* The stream the context is bound to now, so that a caller that rebinds it for one call can put the binding back:
 * kind 0 = the private stream (restore with qk_ctx_set_stream(ctx, NULL)), 1 = the NULL stream (qk_ctx_set_null_stream),
 * 2 = a caller-owned stream (*hip_stream; qk_ctx_set_stream(ctx, *hip_stream)). */
QK_API int qk_ctx_get_stream(qk_ctx *ctx, void **hip_stream, int *kind);
/* Form feedback (default on): the partition scan has several forms with identical results (16 x 16 tiles, per-wave row-per-lane
 * walk, mixed sequence with dense hot items); which is fastest depends on how the batch's queries concentrate on lists, which
 * the host cannot see.  With feedback on, a context times whole scan calls per (store, batch shape) with HIP events it reads
 * back later without synchronising, tries every admissible form twice, then uses the fastest and re-checks the others every
 * few hundred calls.  Off: the static rule alone (what the first call of a shape always uses).  No reference counterpart:
 * the reference picks serial / batched / worker scans by SearchParams (query_coordinator.cpp:612-673). */
QK_API int qk_ctx_set_form_feedback(qk_ctx *ctx, int enabled);
/* The feedback RULE on injected figures: with ms3 = {tile form, per-wave walk, mixed sequence} (all > 0) every measurement the
 * context harvests reads ms3[form] in place of the elapsed time of its event pair, so which form answers which call is a pure
 * function of the call sequence (tests/test_scan_feedback_gpu.py asserts the sequence).  NULL: measured times again.  The
 * environment variable QK_FORM_FEEDBACK=0 creates every context with feedback off. */
QK_API int qk_ctx_set_form_times(qk_ctx *ctx, const float *ms3);
/* The fp16 shadow form: qk_search with one list per query (nprobe = 1), k <= 16, d <= 256, L2 or IP, streams an
 * fp16 mirror of the store's rows -- half the bytes --, keeps the 32 best approximate keys per segment and finishes in fp32: every
 * candidate's canonical key is recomputed, the answer is verified against a bound of the approximation error, and a query that
 * does not verify is answered by an exact scan of its list.  Same bits as every other form.  mode 0 = never, 1 = automatic (the
 * default; QK_SHADOW in the environment overrides it at creation): the form feedback measures the form next to the tile form and
 * uses it where it is faster -- batches of >= 1024 queries; the shadow is built at the second such call on an unchanged store,
 * again after 8 calls once the store was modified --, 2 = forced: whenever eligible, whatever the batch size and the feedback,
 * building the shadow at once (tests).  qk_ctx_last_scan_kernel names "k_scan (fp16 shadow)".  No reference counterpart. */
QK_API int qk_ctx_set_shadow(qk_ctx *ctx, int mode);
/* queries the shadow form's finish verified / answered by the exact scan of their list, candidates re-scored in fp32, and queries
 * whose pair left more records than its slot line lists (the finish walked the record chain), since the context was created
 * (synchronises the stream).  Any pointer may be NULL. */
QK_API int qk_ctx_shadow_stats(qk_ctx *ctx, int64_t *verified, int64_t *fallback, int64_t *candidates, int64_t *chained);
/* The fourth figure of qk_ctx_set_form_times: ms > 0 is what a harvested measurement of the shadow form reads; 0 clears it.  While
 * three figures are injected and this one is not, the form is not admissible. */
QK_API int qk_ctx_set_shadow_form_time(qk_ctx *ctx, float ms);
/* The bound E the shadow form works with: |approximate key - canonical fp32 key| <= E for a query of norm qnorm whose fp16 image is
 * rho_q away from it, against rows of a store whose fp16 images are at most rho away and at most xmax long (Euclidean norms; a
 * distance to the image counts an fp16 subnormal as the farther of itself and zero).  Pure host arithmetic, no GPU needed;
 * DESIGN.md 5.20 has the derivation, tests/test_shadow_bound.py checks it against emulated arithmetic. */
QK_API float qk_shadow_error_bound(int metric, int d, float qnorm, float rho_q, float rho, float xmax);
QK_API int qk_ctx_synchronize(qk_ctx *ctx);
/* hipEvent timing of the phases, recorded on the context's stream around the kernels:
 *   0 off; 1 per call (the qk_timing* passed to qk_scan/qk_search is filled, which synchronises the stream);
 *   2 deferred (no synchronisation inside the calls; qk_ctx_read_timing sums everything recorded since the last read);
 *   3 deferred, scan kernel only: one event pair per call around the partition-scan kernel (an event record costs the stream
 *     a few microseconds; the 8 of mode 2 add ~10 % to a 0.35 ms search). */
QK_API int qk_ctx_set_timing(qk_ctx *ctx, int mode);
/* The mode set last (0 at creation): a caller that switches the mode for one call restores what it found
 * (QueryCoordinator::search fills SearchTimingInfo, query_coordinator.cpp:612-657, on a context others may be timing with). */
QK_API int qk_ctx_get_timing(qk_ctx *ctx, int *mode);
/* Synchronises, then returns the SUM of the phase durations over the calls recorded in deferred mode and their count. */
QK_API int qk_ctx_read_timing(qk_ctx *ctx, qk_timing *sum, int64_t *calls);
/* Device properties the harness prints: CU count, clock (kHz), total HBM bytes, gcnArchName. */
QK_API int qk_ctx_device_info(qk_ctx *ctx, int *num_cus, int *clock_khz, int64_t *hbm_bytes, char *arch, int arch_len);
/* Name of the partition-scan kernel the last qk_scan / qk_search on this context launched ("k_scan", "k_scan (query-sharing)",
 * "k_scan_rl", "k_scan_rl (mixed)", "k_search_small", "k_dense"; "" before the first call): what a harness labels its kernel timings with. */
QK_API int qk_ctx_last_scan_kernel(qk_ctx *ctx, char *name, int name_len);

/* ---- partition store ---------------------------------------------------------------------------
 * Replaces faiss::DynamicInvertedLists / IndexPartition as the thing the scan reads
 * (dynamic_inverted_list.h:25-33, index_partition.h:19-32, accessors dynamic_inverted_list.cpp:68-90).
 * Observable behaviour kept: append order, swap-with-last remove (index_partition.cpp:79-102).      */
/* A store belongs to the context it was created with (mutations run on that context's stream), but it may be SEARCHED through
 * any context of the same device -- several at once, each on its own stream -- as long as nobody mutates it meanwhile
 * (bench.py's `batches_in_flight` measurement does that: two contexts, one index). */
QK_API int qk_store_create(qk_ctx *ctx, int d, qk_store **out);                 /* DynamicInvertedLists(0, d*4) */
QK_API int qk_store_destroy(qk_store *s);
QK_API int qk_store_reset(qk_store *s);                                         /* reset() :300-304 */
QK_API int qk_store_add_list(qk_store *s, int64_t list_no);                     /* add_list :262-270 */
QK_API int qk_store_remove_list(qk_store *s, int64_t list_no);                  /* remove_list :251-260 */
/* add_entries :152-173 -> IndexPartition::append (index_partition.cpp:52-59).  vecs [n][d] row-major f32. */
QK_API int qk_store_add_entries(qk_store *s, int64_t list_no, int64_t n, const int64_t *ids, const float *vecs, int mem);
/* Batched form of the add loop of PartitionManager::add (partition_manager.cpp:236-258): vector i is appended to list
 * assign[i]; the append order inside a list is the input order.  ids/vecs/assign all live in `mem`. */
QK_API int qk_store_add_batch(qk_store *s, int64_t n, const int64_t *ids, const float *vecs, const int64_t *assign, int mem);
/* Bulk form of init_partitions (partition_manager.cpp:33-121): lists 0..nlist-1 created and filled from a CSR
 * arena (vecs [offsets[nlist]][d], ids, offsets [nlist+1] on the HOST always; vecs/ids in `mem`). */
QK_API int qk_store_build_csr(qk_store *s, int64_t nlist, const int64_t *offsets_host, const int64_t *ids,
                              const float *vecs, int mem);
/* remove_vectors :137-149: remove every id in `ids` from every list, swap-with-last per removal.
 * n_removed (may be NULL) receives the number of rows removed. */
QK_API int qk_store_remove_ids(qk_store *s, int64_t n, const int64_t *ids_host, int64_t *n_removed);
QK_API int qk_store_list_size(qk_store *s, int64_t list_no, int64_t *out);      /* list_size :68-74 */
/* PartitionManager::get_partition_sizes(Tensor) (partition_manager.cpp:296-306): the sizes of n lists in one call (host arrays);
 * an absent list is QK_ERR_NOT_FOUND like list_size.  The maintenance policy asks for every partition's size on every call. */
QK_API int qk_store_list_sizes(qk_store *s, const int64_t *list_nos, int64_t n, int64_t *out);
QK_API int64_t qk_store_ntotal(qk_store *s);                                    /* ntotal :60-66 */
QK_API int64_t qk_store_nlist(qk_store *s);
QK_API int qk_store_d(qk_store *s);
/* list numbers currently present, ascending; out may be NULL to query the count (return value via *n). */
QK_API int qk_store_list_ids(qk_store *s, int64_t *out_host, int64_t *n);
/* get_codes / get_ids :76-90 as a copy-out: rows in partition order, row-major [n][d]. */
QK_API int qk_store_get_list(qk_store *s, int64_t list_no, float *vecs_out, int64_t *ids_out, int mem);
/* The same for n lists at once, rows (and ids) laid one list after the other in list_nos order -- the caller sizes the buffers from
 * qk_store_list_sizes.  PartitionManager::select_partitions (partition_manager.cpp:344-390) / the rejection rule of the maintenance
 * policy (maintenance_policies.cpp:79-101), which read hundreds of lists per call. */
QK_API int qk_store_get_lists(qk_store *s, const int64_t *list_nos, int64_t n, float *vecs_out, int64_t *ids_out, int mem);
/* get_vector_for_id :280-293 (first match in ascending list order); *found = 0 if absent. */
QK_API int qk_store_get_vector(qk_store *s, int64_t id, float *vec_out_host, int *found);
/* PartitionManager::get(ids) (partition_manager.cpp:264-283): n vectors by id in ONE call -- found[i] = 0 and row i undefined for an
 * id the store does not hold.  (The maintenance policy reads hundreds of centroids of the parent per call.) */
QK_API int qk_store_get_vectors(qk_store *s, const int64_t *ids_host, int64_t n, float *vecs_out_host, int *found);
/* What the store's mutations have cost so far beyond the rows they were asked to write (no reference counterpart: IndexPartition
 * reallocs one partition at a time, index_partition.cpp:247-255): out[0] arena re-allocations (new arena, copy of everything, free),
 * [1] arena compactions, [2] list relocations (a list outgrew its extent), [3] rows copied by [0]-[2], [4] rebuilds of the row-major
 * copy of a parent's centroids, [5] uploads of the partition table, [6] rebuilds of the id -> list index (lazy: the first remove /
 * get after a bulk build walks every id), [7] re-allocations of the scratch buffers of the store's CONTEXT (hipFree + hipMalloc
 * behind a synchronisation).  A harness takes the difference around an operation
 * to attribute a slow add / remove / maintenance step. */
/* Make pending changes visible to searches NOW: a store that was modified uploads its list table (and, a one-list store, rebuilds
 * the row-major copy of its rows) at the next search -- two or three stream synchronisations and a copy, ~0.2 ms, inside a query.
 * A caller that has just finished a batch of modifications (add / remove / maintenance) calls this so that the queries after it do
 * not pay.  No reference counterpart (its lists are host vectors). */
QK_API int qk_store_publish(qk_store *s);
QK_API int qk_store_counters(qk_store *s, int64_t *out, int n);
/* bytes of HBM held by the arena (vectors+norms+ids) and, once built, its fp16 shadow, for capacity planning */
QK_API int64_t qk_store_device_bytes(qk_store *s);
/* The fp16 shadow of the store (qk_ctx_set_shadow): *valid = 1 when a shadow mirrors the store as it is now, *bytes = HBM it holds,
 * *builds = conversions that left a valid shadow so far.  Any pointer may be NULL.  A store that holds a non-finite value or one
 * beyond the fp16 range (65504) has no shadow. */
QK_API int qk_store_shadow_info(qk_store *s, int *valid, int64_t *bytes, int64_t *builds);
/* frees the shadow (qk_store_destroy and qk_store_reset do so too); the next eligible searches build it again */
QK_API int qk_store_shadow_drop(qk_store *s);

/* ---- search ------------------------------------------------------------------------------------ */
/* Coarse step = parent_->search(x, {k = min(nprobe, nlist), batched_scan = true})
 * (query_coordinator.cpp:628-644 -> batched_scan_list over the centroid list, list_scanning.h:313-366).
 * `parent` is the store of the parent (flat) index: its lists hold the centroids, ids = partition ids.
 * out_pids [Q][kk], out_dist [Q][kk] (may be NULL), kk = min(nprobe, parent ntotal); rows padded with -1. */
QK_API int qk_coarse(qk_ctx *ctx, qk_store *parent, const float *x, int64_t Q, int nprobe, int metric, int64_t *out_pids,
                     float *out_dist, int mem);

/* QueryCoordinator::scan_partitions (query_coordinator.cpp:659-673; serial_scan :471-611 and
 * batched_serial_scan :675-799 give the same result here).  x [Q][d]; pids [Q][P] partition numbers to scan
 * per query, -1 = skip (:540); out_ids/out_dist [Q][k].  timing may be NULL. */
QK_API int qk_scan(qk_ctx *ctx, qk_store *s, const float *x, int64_t Q, const int64_t *pids, int P, int k, int metric,
                   int64_t *out_ids, float *out_dist, int mem, qk_timing *timing);

/* QueryCoordinator::search (query_coordinator.cpp:612-657) at fixed nprobe: coarse + scan in one enqueue,
 * no host round trip between the two.  parent == NULL: flat index, every list of `s` is scanned (:624-626). */
QK_API int qk_search(qk_ctx *ctx, qk_store *parent, qk_store *s, const float *x, int64_t Q, int nprobe, int k, int metric,
                     int64_t *out_ids, float *out_dist, int mem, qk_timing *timing);

/* qk_search that also hands out WHICH lists every query scanned -- out_probed [Q][min(nprobe, parent lists)] list numbers in rank
 * order (host or device like the other buffers) -- in the same enqueue: what QuakeIndex::search passes to
 * MaintenancePolicy::record_query_hits (maintenance_policies.cpp:179-182; the reference has the list on the host anyway).  The
 * nearest-centroid step writes the caller's buffer and the scan reads it: no second call, no copy. */
QK_API int qk_search_tracked(qk_ctx *ctx, qk_store *parent, qk_store *s, const float *x, int64_t Q, int nprobe, int k, int metric,
                             int64_t *out_ids, float *out_dist, int64_t *out_probed, int mem, qk_timing *timing);

/* ---- filtered search ---------------------------------------------------------------------------
 * No reference counterpart (its SearchParams ends at aps_flush_period_us): search restricted to a set of ids.
 * A filter is a set of ids S and a mode -- QK_FILTER_ALLOW: a row is a candidate iff its id is in S; QK_FILTER_DENY: iff it is
 * not.  The coarse step is not filtered: a filtered search probes the lists the unfiltered one probes and returns the k best
 * CANDIDATE rows of those lists under the total order (key, id), with the same distance bits -- it equals the unfiltered search
 * over a store that holds the same lists without the other rows.  Fewer than k candidates in the probed lists: padded like any
 * short result (id -1, +inf / -inf).  Ids of S the store does not hold are ignored; every copy of an id stored twice follows the
 * filter; rows added after the filter was made follow the mode (absent from an allow-set: not a candidate).
 *
 * A filter belongs to ONE store (another store's: QK_ERR_INVALID) but is defined by ids, not rows: inside, it keeps S sorted on
 * the device and a row mask -- one bit per arena row, cap_rows / 8 bytes -- stamped with the store's version.  Whatever moves rows
 * (add, remove, list relocation, compaction, refinement, maintenance) changes that version, and the next filtered call re-derives
 * the mask (k_filter_build: one pass over the stored ids, a binary search each) on ITS context's stream, in front of its scan.
 * Ordering: a mask is read by the scans enqueued behind its build on that stream; a filtered call on another context waits for
 * the build by event.  A caller that rebinds a context to streams of its own (qk_ctx_set_stream) must order a stream behind the
 * one that ran the last filtered call after a store change before it issues filtered calls on it -- and, as for every search,
 * nobody mutates the store while searches are in flight.
 * The filter holds everything it needs: it may be destroyed after its store (it can no longer be used then).
 *
 * Limits, all QK_ERR_UNSUPPORTED: k > QK_MAX_K (no wide-k path), and there is no filtered form of qk_search_aps (recall target:
 * its recall model counts volume, not candidate rows) nor of the device group (qk_group_search).  With a filter the scan is the
 * 16 x 16 tile form (k_scan_filt, or k_scan_wide_filt for wide rows) without bound seeding -- a bound from a row that is not a
 * candidate would drop rows that are -- whatever form the unfiltered call of the same shape takes; tiles without a candidate
 * are not read.  A flat index (parent == NULL) takes the same scan, not the dense forms. */
typedef struct qk_filter qk_filter;
#define QK_FILTER_ALLOW 0
#define QK_FILTER_DENY 1
/* ids [n] in `mem` (any order, duplicates allowed; n == 0: the empty set).  Builds the first mask on the store's context. */
QK_API int qk_filter_create(qk_store *s, const int64_t *ids, int64_t n, int mode, int mem, qk_filter **out);
QK_API int qk_filter_destroy(qk_filter *f);
/* Any pointer may be NULL.  n_ids: distinct ids of S; rows_allowed: candidate rows of the store as of the last mask build
 * (synchronises with that build); store_version: the stamp of the mask; rebuilds: mask builds after the first, one per filtered
 * call that found the store changed; device_bytes: HBM held by the filter (not part of qk_store_device_bytes). */
QK_API int qk_filter_info(qk_filter *f, int64_t *n_ids, int64_t *rows_allowed, uint64_t *store_version, int64_t *rebuilds,
                          int64_t *device_bytes);
/* qk_search / qk_search_tracked / qk_scan restricted to the filter's candidates; timing is filled as for the unfiltered calls
 * (partitions_scanned = lists probed, scan_bytes = the algorithmic bytes of those lists, not what the mask left to read).
 * qk_ctx_last_scan_kernel names "k_scan (filtered)" / "k_scan_wide (filtered)" afterwards. */
QK_API int qk_search_filtered(qk_ctx *ctx, qk_store *parent, qk_store *s, const float *x, int64_t Q, int nprobe, int k, int metric,
                              qk_filter *f, int64_t *out_ids, float *out_dist, int mem, qk_timing *timing);
QK_API int qk_search_filtered_tracked(qk_ctx *ctx, qk_store *parent, qk_store *s, const float *x, int64_t Q, int nprobe, int k,
                                      int metric, qk_filter *f, int64_t *out_ids, float *out_dist, int64_t *out_probed, int mem,
                                      qk_timing *timing);
QK_API int qk_scan_filtered(qk_ctx *ctx, qk_store *s, const float *x, int64_t Q, const int64_t *pids, int P, int k, int metric,
                            qk_filter *f, int64_t *out_ids, float *out_dist, int mem, qk_timing *timing);

/* One filter per QUERY of a batch (a server has one filter per user or tenant; its batches mix them): query i is answered under
 * filters[qfilter[i]].  Row i of the result equals row 0 of the single-filter call above made with query i alone and that
 * filter -- ids and distance bits -- so everything said there holds per query: the coarse step is not filtered, a short row is
 * padded, ids that are not stored are ignored, a filter follows its ids through add / remove / refine / maintenance, and no bound
 * is learned from a row that was not tested against that query's filter.
 *   filters [F]  HOST array of handles of this store (1 <= F <= QK_MAX_BATCH_FILTERS), each brought up to date like the single one;
 *   qfilter [Q]  int32 in `mem` like the other buffers.  There is no "unfiltered" code: a query that should see every row names a
 *                QK_FILTER_DENY filter of the empty set.
 * QK_ERR_INVALID: F < 1, a null handle, a filter of another store or device, a host qfilter value outside [0, F).  A DEVICE
 * qfilter is not read by the host: a value outside [0, F) gives that query an all-padding row (the kernel checks the range before
 * it indexes the table).  QK_ERR_UNSUPPORTED: k > QK_MAX_K, F > QK_MAX_BATCH_FILTERS.
 * Inside: the kernels k_scan_filtq / k_scan_wide_filtq test every row against the mask word of its lane's own query, and read the
 * tiles that hold a candidate of at least one of the F filters -- the OR of the masks (k_filter_union), kept on the context
 * together with the device table of the mask pointers and reused while the same filters come in the same order and neither they
 * nor the store changed.  qk_ctx_last_scan_kernel names "k_scan (filtered, per query)" / "k_scan_wide (filtered, per query)". */
#define QK_MAX_BATCH_FILTERS 4096
QK_API int qk_search_filtered_batch(qk_ctx *ctx, qk_store *parent, qk_store *s, const float *x, int64_t Q, int nprobe, int k,
                                    int metric, qk_filter *const *filters, int F, const int32_t *qfilter, int64_t *out_ids,
                                    float *out_dist, int mem, qk_timing *timing);
QK_API int qk_search_filtered_batch_tracked(qk_ctx *ctx, qk_store *parent, qk_store *s, const float *x, int64_t Q, int nprobe, int k,
                                            int metric, qk_filter *const *filters, int F, const int32_t *qfilter, int64_t *out_ids,
                                            float *out_dist, int64_t *out_probed, int mem, qk_timing *timing);
QK_API int qk_scan_filtered_batch(qk_ctx *ctx, qk_store *s, const float *x, int64_t Q, const int64_t *pids, int P, int k, int metric,
                                  qk_filter *const *filters, int F, const int32_t *qfilter, int64_t *out_ids, float *out_dist,
                                  int mem, qk_timing *timing);

/* Adaptive probing: probe until min_candidates candidates.  A filtered search probes exactly nprobe lists, whatever its filter
 * leaves in them; under a selective filter that is a short or poor row, and raising nprobe for the whole batch makes the least
 * selective query pay for the most selective one.  Here every query probes the shortest prefix of its ranked lists that holds
 * enough candidates of ITS filter.  The definition, per query q under its filter:
 *   M = min(max_nprobe, lists of the parent), n0 = min(nprobe, M);
 *   r_1 .. r_M: the lists the unfiltered coarse step (qk_coarse) ranks for q at nprobe = M; a -1 padding entry (a NaN centroid,
 *     fewer than M lists) is a list of 0 rows;
 *   c(p): the rows of list p that are candidates of q's filter.  Only the mask counts -- a property of the store and the filter,
 *     not of the query: a row whose distance to q is NaN still counts;
 *   nprobed(q): the smallest t in [n0, M] with c(r_1) + .. + c(r_t) >= min_candidates; M if there is none;
 *   the result row of q is, bit for bit, the row qk_scan_filtered returns for q alone with pids = r_1 .. r_nprobed(q): the same
 *     ids and distance bits, padded if those lists still hold fewer than k candidates.
 * With max_nprobe == nprobe the call equals qk_search_filtered / qk_search_filtered_batch, bit for bit.
 *   filters [F], qfilter [Q]: as for qk_search_filtered_batch; F == 1 && qfilter == NULL: filters[0] for every query.  A DEVICE
 *     qfilter value outside [0, F): nprobed = 0, an all -1 probed row, an all-padding result (range checked before any table is
 *     indexed); a HOST one: QK_ERR_INVALID.
 *   out_nprobed int32 [Q], may be NULL; out_probed int64 [Q][M], may be NULL: r_1 .. r_nprobed(q), then -1 (what the policy's hit
 *     tracker takes, like qk_search_tracked's buffer).  Both in `mem`.
 * QK_ERR_INVALID: min_candidates < 1, max_nprobe < nprobe, nprobe < 1, parent == NULL (a flat index has nothing to adapt), and
 * what qk_search_filtered_batch refuses.  QK_ERR_UNSUPPORTED: k > QK_MAX_K, M > QK_MAX_NPROBE, F > QK_MAX_BATCH_FILTERS.
 * timing is filled as for qk_search_filtered; partitions_scanned counts the pairs actually scanned (present, non-empty lists
 * of the prefixes), not Q * M; the cut itself lies between coarse_ms and group_ms and is part of total_ms only.
 * Inside, one enqueue, no host wait and no atomics between the coarse step and the scan: the coarse step at M; per filter an
 * int32 count per list number (k_filter_list_counts: a wave per list, the popcount of the mask words of its extent), kept on
 * the filter, dropped by every mask build and derived again by the next ADAPTIVE call -- the other filtered calls neither
 * allocate nor launch anything for it, qk_filter_info's device_bytes includes it once it exists; k_probe_trim, a wave per query:
 * a prefix sum of the counts along the ranked row, -1 written over the tail; then the filtered scan of the calls above at
 * P = M, which skips -1.  The per-query form reads the count pointer of filters[qfilter[q]] from a device table kept next to
 * the mask table under the same rule.
 * Out of scope: range search, grouped search, the device group and the sharded index probe a fixed nprobe under a filter. */
QK_API int qk_search_filtered_adaptive(qk_ctx *ctx, qk_store *parent, qk_store *s, const float *x, int64_t Q, int nprobe,
                                       int max_nprobe, int64_t min_candidates, int k, int metric, qk_filter *const *filters, int F,
                                       const int32_t *qfilter, int64_t *out_ids, float *out_dist, int32_t *out_nprobed,
                                       int64_t *out_probed, int mem, qk_timing *timing);

/* Exact filtered search: compact the filter's candidates, search them flat.  A probed filtered search returns the best candidates
 * OF THE PROBED LISTS; under a selective filter those hold almost none of the filter's rows.  The right answer for such a filter
 * is the exact top-k of its candidates, and it is cheap: the candidates are gathered once into a private one-list store kept on
 * the filter, and every call is the flat search of that store -- no parent, no nprobe, cost by candidates, not by lists.
 *   Result: row q is bit for bit -- ids and distance bits, padding included -- what qk_search(ctx, NULL, c, ..) returns over a
 *     one-list store c that holds exactly the candidate rows; that is qk_search_filtered with every list probed.  (A row's key
 *     does not depend on its neighbours and results are ordered by (key, id): where the rows sit cannot show.)
 *   1 <= k <= 8192, whatever the flat search accepts (QK_ERR_UNSUPPORTED beyond): the filtered route beyond QK_MAX_K.
 *   qk_ctx_set_squared_l2 is honoured as in qk_search; NaN / Inf / overflow follow the flat search's contract (see the top).
 *   No candidates, fewer than k, an empty store: padded rows (-1, +inf / -inf).
 *   max_rows > 0: a filter with more candidates is refused with QK_ERR_UNSUPPORTED before anything is allocated or enqueued for
 *     the candidate store -- the caller bounds its memory, rows x (dpad * 4 + 12) bytes (never less than the 1024 rows every
 *     arena starts with; the prefiltered dense forms keep a row-major copy of a list of up to 128 MiB next to it, as they do
 *     for every flat index: qk_filter_exact_info counts it); max_rows == 0: no bound.
 *   QK_ERR_INVALID: another store's filter, a filter on another device, max_rows < 0.
 *   timing is filled as the flat search fills it: scan_bytes = the candidate rows' bytes, coarse_ms = 0; a mask build and the
 *     gather lie in front of the scan's events and are part of total_ms only, like the cut of an adaptive call.  qk_ctx_last_scan_kernel names the
 *     dense kernel that ran.
 * The candidate store follows the life cycle of the adaptive counts: derived from the row mask by the first EXACT call behind a
 * mask build, on that call's stream behind the mask; a call on another context waits for it by event; every mask build drops it
 * (the memory is kept, and grown geometrically); qk_filter_destroy frees it; the other filtered calls neither allocate nor launch
 * anything for it; qk_filter_info's device_bytes includes it once it exists.  It reads only the mask, so id sets, deny sets and
 * predicates are served alike.  Inside: k_filter_block_counts (candidates per 64 mask words), k_filter_block_scan (their
 * exclusive prefix sum, int64, one workgroup) and k_filter_gather (a wave per destination tile: destination row j is the j-th
 * candidate in ascending arena-row order; vectors, norm bits and ids are copied, the tail of the last tile is written with what a
 * fresh arena holds) -- no atomics, no device library, and no row or id travels to the host: the only host read is the candidate
 * count, 8 bytes per mask build.
 * qk_filter_candidate_rows: the candidates of f in s NOW -- brings the mask up to date on ctx's stream and waits for it only if
 * the count of this build has not been read yet.  qk_filter_exact_info (any pointer may be NULL): rows = rows of the candidate
 * store as of its last derivation, builds = derivations so far -- one per exact call that found the mask newer than the store,
 * none otherwise --, device_bytes = what the candidate store holds (0 before the first exact call).
 * Out of scope: per-query filters, range / grouped / paged search over the candidate store, the device group. */
QK_API int qk_filter_candidate_rows(qk_ctx *ctx, qk_store *s, qk_filter *f, int64_t *rows);
QK_API int qk_search_filtered_exact(qk_ctx *ctx, qk_store *s, const float *x, int64_t Q, int k, int metric, qk_filter *f,
                                    int64_t max_rows, int64_t *out_ids, float *out_dist, int mem, qk_timing *timing);
QK_API int qk_filter_exact_info(qk_filter *f, int64_t *rows, int64_t *builds, int64_t *device_bytes);

/* Exact filtered search, one filter per query: a candidate pool, one list per filter.  A batch that mixes tenants is answered
 * exactly in one enqueue: query i gets the exact top-k of the candidates of filters[qfilter[i]].
 *   Result: row i is bit for bit -- ids, distance bits, padding -- row 0 of qk_search_filtered_exact(query i alone,
 *     filters[qfilter[i]]).  1 <= k <= 8192, d up to QK_MAX_D, qk_ctx_set_squared_l2 and the NaN / Inf / overflow / signed zero
 *     contract as there.
 *   filters [F], qfilter [Q]: as in qk_search_filtered_batch -- a host array of 1 .. QK_MAX_BATCH_FILTERS handles of s (the same
 *     handle may appear twice: one slot); qfilter in `mem`; a host value outside [0, F) is QK_ERR_INVALID, a device value outside
 *     gives that query an all-padding row (checked on the device before any table is indexed).
 *   The POOL is a private store owned by s: made by the first call, freed by qk_store_exact_pool_drop and qk_store_destroy.  A
 *     filter that was ADMITTED holds a slot = a list of the pool with exactly its candidate rows (vectors, norm bits, ids) in
 *     ascending arena-row order: the rows and the order of the private candidate store of qk_search_filtered_exact, which stays as
 *     it is -- a filter used by both calls holds two copies.  A slot is valid while the filter's mask is current: every mask
 *     build gives it back, the next call that names the filter gathers it again, qk_filter_destroy frees it, a call on another
 *     context waits for an admission by event, and no other call allocates or launches anything for the pool.  Slots persist
 *     across calls with different filter lists: after [A, B], a call with [B, C] gathers C only.  Every filter of `filters` is
 *     admitted, whether a query names it or not (also with Q == 0).
 *   Admission of the M filters of a call without a valid slot is one launch series (per 64 MiB of block offsets: 400 filters at
 *     10M rows): k_pool_block_counts, k_pool_block_scan, k_pool_gather -- the three kernels of the single-filter call indexed by
 *     a device table of (mask, candidates, destination extent, first destination tile); the gather finds its filter from its
 *     destination tile.  No atomics, no device library, int64 offsets; no row or id travels to the host.  The candidate counts
 *     nobody has read since the mask build come back in ONE copy behind ONE wait; the pool's list table is written in stream
 *     order from host memory without a wait.  A call whose filters are all resident waits for nothing and uploads no table.
 *   max_rows > 0: if a filter of the call has more candidates the call fails with QK_ERR_UNSUPPORTED, naming the first such index,
 *     before anything is allocated or enqueued for the pool.
 *   pool_rows > 0 bounds the rows the pool holds after the call, counted as the sum over resident slots of the candidates rounded
 *     up to 16: slots of filters NOT named by this call are evicted, least recently named first (ties: lowest slot number); if the
 *     filters of the call alone need more: QK_ERR_UNSUPPORTED, the pool unchanged.  The pool arena then never exceeds
 *     max(2 pool_rows, 1024) rows; pool_rows == 0: no bound.  Extents of evicted, rebuilt and destroyed filters are handed out
 *     again (first fit); when nothing fits, the live extents are packed into a fresh arena (both exist during the copy).
 *   QK_ERR_INVALID: a null handle, another store's or device's filter, max_rows < 0, pool_rows < 0, k < 1.
 *   Inside: k_pool_pids turns a device qfilter into pids [Q][1] of pool list numbers (-1 out of range; a host qfilter is mapped
 *     on the host), then the unfiltered partition scan of the pool runs with P = 1 (the wide-k pipeline beyond QK_MAX_K):
 *     qk_ctx_last_scan_kernel names an unfiltered form.  timing as qk_scan fills it; mask builds and the admission lie in front
 *     of the scan's events and are part of total_ms only.
 * qk_store_exact_pool_info (any pointer may be NULL; all 0 before the first call and after a drop): slots = resident slots,
 * rows = the measure pool_rows bounds, cap_rows = the pool arena's capacity, builds = slots gathered so far (one per filter
 * admitted, not per admission), evictions = slots evicted by a budget, device_bytes = arena + list table.
 * qk_store_exact_pool_drop frees the pool; filters stay valid and are admitted again on demand.
 * Out of scope: the device group, range / grouped / paged search over the pool, the recall-target walk. */
QK_API int qk_search_filtered_exact_batch(qk_ctx *ctx, qk_store *s, const float *x, int64_t Q, int k, int metric,
                                          qk_filter *const *filters, int F, const int32_t *qfilter, int64_t max_rows,
                                          int64_t pool_rows, int64_t *out_ids, float *out_dist, int mem, qk_timing *timing);
QK_API int qk_store_exact_pool_info(qk_store *s, int64_t *slots, int64_t *rows, int64_t *cap_rows, int64_t *builds,
                                    int64_t *evictions, int64_t *device_bytes);
QK_API int qk_store_exact_pool_drop(qk_store *s);

/* ---- range search --------------------------------------------------------------------------------
 * No reference counterpart (every search of the reference is a top-k): all rows of the probed lists within a radius of each query.
 * Lists: qk_range_search probes what the unfiltered qk_search probes -- the same min(nprobe, parent lists) lists in the same rank
 * order, every list with parent == NULL; qk_range_scan takes pids [Q][P] like qk_scan (distinct list numbers per row), where -1,
 * absent and empty lists contribute nothing (no QK_ERR_NOT_FOUND here).
 * Hits: a row of a probed list is a hit iff the float32 distance qk_search would report for it -- sqrt L2, squared L2 after
 * qk_ctx_set_squared_l2(ctx, 1), the dot product for IP -- satisfies dist <= radius (L2) / dist >= radius (IP), inclusive, in
 * float32; a NaN distance is never a hit; radius = +inf (L2) / -inf (IP) returns every probed row whose distance is not NaN; a NaN
 * radius is QK_ERR_INVALID.  The host turns the radius into one closed interval of the integer keys the scan emits (L2 with sqrt:
 * the largest float t >= 0 with sqrtf(t) <= radius, found by stepping ulps around radius * radius), so the test is exact.
 * `filter`: a qk_filter of this store or NULL; a hit must also be a candidate of the filter (brought up to date like any
 * filtered call; another store's filter: QK_ERR_INVALID).
 * Order: query q's hits are out_ids / out_dist [lims[q], lims[q+1]), lims[0] = 0; inside a query in scan order -- the probed
 * lists in rank order (the order of its pids row), the rows of a list in stored order.  Ids are the stored ids, distances the bits
 * qk_search returns for those rows.  No atomic decides a position: the result is a pure function of the store and the call.
 * Capacity: out_lims [Q + 1] is always written in full and exact, whatever cap is; ids and distances are written at positions
 * < cap only -- a prefix of the global order -- and nothing beyond min(cap, lims[Q]) is touched.  lims[Q] > cap is still QK_OK: the
 * caller compares and calls again with larger buffers.  cap == 0 with NULL out_ids / out_dist counts only (out_dist may be NULL
 * with any cap).  cap < 0 or out_lims == NULL: QK_ERR_INVALID.  Q == 0: QK_OK, lims[0] = 0.
 * Inside: the key-emission scan of the wide-k path (one launch per pass of queries, the only kernel that reads the vectors), then
 * k_range_count / k_range_qscan / k_range_offsets / k_range_write (qk_range.hip): count per slice, exclusive scans -- per query,
 * then over the queries, continued across passes on the device -- and a stable compaction.  timing: coarse_ms the coarse step, scan_ms the emission scan, merge_ms counting + compaction (of
 * the last pass when there are several), n_items the number of query passes, scan_bytes / partitions_scanned as for qk_search.
 * qk_ctx_last_scan_kernel names "k_scan (range)" / "k_scan_wide (range)".  There is no range form of qk_search_aps, of the device
 * group or of per-query filter tables. */
QK_API int qk_range_search(qk_ctx *ctx, qk_store *parent, qk_store *s, const float *x, int64_t Q, int nprobe, int metric, float radius,
                           qk_filter *filter, int64_t cap, int64_t *out_lims, int64_t *out_ids, float *out_dist, int mem,
                           qk_timing *timing);
QK_API int qk_range_scan(qk_ctx *ctx, qk_store *s, const float *x, int64_t Q, const int64_t *pids, int P, int metric, float radius,
                         qk_filter *filter, int64_t cap, int64_t *out_lims, int64_t *out_ids, float *out_dist, int mem,
                         qk_timing *timing);

/* ---- attribute filters ---------------------------------------------------------------------------
 * No reference counterpart.  A COLUMN (qk_attr) is a partial map id -> int64 that belongs to one store and lives on its device.  It
 * is keyed by id, not by row: add, remove, relocation, compaction, refinement and maintenance never touch it; removing a vector
 * leaves its values in place (an id that is not stored is never a candidate), so remove + add of an id keeps its attributes.
 * A PREDICATE filter is a qk_filter made from 1 .. QK_MAX_CLAUSES clauses {column, op, a, b} instead of an id list.  A stored row
 * is a candidate iff, for EVERY clause, its id has a value v in the clause's column and
 *   QK_OP_RANGE      a <= v <= b, signed and inclusive (a > b: the empty interval, matches nothing)
 *   QK_OP_NOT_RANGE  the complement of QK_OP_RANGE
 *   QK_OP_ANY_BITS   (v & a) != 0          QK_OP_ALL_BITS  (v & a) == a          QK_OP_NO_BITS  (v & a) == 0
 * holds.  An id without a value fails every op, NOT_RANGE and NO_BITS included (SQL's NULL); every copy of an id stored twice
 * follows its id; the order of the clauses does not matter.  At any moment the filter answers exactly like the QK_FILTER_ALLOW
 * filter over {id : every clause holds for id} -- ids, distance bits and padding -- so everything said under "filtered search"
 * holds, and it is passed to the same entry points: qk_search_filtered*, qk_scan_filtered*, the per-query table (mixed freely
 * with id-set filters), qk_range_search / qk_range_scan.  It holds no ids: creating it costs one mask build (k_filter_build_where:
 * per stored row the id, then per clause a lookup in the column and the op, stopping at the first clause that fails).
 * Liveness: the mask is stamped with the store's (uid, version, cap_rows) AND (serial, version) of every clause's column;
 * qk_attr_set / qk_attr_unset bump the column's version, and the next filtered call that uses the filter re-derives the mask once,
 * on its own stream, in front of its scan.  Column updates are enqueued on the store's context stream; a mask build on another
 * context waits for the column's last update by event.  As for store mutations, nobody updates a column while searches that use it
 * are in flight.  A filter shares ownership of its columns' device data: qk_attr_destroy while filters are alive is legal, those
 * filters keep answering with the last values.
 * Layout (never visible in a result): a direct table -- values[id] and one presence bit per id -- while max_id < 4 * n_ids + 65536,
 * else ascending (id, value) pairs looked up by binary search; re-decided on every set / unset and converted when the rule flips. */
typedef struct qk_attr qk_attr;
#define QK_OP_RANGE 0
#define QK_OP_NOT_RANGE 1
#define QK_OP_ANY_BITS 2
#define QK_OP_ALL_BITS 3
#define QK_OP_NO_BITS 4
#define QK_MAX_CLAUSES 8
#define QK_ATTR_TABLE 0
#define QK_ATTR_SORTED 1
typedef struct {
    qk_attr *attr;
    int op;
    int64_t a, b; /* b is read by the RANGE ops only */
} qk_clause;
QK_API int qk_attr_create(qk_store *s, qk_attr **out);
QK_API int qk_attr_destroy(qk_attr *a);
/* upsert values[i] for ids[i] (an id given twice: the last value wins); a negative id: QK_ERR_INVALID, nothing is changed */
QK_API int qk_attr_set(qk_attr *a, const int64_t *ids, const int64_t *values, int64_t n, int mem);
/* the ids lose their values; ids that have none are ignored */
QK_API int qk_attr_unset(qk_attr *a, const int64_t *ids, int64_t n, int mem);
/* values_out_host[i], found[i] (0 / 1) for ids_host[i], read back from the device (synchronises; either output may be NULL) */
QK_API int qk_attr_get(qk_attr *a, const int64_t *ids_host, int64_t n, int64_t *values_out_host, int *found);
/* n_ids: ids that have a value; version: bumped by every set / unset; layout: QK_ATTR_TABLE / QK_ATTR_SORTED; device_bytes: HBM
 * held by the column (not part of qk_store_device_bytes) */
QK_API int qk_attr_info(qk_attr *a, int64_t *n_ids, uint64_t *version, int *layout, int64_t *device_bytes);
/* QK_ERR_INVALID: n_clauses < 1, a null column, a column of another store, an unknown op; QK_ERR_UNSUPPORTED: n_clauses >
 * QK_MAX_CLAUSES.  qk_filter_info of the result: n_ids = -1, device_bytes = the mask only. */
QK_API int qk_filter_create_where(qk_store *s, const qk_clause *clauses, int n_clauses, qk_filter **out);
/* An EXPRESSION filter: an OR of 1 .. QK_MAX_TERMS conjunctions (terms) over the five ops above and two value-set ops
 *   QK_OP_IN_SET      the id has a value and it is one of the set's
 *   QK_OP_NOT_IN_SET  the id has a value and it is none of the set's
 * `clauses` holds the terms one after the other, term t has term_sizes[t] >= 1 clauses.  A stored row is a candidate iff, for SOME
 * term, EVERY clause of that term holds for its id; an id without a value in a clause's column fails that clause, NOT_IN_SET
 * included.  set / n_set: a HOST array read by the two set ops only -- any order, duplicates allowed; the empty set is legal
 * (IN_SET of it matches nothing, NOT_IN_SET of it every id that has a value); a / b are read by the other five.  At creation the
 * sets are sorted, de-duplicated and uploaded once into one buffer the filter owns.  Neither term order nor clause order matters.
 * Otherwise a predicate filter in every respect: it answers like the QK_FILTER_ALLOW filter over {id : some term holds}, is passed
 * to every entry point that takes a filter, is stamped with the store's (uid, version, cap_rows) and the (serial, version) of the
 * column of every clause of every term and re-derived by the next filtered call when a stamp moved (k_filter_build_expr: the
 * sibling of k_filter_build_where -- per row `accepted by an earlier term` and `alive in this term`, a term skipped by a wave none
 * of whose rows is undecided, set membership by the sorted layout's branch-free binary search), shares ownership of its columns.
 * QK_ERR_INVALID: n_terms < 1, a term_sizes[t] < 1, a null column, a column of another store, an op outside 0 .. 6, n_set < 0,
 * n_set > 0 with a null set; QK_ERR_UNSUPPORTED: n_terms > QK_MAX_TERMS, more than QK_MAX_EXPR_CLAUSES clauses in total, n_set >
 * QK_MAX_SET_VALUES.  qk_filter_info of the result: n_ids = -1, device_bytes = the mask + the set buffer (the clause table travels
 * in the kernel arguments).  Footprint: every set clause keeps its own sorted copy -- a set named by several clauses is held once
 * per clause -- so the worst case, 32 set clauses of 2^20 values, is 256 MB of host temporaries during the call and 256 MB of
 * device buffer for the filter's life; QK_ERR_OOM when either is not to be had.  qk_filter_create_where is unchanged: its own
 * kernel, QK_MAX_CLAUSES, ops 0 .. 4. */
#define QK_OP_IN_SET 5
#define QK_OP_NOT_IN_SET 6
#define QK_MAX_TERMS 8
#define QK_MAX_EXPR_CLAUSES 32      /* over all terms */
#define QK_MAX_SET_VALUES (1 << 20) /* per clause, as given */
typedef struct {
    qk_attr *attr;
    int op;
    int64_t a, b;
    const int64_t *set; /* HOST array, read by the two set ops only; any order, duplicates allowed */
    int64_t n_set;
} qk_expr_clause;
QK_API int qk_filter_create_expr(qk_store *s, const qk_expr_clause *clauses, const int *term_sizes, int n_terms, qk_filter **out);

/* ---- grouped search -------------------------------------------------------------------------------
 * No reference counterpart.  The k best GROUPS of a column per query, every group represented by its best row: results that are
 * distinct by an attribute (the 10 best documents of a store of chunks, each by its best chunk), exact -- what oversampling
 * qk_search and de-duplicating on the host cannot give.
 * Lists: qk_search_grouped probes what the unfiltered qk_search probes (every list with parent == NULL); qk_scan_grouped takes
 * pids [Q][P] like qk_range_scan: -1, absent and empty lists contribute nothing.
 * Candidates of a query: the rows of its probed lists whose id has a value in `group_by` (an id without a value is never a
 * candidate, as for predicate filters), whose key is not that of a NaN value (0xFFFFFFFF), and which `filter` -- a qk_filter of
 * this store or NULL -- allows.  The representative of a value g is the candidate with that value that is smallest under the
 * library's total order (key, id); the result is the k smallest representatives under (key, id): out_ids / out_dist [Q][k] with the
 * distance bits qk_search reports for those rows, out_groups [Q][k] (may be NULL) the value of each entry.  Fewer than k groups:
 * padded like qk_search (id -1, distance +inf / -inf), out_groups 0 there.  With every id in a group of its own the result is
 * qk_search's bit for bit; with a filter a group is represented by its best ALLOWED row; +-inf are ordinary values; -0 and +0
 * have one key and tie on the id.  Ids are unique within a store and, having values, non-negative.
 * Liveness: the values are looked up when the call runs.  The column keeps its value of every arena row of the store, stamped with
 * the store's (version, cap_rows) and its own version; a call that finds a stamp moved -- add, remove, anything that moves rows,
 * qk_attr_set / qk_attr_unset -- re-derives them once (k_grouped_rowvals: one lookup per stored row) on its stream in front of its
 * scan, otherwise nothing is done (qk_attr_group_info counts the derivations).  Ordering across contexts and streams as for filters.
 * 1 <= k <= 8192; every k goes through key emission (there is no fused form for small k): the emission scan of the wide-k path,
 * then per pass of queries an open-addressing table per query -- k_grouped_claim / k_grouped_minid / k_grouped_rewrite
 * (qk_grouped.hip): atomicCAS claims a value's slot, atomicMin folds keys, then ids; every key that is not its group's (min key,
 * min id) becomes 0xFFFFFFFF -- then the exact selection of the wide-k path and k_grouped_values.  No kernel waits or spins; the
 * result is a pure function of the store, the column and the call.
 * Workspace: per query of a pass 8 bytes per key it has room for (P lists of the store's largest size: per_query_ub) and 20 per
 * table slot, T + 1 slots with T = the power of two >= max(16, 2 * min(per_query_ub, ids that have a value)).  Queries per pass =
 * min(the wide-k rule: 2^29 / per_query_ub, QK_GROUPED_PASS_BYTES / that many bytes), at least 1; tables are cleared on the stream,
 * nothing synchronises between passes.  QK_ERR_INVALID: group_by == NULL, a column or filter of another store, k < 1;
 * QK_ERR_UNSUPPORTED: k > 8192, a single query whose bytes exceed QK_GROUPED_PASS_BYTES (or whose keys exceed 2^30).
 * timing: coarse_ms / group_ms / scan_ms / merge_ms / total_ms as for the wide-k path (merge_ms: reduction + selection of the last
 * pass), n_items = the number of query passes; no list statistics.  qk_ctx_last_scan_kernel names "k_scan (grouped)" /
 * "k_scan_wide (grouped)".  There is no grouped form of per-query filters, of qk_search_aps or of the device group. */
#define QK_GROUPED_PASS_BYTES ((int64_t)1 << 31)
QK_API int qk_search_grouped(qk_ctx *ctx, qk_store *parent, qk_store *s, const float *x, int64_t Q, int nprobe, int k, int metric,
                             qk_attr *group_by, qk_filter *filter, int64_t *out_ids, float *out_dist, int64_t *out_groups, int mem,
                             qk_timing *timing);
QK_API int qk_scan_grouped(qk_ctx *ctx, qk_store *s, const float *x, int64_t Q, const int64_t *pids, int P, int k, int metric,
                           qk_attr *group_by, qk_filter *filter, int64_t *out_ids, float *out_dist, int64_t *out_groups, int mem,
                           qk_timing *timing);
/* Grouped search with members: the group_size = m best rows of each of the k best groups, 1 <= m <= QK_MAX_GROUP_SIZE.  The
 * argument lists of qk_search_grouped / qk_scan_grouped with group_size behind k; those two are these with m = 1, launch for launch.
 * Candidates, the total order (key, id), the ranking of the groups by their best candidate and the choice of the k best groups are
 * unchanged.  Of each chosen group the call returns its min(m, candidates of that group for this query) best candidates under
 * (key, id), ascending: out_ids [Q][k][m], out_dist [Q][k][m] (may be NULL; the bits qk_search reports), out_groups [Q][k] (may be
 * NULL).  Members a group does not have are padding (id -1, distance +inf / -inf), every member of a padded group slot is padding,
 * out_groups is 0 where member 0 is.  Equal keys are ordered by id and both rows appear where there is room; ids are compared as
 * 64-bit words, nothing is packed.  Member 0 of every group, and out_groups, are the one-row call's result bit for bit.
 * m > 1: k_grouped_rewrite leaves the emitted keys alone and fills a second key array for the selection.  Behind the selection
 * k_grouped_mark finds the slot of every selected row's value again (the hash and the bounded walk of k_grouped_claim, read only),
 * records j there and places member 0; k_grouped_renumber turns every key's slot number into the j of its group or -1; then per
 * member r = 1 .. m - 1 two sweeps over the pass's keys: k_grouped_next_key folds the keys of the group's candidates strictly above
 * member r - 1 under (key, id) into a 32-bit word (atomicMin), k_grouped_next_id folds the ids of those that equal it into out_ids
 * (64-bit atomicMin; the cleared word, all ones, is the padding id); k_grouped_member_dist converts the keys.  A key of a group that
 * was not selected leaves a sweep after one load.  Hazards as above: no kernel waits, spins or locks, every loop is bounded, phases
 * are kernel boundaries, only commutative minima decide a word.
 * Workspace for m > 1, per query of a pass: 12 bytes per key it has room for (key, slot number, the selection's key), 24 per table
 * slot (T + 1 slots, T as above), 12 per result of the one-row selection (k of them) and 4 per member word (k * m of them):
 *   bytes = 12 * per_query_ub + 24 * (T + 1) + 12 * k + 4 * k * m
 * Queries per pass = min(2^29 / per_query_ub, QK_GROUPED_PASS_BYTES / bytes), at least 1.  QK_ERR_INVALID: group_size < 1 (and
 * the checks above); QK_ERR_UNSUPPORTED: group_size > QK_MAX_GROUP_SIZE, a single query whose bytes exceed QK_GROUPED_PASS_BYTES.
 * The cap is a design choice: every member beyond the first costs two sweeps over the pass's keys.
 * timing: the member rounds belong to merge_ms of their pass; n_items stays the number of query passes. */
#define QK_MAX_GROUP_SIZE 16
QK_API int qk_search_grouped_n(qk_ctx *ctx, qk_store *parent, qk_store *s, const float *x, int64_t Q, int nprobe, int k, int group_size,
                               int metric, qk_attr *group_by, qk_filter *filter, int64_t *out_ids, float *out_dist, int64_t *out_groups,
                               int mem, qk_timing *timing);
QK_API int qk_scan_grouped_n(qk_ctx *ctx, qk_store *s, const float *x, int64_t Q, const int64_t *pids, int P, int k, int group_size,
                             int metric, qk_attr *group_by, qk_filter *filter, int64_t *out_ids, float *out_dist, int64_t *out_groups,
                             int mem, qk_timing *timing);
/* builds: derivations of the column's row values so far (one per grouped call that found the store or the column changed);
 * device_bytes: HBM they hold (not part of qk_attr_info).  Either pointer may be NULL. */
QK_API int qk_attr_group_info(qk_attr *a, int64_t *builds, int64_t *device_bytes);

/* ---- facet counts -----------------------------------------------------------------------------------
 * No reference counterpart.  Per query, how many of its range hits carry each value of up to QK_MAX_FACET_COLS columns, and the
 * n_values most frequent values of every column: the aggregation a caller would otherwise compute on the host from every hit's id.
 * Hits: the hit multiset H(q) is BY DEFINITION that of qk_range_search / qk_range_scan for the same (parent, nprobe | pids, metric,
 * radius, filter): the same probed lists (qk_facet_scan: -1, absent and empty lists contribute nothing), the same inclusive
 * float32 radius test (L2 dist <= r, IP dist >= r; qk_ctx_set_squared_l2 is honoured), a NaN distance is never a hit, radius =
 * +inf (L2) / -inf (IP) takes every probed candidate row whose distance is not NaN, a NaN radius is QK_ERR_INVALID, a filter of
 * another store is QK_ERR_INVALID, a row stored twice counts twice.
 * Per column c of facet_by [n_cols] (the same column twice is allowed), val_c(row) being the column's value for the row's id:
 *   total[q]        = |H(q)| = lims[q + 1] - lims[q] of the range call                        out_total [Q] (may be NULL)
 *   missing[c][q]   = hits whose id has no value in c                                         out_missing [n_cols][Q] (may be NULL)
 *   count(c, q, v)  = hits with val_c = v;  sum over v of count + missing = total
 *   distinct[c][q]  = number of v with count > 0                                              out_distinct [n_cols][Q] (may be NULL)
 * Returned: the n_values entries with the largest count, ties broken by the smaller value (signed int64), in that order:
 * out_values / out_counts [n_cols][Q][n_values]; entries behind `distinct` are padding, value = 0 and count = 0 (a returned value
 * always has count >= 1, so count 0 marks padding).  Every int64 is a legal value, -1, INT64_MIN and INT64_MAX included.  The
 * result is a pure function of the store, the columns and the call: counters are integer sums, the selection is exact on distinct
 * keys, and which thread claimed which table slot is not visible.
 * Liveness: values are looked up when the call runs, through the per-row values grouped search keeps (k_grouped_rowvals, re-derived
 * once per column when the store or the column changed).
 * Limits: 1 <= n_cols <= QK_MAX_FACET_COLS and 1 <= n_values <= QK_MAX_FACET_VALUES -- below: QK_ERR_INVALID, above:
 * QK_ERR_UNSUPPORTED; a NULL column or one of another store: QK_ERR_INVALID.  Q == 0: QK_OK.  No lists probed: all zeros.
 * Inside: the key-emission scan of range search (the same launches, the same pass size), then per pass of queries k_facet_hits --
 * the hit test of k_range_count, the hits of every query -- and, per group of queries whose tables fit the workspace,
 * k_facet_clear, k_facet_count -- one sweep over the group's keys for all columns: per column an atomic add to the query's missing
 * counter or to the 32-bit counter of the value's slot in an open-addressing table per (column, query) (64-bit atomicCAS claims,
 * linear probing, at most as many probes as slots; the value -1, the empty marker, owns the slot behind the others) -- and
 * k_facet_select, one workgroup per (column, query): compaction of the occupied slots, an exact most-significant-byte-first
 * selection on the 96-bit key (~count, value ^ sign bit) when more than 256 values are present, a bitonic sort in LDS.  No kernel
 * waits or spins (qk_facet.hip).
 * Workspace: keys as for range search (queries per pass = 2^29 / per_query_ub, per_query_ub = P lists of the store's largest
 * size; a query whose keys exceed 2^30 is QK_ERR_UNSUPPORTED).  Tables are RESERVED by the grouped rule: T + 1 slots of 12 bytes
 * per (column, query), T = the power of two >= max(16, 2 * min(per_query_ub, the largest number of ids with a value among the
 * call's columns)), for min(queries per pass, QK_GROUPED_PASS_BYTES / (12 * n_cols * (T + 1))) queries at a time, at least 1 -- a
 * pass's queries go through the tables group after group; a single query whose tables exceed QK_GROUPED_PASS_BYTES is
 * QK_ERR_UNSUPPORTED.  Tables are USED by a tighter rule, known on the device once the hits are counted: a query's tables have
 * T_q = the power of two >= max(16, 2 * min(its hits, that number of ids)) slots (a query has no more distinct values than hits);
 * only those are cleared, probed and selected from, so a call costs what its hits cost.  Counters are 32-bit inside a pass (a
 * query has fewer than 2^30 keys), outputs int64.  Nothing synchronises between passes or groups.
 * timing: coarse_ms and scan_ms as for range search, merge_ms = counting + selection (of the last pass), n_items = the number of
 * query passes; no list statistics.  qk_ctx_last_scan_kernel names "k_scan (facet)" / "k_scan_wide (facet)".  There is no facet
 * form of qk_search_aps, of the device group, of per-query filter tables or of adaptive probing. */
#define QK_MAX_FACET_COLS 4
#define QK_MAX_FACET_VALUES 256
QK_API int qk_facet_search(qk_ctx *ctx, qk_store *parent, qk_store *s, const float *x, int64_t Q, int nprobe, int metric, float radius,
                           qk_filter *filter, qk_attr *const *facet_by, int n_cols, int n_values, int64_t *out_values,
                           int64_t *out_counts, int64_t *out_distinct, int64_t *out_missing, int64_t *out_total, int mem,
                           qk_timing *timing);
QK_API int qk_facet_scan(qk_ctx *ctx, qk_store *s, const float *x, int64_t Q, const int64_t *pids, int P, int metric, float radius,
                         qk_filter *filter, qk_attr *const *facet_by, int n_cols, int n_values, int64_t *out_values,
                         int64_t *out_counts, int64_t *out_distinct, int64_t *out_missing, int64_t *out_total, int mem,
                         qk_timing *timing);

/* ---- facet statistics -------------------------------------------------------------------------------
 * No reference counterpart.  The numeric half of faceted navigation: per query, over its range hits, the count, minimum, maximum,
 * exact sum and a histogram with caller-chosen bucket edges of up to QK_MAX_FACET_COLS columns -- a price slider, "under 10 /
 * 10-50 / 50-200 / above", the sum and count behind a rating.  None of these follows from the n_values most frequent values of
 * facet counts, and a price or timestamp column has almost as many distinct values as rows.
 * Hits: the hit multiset H(q) is BY DEFINITION that of qk_range_search / qk_range_scan for the same (parent, nprobe | pids, metric,
 * radius, filter), exactly as for facet counts above: the inclusive float32 radius test, qk_ctx_set_squared_l2 honoured, a NaN
 * distance never a hit, a NaN radius QK_ERR_INVALID, radius +inf (L2) / -inf (IP) every probed candidate row, a row stored twice
 * counts twice, -1 / absent / empty lists contribute nothing, a filter or column of another store is QK_ERR_INVALID.
 * Per column c of facet_by [n_cols] (the same column twice is allowed), val_c being the int64 value the column has for a hit's id
 * at the moment of the call; every output but out_total may be NULL, each on its own:
 *   total[q]        = |H(q)|                                                                  out_total [Q]
 *   missing[c][q]   = hits whose id has no value in c                                         out_missing [n_cols][Q]
 *   count[c][q]     = total[q] - missing[c][q]                                                out_count [n_cols][Q]
 *   min / max[c][q] = signed minimum / maximum of val_c over the hits that have a value       out_min, out_max [n_cols][Q]
 *                     count == 0: the identities INT64_MAX / INT64_MIN -- both are legal values, so it is count == 0, not the
 *                     value, that says "no value"
 *   sum[c][q]       = the exact integer sum of val_c, a 128-bit two's-complement number in two words: out_sum_lo [n_cols][Q] its
 *                     low 64 bits (stored in an int64), out_sum_hi [n_cols][Q] its high 64 bits, signed.  It neither wraps nor
 *                     saturates: a query has fewer than 2^30 keys (below), and 2^30 * 2^63 fits 128 bits easily
 *   hist[c][q][b]   : column c comes with n_edges[c] = E edges e_0 < e_1 < ... < e_{E-1}, 0 <= E <= QK_MAX_FACET_EDGES, signed
 *                     int64, strictly ascending, any int64 (INT64_MIN and INT64_MAX included).  The bucket of a value v is
 *                     b(v) = |{i : e_i <= v}|: bucket 0 holds v < e_0, bucket i holds e_{i-1} <= v < e_i, bucket E holds
 *                     v >= e_{E-1}; E == 0: one bucket equal to count.  The buckets of (c, q) add up to count[c][q].
 *                     out_hist [n_cols][Q][hist_stride], hist_stride = 1 + max_c n_edges[c]; entries behind a column's own
 *                     E + 1 buckets are 0
 * edges: the columns' edges one after the other, n_edges [n_cols]: both HOST memory whatever `mem` says (they are small, checked
 * on the host and uploaded once per call); both NULL: no edges, out_hist is then NULL or receives the single bucket.  `mem`
 * governs x / pids / the outputs as everywhere.  Both arrays need to stay valid only until the call returns, also where the call
 * itself returns before the device has finished (device memory, no timing): n_edges and the edges are read on the host inside
 * the call, and the upload is a stream-ordered copy from pageable memory, whose source the runtime has staged when the copy call
 * returns -- the rule every host-to-device copy of this library relies on (qk_store.hip, qk_attr.hip).  That copy may make the
 * host wait once per call, behind the coarse search and in front of the first emission; nothing waits between passes.
 * Every int64 is a legal value.  The result is a pure function of the store, the columns and the call: only integer additions,
 * minima and maxima decide it.  Liveness as for facet counts (the per-row values grouped search keeps).
 * Limits: n_cols < 1, a negative n_edges[c], edges that are not strictly ascending, a NULL column, one of edges / n_edges NULL
 * while the other names edges: QK_ERR_INVALID; n_cols > QK_MAX_FACET_COLS, n_edges[c] > QK_MAX_FACET_EDGES: QK_ERR_UNSUPPORTED.
 * Q == 0: QK_OK.  No lists probed: every count is zero, min / max hold their identities.
 * Inside: the key-emission scan of range search (the same launches, the same pass size), then per pass of queries ONE sweep,
 * k_facet_stats, over all columns and all queries of the pass -- no table sized by hits, no group loop, no selection: the
 * decomposition and the hit test of k_facet_hits; every lane keeps per column min / max (on sign-flipped words) and two sum
 * accumulators in registers (the low 32 bits of every value added unsigned into 64 bits, the high 32 bits added signed into 64
 * bits: below 2^30 hits neither can overflow, together they are the exact sum); a hit's bucket comes from a branch-free binary
 * search (8 steps) over the call's edges in LDS and is counted by an LDS atomic add; behind its last slice a workgroup reduces
 * across the wave (shuffles), across its four waves (LDS) and issues one global atomic per statistic (add / min / max) and per
 * non-zero bucket.  k_facet_stats_finish widens the counters, undoes the sign flip, combines the sum halves with the carry and
 * writes the outputs.  No kernel waits or spins (qk_facet.hip, second part).
 * Workspace: keys as for range search (queries per pass = 2^29 / per_query_ub; a query whose keys exceed 2^30 is
 * QK_ERR_UNSUPPORTED); next to them 4 + 36 * n_cols bytes of accumulators per query of a pass, plus 4 * n_cols * hist_stride when
 * a histogram with edges is asked for; a pass is shortened only where these would exceed QK_GROUPED_PASS_BYTES.  Nothing
 * synchronises between passes.
 * timing: coarse_ms and scan_ms as for range search, merge_ms = sweep + finish (of the last pass), n_items = the number of query
 * passes.  qk_ctx_last_scan_kernel names "k_scan (facet stats)" / "k_scan_wide (facet stats)".  There is no form for
 * qk_search_aps, the device group, per-query filter tables or adaptive probing. */
#define QK_MAX_FACET_EDGES 255
QK_API int qk_facet_stats_search(qk_ctx *ctx, qk_store *parent, qk_store *s, const float *x, int64_t Q, int nprobe, int metric,
                                 float radius, qk_filter *filter, qk_attr *const *facet_by, int n_cols, const int64_t *edges,
                                 const int *n_edges, int64_t *out_count, int64_t *out_missing, int64_t *out_min, int64_t *out_max,
                                 int64_t *out_sum_lo, int64_t *out_sum_hi, int64_t *out_hist, int64_t *out_total, int mem,
                                 qk_timing *timing);
QK_API int qk_facet_stats_scan(qk_ctx *ctx, qk_store *s, const float *x, int64_t Q, const int64_t *pids, int P, int metric,
                               float radius, qk_filter *filter, qk_attr *const *facet_by, int n_cols, const int64_t *edges,
                               const int *n_edges, int64_t *out_count, int64_t *out_missing, int64_t *out_min, int64_t *out_max,
                               int64_t *out_sum_lo, int64_t *out_sum_hi, int64_t *out_hist, int64_t *out_total, int mem,
                               qk_timing *timing);

/* ---- ordered search ---------------------------------------------------------------------------------
 * No reference counterpart.  "Sort by": per query, the k first of its range hits by an attribute column -- the 10 cheapest items
 * near this query, the 20 newest documents within this radius, highest rated first.
 * Hits: the hit multiset H(q) is BY DEFINITION that of qk_range_search / qk_range_scan for the same (parent, nprobe | pids, metric,
 * radius, filter), exactly as for facet counts above: the inclusive float32 radius test, qk_ctx_set_squared_l2 honoured, a NaN
 * distance never a hit, a NaN radius QK_ERR_INVALID, radius +inf (L2) / -inf (IP) every probed candidate row, a row stored twice
 * is two hits, -1 / absent / empty lists contribute nothing.
 * order_by: one column of the store.  flags: QK_ORDER_DESC | QK_ORDER_MISSING_LAST.  1 <= k <= QK_MAX_ORDER_K; below:
 * QK_ERR_INVALID, above: QK_ERR_UNSUPPORTED.
 * Order: every hit has a record (class, value, key, id), compared field by field:
 *   class  0 if the row's id has a value in the column at the moment of the call, 1 if not
 *   value  the signed int64 value, ascending; descending under QK_ORDER_DESC.  Every int64 is legal (INT64_MIN, INT64_MAX, -1).
 *          Records of class 1 compare equal on it
 *   key    the search order's uint32 key of the pair: smaller = nearer under both metrics, -0 and +0 share a key (the key
 *          qk_search_after documents) -- ascending in BOTH directions
 *   id     signed, ascending
 * -- by the column in the direction asked, ties to the nearer row, ties of those to the smaller id, as qk_search breaks them.
 * Two hits that tie on all four fields (a row stored twice) are indistinguishable; each is an entry.
 * Returned: without QK_ORDER_MISSING_LAST the first min(k, count[q]) records of class 0; with it the first min(k, total[q]) records
 * of both classes, class 1 behind class 0 -- entry j has a value iff j < count[q].
 *   out_ids     [Q][k]               padding -1
 *   out_dist    [Q][k], may be NULL  the float32 distance qk_search reports for the pair; padding +inf (L2) / -inf (IP)
 *   out_values  [Q][k], may be NULL  0 for entries without a value and for padding
 *   out_count   [Q], may be NULL     hits with a value   } as int64; equal to count, missing and total of
 *   out_missing [Q], may be NULL     hits without one    } qk_facet_stats_search for the same arguments
 *   out_total   [Q], may be NULL     count + missing     }
 * Q == 0: QK_OK.  No lists probed: all padding and zeros.  The result is a pure function of the store, the column and the call.
 * Liveness as for facets: values are read when the call runs, through the per-row values grouped search keeps; a later
 * set / add / remove / maintenance is seen by the next call.
 * Limits: a NULL column, a column or filter of another store, unknown flag bits: QK_ERR_INVALID.  A query whose keys exceed 2^30 is
 * QK_ERR_UNSUPPORTED (qk_emit_passes).  There is no form for qk_search_aps, the device group, per-query filter tables or adaptive
 * probing.
 * Inside (qk_order.hip): the key-emission scan of range search (the same launches), then per pass k_order_partial -- the
 * decomposition and hit test of k_facet_stats; every workgroup keeps the k smallest records it met in an LDS buffer of 512 / 1024 /
 * 2048 records (k <= 64 / 256 / 1024 = KP) that a bitonic pass cuts back to k whenever fewer than 256 slots are free, the k-th record
 * being the bound later hits are compared against in registers -- and k_order_merge, one workgroup per query, which streams the
 * workgroups' sorted lists through the same buffer and writes the outputs.  No kernel waits or spins.
 * Workspace: keys as for range search; next to them 8 bytes of counters per query and Sg lists of KP records of 24 bytes per
 * query, Sg = min(slices of a query, 256, 16384 / queries of the pass, 128 MiB / (queries per pass * list bytes)), at least 1: a
 * large k lowers Sg, never refuses; a pass is shortened only where one list per query would exceed QK_GROUPED_PASS_BYTES.
 * timing: coarse_ms and scan_ms as for range search, merge_ms = partial + merge (of the last pass), n_items = the number of query
 * passes.  qk_ctx_last_scan_kernel names "k_scan (order)" / "k_scan_wide (order)". */
#define QK_MAX_ORDER_K 1024
#define QK_ORDER_DESC 1
#define QK_ORDER_MISSING_LAST 2
QK_API int qk_order_search(qk_ctx *ctx, qk_store *parent, qk_store *s, const float *x, int64_t Q, int nprobe, int metric, float radius,
                           qk_filter *filter, qk_attr *order_by, int flags, int k, int64_t *out_ids, float *out_dist,
                           int64_t *out_values, int64_t *out_count, int64_t *out_missing, int64_t *out_total, int mem,
                           qk_timing *timing);
QK_API int qk_order_scan(qk_ctx *ctx, qk_store *s, const float *x, int64_t Q, const int64_t *pids, int P, int metric, float radius,
                         qk_filter *filter, qk_attr *order_by, int flags, int k, int64_t *out_ids, float *out_dist,
                         int64_t *out_values, int64_t *out_count, int64_t *out_missing, int64_t *out_total, int mem,
                         qk_timing *timing);

/* ---- multi-vector search ------------------------------------------------------------------------------
 * No reference counterpart.  Late interaction (ColBERT / ColPali token embeddings, a question expanded into several vectors): a
 * logical query is T sub-queries, a document is the rows whose ids share a value of an attribute column, and
 *   score(doc) = sum over the sub-queries t of the best hit of t among the document's rows     (sum of MaxSim)
 * x: [L * T][d], logical query l owns the sub-queries l * T .. l * T + T - 1; qk_maxsim_scan: pids [L * T][P].  n_tokens: int32 [L]
 * in `mem`, or NULL meaning T for every logical query; only the first n_tokens[l] sub-queries of l take part.  A host value outside
 * [0, T] is QK_ERR_INVALID, a device value is clamped to [0, T].
 * 1 <= T <= QK_MAXSIM_MAX_TOKENS, 1 <= k <= QK_MAXSIM_MAX_K; below: QK_ERR_INVALID, above: QK_ERR_UNSUPPORTED.  `missing` NaN:
 * QK_ERR_INVALID.  L == 0: QK_OK.
 * Hits: the hit multiset H(l, t) is BY DEFINITION that of qk_range_search / qk_range_scan for sub-query l * T + t with the same
 * (parent, nprobe | pids, metric, radius, filter), exactly as for facet counts and ordered search above: the inclusive float32 radius
 * test, qk_ctx_set_squared_l2 honoured, a NaN distance never a hit, a NaN radius QK_ERR_INVALID, radius +inf (L2) / -inf (IP) every
 * probed candidate row.  A sub-query with t >= n_tokens[l] has no hits.
 * Terms: a hit whose id has a value g in group_by at the moment of the call is a candidate of (l, t, g).  best(l, t, g) is the
 * candidate with the smallest search key (the uint32 key qk_search_after documents; ids do not matter), term(l, t, g) the float32
 * distance qk_range_search reports for that key -- sqrtf for L2 unless qk_ctx_set_squared_l2, the product for IP.  Without a
 * candidate term(l, t, g) = missing; every float but NaN is a legal `missing`, +-inf included (0 is the usual choice for IP).
 * Score: s = +0.0f, then for t = 0 .. n_tokens[l] - 1 in that order s = s + term(l, t, g): one separately rounded float32 addition
 * each, no reassociation, no tree, no wider accumulator (the library is built with -ffp-contract=off and without fast-math).
 * Candidates of l: every value g with a candidate in at least one participating t.
 * Order: the better score first -- larger for IP, smaller for L2 -- compared as float32 values (-0 equals +0); a NaN score
 * (inf + -inf) sorts behind every number; ties, and NaN among NaN, go to the smaller signed value.  Every int64 is a legal value:
 * -1, INT64_MIN, INT64_MAX.
 * Returned, entries behind min(k, n_groups[l]) being padding:
 *   out_groups   [L][k]   int64                 padding 0
 *   out_scores   [L][k]   float32, may be NULL  padding +inf (L2) / -inf (IP); a NaN score is reported as 0x7FC00000
 *   out_matched  [L][k]   int32, may be NULL    the number of t with a candidate; padding 0
 *   out_n_groups [L]      int64, may be NULL    the exact number of candidate values
 *   out_hits     [L][T]   int64, may be NULL    |H(l, t)| = lims[q + 1] - lims[q] of the range call for q = l * T + t; 0 for a t that
 *                                               does not take part
 * No lists probed: all padding and zeros.  The result is a pure function of the store, the column, the filter and the call, and row
 * l equals the call made with logical query l alone.  Liveness as for facets: values are read when the call runs, through the
 * per-row values grouped search keeps; a later set / add / remove / maintenance is seen by the next call.
 * Limits: a NULL column, a column or filter of another store: QK_ERR_INVALID.  A sub-query whose keys exceed 2^30 is
 * QK_ERR_UNSUPPORTED (qk_emit_passes).  There is no form for qk_search_aps, the device group, per-query filter tables or adaptive
 * probing.
 * Inside (qk_maxsim.hip): the key-emission scan of range search over the L * T sub-queries (the same launches), then per pass
 * k_maxsim_hits (the hits of every sub-query) and, per group of logical queries that fits the pool of table slots, k_maxsim_clear, k_maxsim_claim -- a candidate finds
 * or claims the slot of its value in the table of its LOGICAL query (atomicCAS, linear probing bounded by the table) and lowers key
 * word t of the slot (atomicMin) -- and k_maxsim_select, one workgroup per logical query: terms, sequential sum and matched count of
 * every occupied slot, an exact byte-wise selection on (score word, value ^ sign bit) down to k when more than 1024 values are met,
 * a bitonic sort in LDS, outputs and padding.  No kernel waits or spins.
 * Workspace: keys as for range search over the sub-queries, except that queries per pass = the wide-k rule (min(L * T, 2^29 /
 * per_query_ub)) lowered to a multiple of T -- a logical query never straddles a pass; fewer than T is QK_ERR_UNSUPPORTED.  Next to
 * the keys 4 bytes per sub-query, 8 per logical query and a POOL of table slots of 16 + 4 * T bytes each: min(logical queries per
 * pass * (S + 1), QK_GROUPED_PASS_BYTES / slot bytes) slots, S = the power of two >= max(16, 2 * min(T * per_query_ub, ids of the
 * column)) being the most one logical query can ever use.  The pool is laid out per pass by the HITS: behind k_maxsim_hits the host
 * reads the pass's hit counts back (4 bytes per sub-query, the one wait inside a pass), gives every logical query a table of the
 * power of two >= max(16, 2 * min(its hits, ids of the column)) slots plus 2, and sends the pass's logical queries through the pool
 * in groups that fit it.  So the workspace follows what a query hits, not the largest list of the store; only a single logical query
 * whose own table exceeds the pool -- more than about QK_GROUPED_PASS_BYTES / (2 * slot bytes) hits -- is QK_ERR_UNSUPPORTED.
 * timing: coarse_ms and scan_ms as for range search, merge_ms = everything behind the last emission, n_items = the number of query
 * passes.  qk_ctx_last_scan_kernel names "k_scan (maxsim)" / "k_scan_wide (maxsim)". */
#define QK_MAXSIM_MAX_TOKENS 64
#define QK_MAXSIM_MAX_K 1024
QK_API int qk_maxsim_search(qk_ctx *ctx, qk_store *parent, qk_store *s, const float *x, int64_t L, int T, const int32_t *n_tokens,
                            int nprobe, int metric, float radius, qk_filter *filter, qk_attr *group_by, float missing, int k,
                            int64_t *out_groups, float *out_scores, int32_t *out_matched, int64_t *out_n_groups, int64_t *out_hits,
                            int mem, qk_timing *timing);
QK_API int qk_maxsim_scan(qk_ctx *ctx, qk_store *s, const float *x, int64_t L, int T, const int32_t *n_tokens, const int64_t *pids,
                          int P, int metric, float radius, qk_filter *filter, qk_attr *group_by, float missing, int k,
                          int64_t *out_groups, float *out_scores, int32_t *out_matched, int64_t *out_n_groups, int64_t *out_hits,
                          int mem, qk_timing *timing);

/* ---- diversified search ------------------------------------------------------------------------------
 * No reference counterpart.  Maximal marginal relevance (MMR): of the fetch_k nearest rows of a query keep k, chosen greedily -- each
 * step takes the candidate that is close to the query and far from everything already taken (the near-duplicate chunks of a
 * document that crowd a plain top-k).  Exact and bit for bit, like every other call.
 * All values below are float32 in the domain the caller sees from qk_search: sqrt L2, squared L2 after qk_ctx_set_squared_l2(ctx, 1),
 * the dot product for IP.  C = fetch_k, lambda in [0, 1], mu = fl(1 - lambda).
 * Candidates: c_0 .. c_{n-1}, n <= C, are the non-padding entries of the row that qk_search (qk_search_filtered with a filter;
 *   qk_scan / qk_scan_filtered for the pids form) returns for the query with k = C and the same other arguments, in that order --
 *   the total order (key, id) -- with the reported distances r_0 .. r_{n-1}.  The index i is the candidate's RANK.
 * Pairwise values: p(i, j) = the distance qk_search would report for the stored row of c_i when the query is the stored vector of
 *   c_j: one k-ordered fp32 fmaf chain for the dot product, the expanded L2 form over the two stored norms with its clamp, the
 *   correctly rounded sqrt unless squared L2 is set.  Symmetric.
 * Selection: the first pick is rank 0.  While fewer than min(k, n) are picked, for every unpicked i:
 *   N_i    = the most similar pairwise value to the picked set S: min over s in S of p(i, s) for L2, max for IP; NaN values are
 *            ignored; if all are NaN the term is dropped and cost_i = fl(lambda * r_i)
 *   cost_i = fl( fl(lambda * r_i) - fl(mu * N_i) ) -- three separately rounded float32 operations, no contraction
 *   pick the smallest cost for L2, the largest for IP; a NaN cost (inf - inf, 0 * inf) loses to every non-NaN cost; ties, and the
 *   all-NaN case, go to the smaller rank.
 * Returned, in selection order:
 *   out_ids  [Q][k]               padding -1 behind min(k, n)
 *   out_dist [Q][k], may be NULL  the r values; padding +inf (L2) / -inf (IP)
 *   out_rank [Q][k], may be NULL  int32, the rank of each pick; padding -1
 * Consequences: lambda = 1 returns the first k entries of the qk_search(k = C) row, ids and distance bits equal; C == k returns a
 * permutation of the qk_search(k) row; row q equals the call made with query q alone.  An id stored more than once takes the vector
 * of its smallest arena row.
 * Limits: 1 <= k <= fetch_k <= QK_MAX_FETCH_K = 256 (inside QK_MAX_K: the filtered tile form serves every C); k < 1 or
 * fetch_k < k: QK_ERR_INVALID, fetch_k > 256: QK_ERR_UNSUPPORTED; a lambda that is NaN or outside [0, 1]: QK_ERR_INVALID; d up to
 * QK_MAX_D; Q == 0: QK_OK; a filter of another store: QK_ERR_INVALID.  qk_diverse_scan: P >= 1, pids as for qk_scan_filtered (-1 /
 * empty lists contribute nothing; host pids naming an absent list: QK_ERR_NOT_FOUND).  There is no form for qk_search_aps, the
 * device group, per-query filter tables, adaptive probing or exact filtered search.
 * Inside (qk_diverse.hip): the candidate search is the shipped one, called unchanged with k = C into a buffer of the context; behind
 * it in the same enqueue, without a host wait, per group of at most 2^22 / C queries: k_diverse_insert (the distinct candidate ids
 * claim slots of an open-addressing table of at least 2 * queries * C slots, atomicCAS), k_diverse_rows (one sweep over the stored
 * ids of every live arena row; a row whose id is in the table writes its row there, atomicMin) and k_diverse_select (one workgroup
 * per query, one lane per candidate; the query's C rows staged in LDS once when C * (dpad + 4) * 4 bytes fit 144 KiB, else the
 * picked vector staged per step and the candidate rows re-read from the arena).  No kernel waits or spins on another.
 * Workspace, kept on the context: Q * C * 12 bytes of candidates, 16 bytes per table slot (at most 128 MiB), and a host caller's
 * staged buffers.
 * timing: as the candidate search fills it; the re-ranking tail lies behind that search's events and is part of total_ms only,
 * like the cut of an adaptive call.  qk_ctx_last_scan_kernel names the candidate search's kernel. */
#define QK_MAX_FETCH_K 256
QK_API int qk_diverse_search(qk_ctx *ctx, qk_store *parent, qk_store *s, const float *x, int64_t Q, int nprobe, int k, int fetch_k,
                             float lambda, int metric, qk_filter *filter /* or NULL */, int64_t *out_ids, float *out_dist,
                             int32_t *out_rank, int mem, qk_timing *timing);
QK_API int qk_diverse_scan(qk_ctx *ctx, qk_store *s, const float *x, int64_t Q, const int64_t *pids, int P, int k, int fetch_k,
                           float lambda, int metric, qk_filter *filter /* or NULL */, int64_t *out_ids, float *out_dist, int32_t *out_rank,
                           int mem, qk_timing *timing);

/* Paged search: continue a search behind a cursor.  Results are totally ordered by (key, id): the key is the 32-bit integer the
 * top-k compares (a monotone image of the squared L2 distance / of the negated inner product), ids are unique and non-negative,
 * and the key 0xFFFFFFFF (a NaN value) is never a candidate.  A cursor (ck, cid) is a position in that order, not a snapshot.
 *   Candidates of query i with cursor (ck, cid): the rows of the probed lists whose key is not 0xFFFFFFFF and whose (key, id) >
 *     (ck, cid) lexicographically -- unsigned key, signed id -- and which `filter` (may be NULL) allows.
 *   Probed lists: the unfiltered qk_search's (the same min(nprobe, parent lists) in the same rank order; every list when parent ==
 *     NULL); qk_scan_after: the pids row, as qk_scan.
 *   The page: the k smallest candidates in (key, id) order, padded with id -1 and distance +inf (L2) / -inf (IP) as qk_search pads.
 *   Start cursor: (0, -1) lies below every row.  after_key == after_id == NULL means that cursor for every query; the page then
 *     equals qk_search's (qk_search_filtered's) bit for bit, ids and distances.
 *   Next cursor: a row that holds k results -> the (key, id) of its k-th, the key being the integer the merge compared (not
 *     re-derived from the reported distance: sqrt is not injective in fp32); fewer, or none -> the exhausted cursor
 *     (0xFFFFFFFF, INT64_MAX), behind which every page is padding.
 * So pages of any sizes chained from the start cursor concatenate to a prefix of the full ordering; after qk_store_add_* /
 * remove between two pages the later page holds the then-current rows behind the cursor and no row is returned twice for one
 * query; the queries of a batch may sit at different depths.  A page costs one filtered-form search whatever its depth: it works
 * under a filter, where k > QK_MAX_K has no other route, and it has no depth limit.
 * after_key / next_key: uint32 [Q], after_id / next_id: int64 [Q], all in `mem`; next_* may alias after_* and may both be NULL.
 * 1 <= k <= QK_MAX_K (QK_ERR_UNSUPPORTED beyond).  QK_ERR_INVALID: exactly one of after_key / after_id (of next_key / next_id) is
 * NULL; the filter belongs to another store.  There is no paged form of the per-query filter tables, of adaptive probing, of
 * qk_search_aps or of the device group.
 * The scan is the filtered call's: k_scan_after / k_scan_wide_after -- the filtered tile form with the cursor test in its
 * epilogue, qk_ctx_last_scan_kernel names "k_scan (after)" / "k_scan_wide (after)" -- without bound seeding: the k nearest rows
 * of a later page all lie before the cursor and must not set a bound.  Without a filter the same kernels run under a deny-nothing
 * filter the store keeps (made by the first such call: a few allocations once per store; counted by neither
 * qk_store_device_bytes nor any qk_filter_info).  k_next_cursor writes the next cursors behind the merge.  One enqueue: with
 * device memory nothing waits for the stream unless `timing` is given. */
QK_API int qk_search_after(qk_ctx *ctx, qk_store *parent, qk_store *s, const float *x, int64_t Q, int nprobe, int k, int metric,
                           const uint32_t *after_key, const int64_t *after_id, qk_filter *filter, int64_t *out_ids, float *out_dist,
                           uint32_t *next_key, int64_t *next_id, int mem, qk_timing *timing);
QK_API int qk_scan_after(qk_ctx *ctx, qk_store *s, const float *x, int64_t Q, const int64_t *pids, int P, int k, int metric,
                         const uint32_t *after_key, const int64_t *after_id, qk_filter *filter, int64_t *out_ids, float *out_dist,
                         uint32_t *next_key, int64_t *next_id, int mem, qk_timing *timing);

/* QueryCoordinator::search with SearchParams::recall_target > 0 and batched_scan == false: adaptive partition
 * scanning (query_coordinator.cpp:612-657 picks M = max((int)(nlist * initial_search_fraction), 1) candidate partitions
 * from the parent; the use_aps branch of serial_scan, :471-611, scans them in rank order and stops a query once the
 * recall estimate of include/geometry.h:57-113,247-295,345-407 reaches recall_target).  The batch advances in rounds on
 * the device; per query the result and the count of partitions scanned are those of the sequential walk.
 * out_ids/out_dist [Q][k]; out_nscanned [Q] (may be NULL) = partitions the walk visited; timing (may be NULL):
 * total_ms and n_items = rounds.  Errors: parent == NULL or fewer than 2 candidates -> QK_ERR_INVALID
 * ("Boundary distances must have at least 2 partitions to create an estimate.", geometry.h:350). */
QK_API int qk_search_aps(qk_ctx *ctx, qk_store *parent, qk_store *s, const float *x, int64_t Q, int k, int metric,
                         float recall_target, float recompute_threshold, int use_precomputed, float initial_search_fraction,
                         int64_t *out_ids, float *out_dist, int32_t *out_nscanned, int mem, qk_timing *timing);

/* Multi-GPU merge step (the cross-worker batch_add of worker_scan, query_coordinator.cpp:167-173,231-235):
 * merge G per-rank results [G][Q][k] (already all-gathered by the caller, e.g. torch.distributed over RCCL) into
 * [Q][k] under the same (key,id) order.  in_key are SQUARED L2 distances / inner products, i.e. what qk_search
 * returns after qk_ctx_set_squared_l2(ctx, 1); the output distances are sqrt'd.  Device pointers only.
 * Precondition: every rank's row of k entries is a SORTED run under the (key, id) order with its -1 padding as a suffix -- what
 * qk_search returns.  (k <= 960 pools the entries and would take any order; k > 960 merges the runs by binary search and relies
 * on it.)  An entry with id < 0 or a NaN key is no candidate, whatever k: it is not returned.  The same (key, id) on two ranks is
 * returned twice. */
QK_API int qk_merge_topk(qk_ctx *ctx, const int64_t *in_ids, const float *in_key, int G, int64_t Q, int k, int metric,
                         int64_t *out_ids, float *out_dist);
/* The same exchange as ONE collective (the ids + keys of an entry travel together, 12 bytes): qk_pack_topk turns a rank's local
 * result ids/key [G*per][k] into G blocks of qk_topk_block_bytes(per, k) bytes -- block j = queries [j*per, (j+1)*per): per*k
 * int64 ids then per*k float keys, padded to 16 bytes -- which is the send buffer of one all_to_all_single with equal splits;
 * qk_merge_topk_packed merges the receive buffer (block r = rank r's results for this rank's `per` queries) into [per][k]
 * under the same (key,id) order.  Device pointers only; 16-byte aligned buffers. */
QK_API size_t qk_topk_block_bytes(int64_t per, int k);
QK_API int qk_pack_topk(qk_ctx *ctx, const int64_t *ids, const float *key, int G, int64_t per, int k, void *packed);
QK_API int qk_merge_topk_packed(qk_ctx *ctx, const void *packed, int G, int64_t per, int k, int metric, int64_t *out_ids,
                                float *out_dist);
/* Test and diagnosis hook: the per-query merge stage of qk_scan / qk_search on records the CALLER laid out, so that a test decides
 * the geometry the merge kernels meet (behind a scan it is a by-product of the scan plan and the CU count).  Device pointers only.
 * The layout is the scan's: pair_slots [Q*P][32] = {record count of the pair, its first 31 record numbers (-1: a record that did
 * not fit)}; pair_head [Q*P] = head of the chain of the records beyond 31 (-1: none), linked through rec_hdr[r][0]; rec_hdr
 * [max_recs][2] = {next record of the chain or -1, entry count n <= k}; rec_ord / rec_id [max_recs][k] = the record's n entries
 * sorted under (key, id), keys as the merge orders them (L2: the bits of the squared distance; IP: the descending map; 0xFFFFFFFF =
 * NaN).  form: 0 = the rule a search applies to (k, P); 1 = the chained walk k_merge<MAXCH>; 2 = k_merge_flat (k <= 32, P <= 64);
 * 3 = k_merge_wide.  out_ids / out_dist [Q][k] as qk_scan writes them (out_dist may be NULL; sqrt_l2: L2 distances leave as
 * sqrt); next_key / next_id [Q] (both NULL, or both set): the next cursor of qk_search_after, written by the same kernel behind
 * the merge.  kernel_name (may be NULL): the kernel and instantiation launched, e.g. "k_merge_flat<2>".  A form the arguments do
 * not admit, k > QK_MAX_K: QK_ERR_INVALID, nothing is launched.  The structures must be WELL FORMED -- every record number -1 or
 * below max_recs, every chain ending in -1: the kernels trust them as they trust the scan.  No reference counterpart. */
QK_API int qk_debug_merge_records(qk_ctx *ctx, int64_t Q, int P, int k, int metric, int sqrt_l2, int form, const int32_t *pair_slots,
                                  const int32_t *pair_head, const int32_t *rec_hdr, const uint32_t *rec_ord, const int64_t *rec_id,
                                  int32_t max_recs, int64_t *out_ids, float *out_dist, uint32_t *next_key, int64_t *next_id,
                                  char *kernel_name, int name_len);
/* Test and diagnosis hook: the exact finish of the fp16 shadow form (k_shadow_finish, through the launcher a search uses) on records
 * the CALLER laid out over a real store, so that a test decides how many records, entries and candidates a query has.  HOST
 * pointers only.  x [Q][d] queries (their norms come from the library's own preparation), E [Q] error bounds (negative or NaN: no
 * bound), lists [Q] the probed list of every query (-1: none).  pair_slots [Q][32], pair_head [Q], rec_hdr [max_recs][2] as for
 * qk_debug_merge_records with P = 1; rec_ord [max_recs][32] approximate keys, ascending within a record; ent_list / ent_pos
 * [max_recs][32]: every entry's row as (list number, position in the list's arena order) -- the hook turns them into arena rows
 * from the store's table.  out_ids / out_dist [Q][k] (out_dist may be NULL); counters [4]: what this call added to verified,
 * fallback, candidates, queries with chained records (qk_ctx_shadow_stats).  A list or position out of range, a record number
 * outside [-1, max_recs), an entry count outside [0, 32], a chain that does not end, k > 16 or d > 256: QK_ERR_INVALID, nothing is
 * launched -- the kernel trusts well-formed structures as it trusts the scan.  No reference counterpart. */
QK_API int qk_debug_shadow_finish(qk_ctx *ctx, qk_store *store, int64_t Q, int k, int metric, int sqrt_l2, const float *x, const float *E,
                                  const int64_t *lists, const int32_t *pair_slots, const int32_t *pair_head, const int32_t *rec_hdr,
                                  const uint32_t *rec_ord, const int64_t *ent_list, const int64_t *ent_pos, int32_t max_recs,
                                  int64_t *out_ids, float *out_dist, int64_t *counters);
/* When enabled, qk_scan/qk_search return squared L2 distances (the merge key) instead of sqrt distances. */
QK_API int qk_ctx_set_squared_l2(qk_ctx *ctx, int enabled);

/* ---- device group: IndexBuildParams::num_workers as GPUs ---------------------------------------------------------------
 * The reference spreads a search over cores with num_workers (common.h:73,127): QueryCoordinator::initialize_workers
 * (query_coordinator.cpp:50-74) starts one thread per core, PartitionManager::distribute_partitions pins partition i to core
 * i % num_workers (partition_manager.cpp:557-603), worker_scan (query_coordinator.cpp:243-469) hands every core the jobs of its
 * partitions and batch_adds the per-core buffers into the global one (:167-173,231-235).  Here a worker is a device: a group is
 * ONE process driving G members -- one context + one shard store each; members may share a physical device (num_workers larger
 * than the node, and one-GPU test boxes) -- and list p lives in member p % G.  A search: the batch reaches the lead (member 0),
 * the others pull it over xGMI; the coarse step is split by queries and every member writes its slice of the [Q][nprobe] list
 * numbers straight into every other member's copy (peer stores); every member scans the whole batch over ITS lists and writes
 * its packed [Q][k] (ids, merge keys) block -- qk_pack_topk's layout -- into the lead's receive buffer; the lead merges the G
 * blocks under the (key, id) order.  Events order the devices; there is no host thread per device and no host synchronisation
 * inside a call on device buffers.  Results (ids and distance bits) equal the one-store search on the same lists.
 * Requires peer access between all distinct devices of the group (QK_ERR_UNSUPPORTED otherwise). */
typedef struct qk_group qk_group;
QK_API int qk_group_create(const int *devices, int G, int d, qk_group **out);   /* initialize_workers :50-74 */
QK_API int qk_group_destroy(qk_group *g);                                       /* shutdown_workers :77-95 */
QK_API int qk_group_size(qk_group *g);
/* member i's context and shard store (borrowed; the store holds the lists p with p % G == i under their global numbers) */
QK_API int qk_group_member(qk_group *g, int i, qk_ctx **ctx, qk_store **store);
QK_API int qk_group_owner(qk_group *g, int64_t list_no);                        /* get_partition_core_id: list_no % G */
/* The lead's stream: outputs in device memory are complete in its order (qk_ctx_set_stream / _set_null_stream / _get_stream of
 * the lead's context); inputs in device memory are read behind whatever that stream holds at the time of the call. */
QK_API int qk_group_set_stream(qk_group *g, void *hip_stream);
QK_API int qk_group_set_null_stream(qk_group *g);
QK_API int qk_group_get_stream(qk_group *g, void **hip_stream, int *kind);
QK_API int qk_group_synchronize(qk_group *g);                                   /* every member's stream */
/* Submit threads (default on, G >= 2): the per-member pieces of a search -- pull the batch, rank a slice of it, scan, pack -- are
 * enqueued by one persistent host thread per member instead of the caller's thread one member after the other (0.39 ms of host
 * time per call at 8 members -> one member's share plus two fork-joins).  Same streams, same events, same results; 0 = the
 * caller's thread does everything.  Reference: one scan thread per worker, query_coordinator.cpp:50-74,98-240. */
QK_API int qk_group_set_submit_threads(qk_group *g, int enabled);
QK_API int qk_group_set_form_feedback(qk_group *g, int enabled);                /* qk_ctx_set_form_feedback on every member */
/* The store surface over the members (same arguments, same errors as the qk_store_* call each one routes to). */
QK_API int qk_group_reset(qk_group *g);
QK_API int qk_group_add_list(qk_group *g, int64_t list_no);
QK_API int qk_group_remove_list(qk_group *g, int64_t list_no);
QK_API int qk_group_add_entries(qk_group *g, int64_t list_no, int64_t n, const int64_t *ids, const float *vecs, int mem);
QK_API int qk_group_add_batch(qk_group *g, int64_t n, const int64_t *ids, const float *vecs, const int64_t *assign, int mem);
QK_API int qk_group_build_csr(qk_group *g, int64_t nlist, const int64_t *offsets_host, const int64_t *ids, const float *vecs,
                              int mem);                                         /* init_partitions + distribute_partitions */
QK_API int qk_group_remove_ids(qk_group *g, int64_t n, const int64_t *ids_host, int64_t *n_removed);
QK_API int qk_group_list_size(qk_group *g, int64_t list_no, int64_t *out);
QK_API int qk_group_list_sizes(qk_group *g, const int64_t *list_nos, int64_t n, int64_t *out);
QK_API int64_t qk_group_ntotal(qk_group *g);
QK_API int64_t qk_group_nlist(qk_group *g);
QK_API int qk_group_d(qk_group *g);
QK_API int qk_group_list_ids(qk_group *g, int64_t *out_host, int64_t *n);
QK_API int qk_group_get_list(qk_group *g, int64_t list_no, float *vecs_out, int64_t *ids_out, int mem); /* complete on return */
QK_API int qk_group_get_lists(qk_group *g, const int64_t *list_nos, int64_t n, float *vecs_out, int64_t *ids_out, int mem);
QK_API int qk_group_get_vector(qk_group *g, int64_t id, float *vec_out_host, int *found);
QK_API int64_t qk_group_device_bytes(qk_group *g);
/* qk_store_refine_lists over lists of several members: they meet in a temporary store on the member holding the first one,
 * are refined there (same order, same arithmetic) and go back to their owners, device to device. */
QK_API int qk_group_refine_lists(qk_group *g, const int64_t *list_nos, int64_t m, float *centroids, int metric,
                                 int refinement_iterations, int mem);
/* worker_scan (query_coordinator.cpp:243-469) through scan_partitions (:659-673): qk_scan over the members. */
QK_API int qk_group_scan(qk_group *g, const float *x, int64_t Q, const int64_t *pids, int P, int k, int metric, int64_t *out_ids,
                         float *out_dist, int mem, qk_timing *timing);
/* QueryCoordinator::search (:612-657) with workers: qk_search over the members.  `parent` is the parent's ordinary store (any
 * device); the group keeps a replica of it per member and refreshes the replicas when the parent has changed.  timing:
 * coarse_ms / scan_ms / merge_ms / total_ms between events on the lead, the counters summed over the members. */
QK_API int qk_group_search(qk_group *g, qk_store *parent, const float *x, int64_t Q, int nprobe, int k, int metric,
                           int64_t *out_ids, float *out_dist, int mem, qk_timing *timing);
/* qk_search_aps over the members (the APS hook of worker_scan, query_coordinator.cpp:364-428 -- whose outcome depends on thread
 * timing upstream; here the deterministic walk): the rounds run on the lead, every member scans the pairs of a round whose lists it
 * holds, the lead takes each pair's top-k from its owner.  Answers and partitions visited equal qk_search_aps on one store. */
QK_API int qk_group_search_aps(qk_group *g, qk_store *parent, const float *x, int64_t Q, int k, int metric, float recall_target,
                               float recompute_threshold, int use_precomputed, float initial_search_fraction, int64_t *out_ids,
                               float *out_dist, int32_t *out_nscanned, int mem, qk_timing *timing);

/* ---- k-means ----------------------------------------------------------------------------------- */
/* Nearest-centroid assignment: IndexFlat::search(n, x, 1) (clustering.cpp:63-66) and the
 * batched_scan_list(k=1) of kmeans_refine_partitions (clustering.cpp:149-159).
 * x [n][d], c [m][d]; assign [n] (row index into c, ties -> lower index); val [n] squared L2 / dot (may be NULL). */
QK_API int qk_kmeans_assign(qk_ctx *ctx, const float *x, int64_t n, const float *c, int64_t m, int d, int metric,
                            int64_t *assign, float *val, int mem);
/* Update: per-centroid fp32 sums and counts; sums [m][d], counts [m]; rows with an assignment outside [0, m) are ignored.
 *   qk_kmeans_accumulate          rows added one after the other in ascending row order -- the order of the reference's own
 *                                 accumulate loop in kmeans_refine_partitions (clustering.cpp:162-176: centroid_sums[c][j] += vec[j]),
 *                                 what qk_store_refine_lists uses
 *   qk_kmeans_accumulate_blocked  the mean update of kmeans() (clustering.cpp:51-55 hands it to faiss::Clustering, whose summation
 *                                 order is its back end's): this library's canonical BLOCKED order -- a centroid's rows in ascending
 *                                 row order, sequential fp32 sums over consecutive blocks of 32 rows, the block partials summed
 *                                 sequentially per group of 32 blocks, the group partials summed sequentially (all from +0) -- so
 *                                 that a large cluster is many independent chains; what qk_kmeans uses */
QK_API int qk_kmeans_accumulate(qk_ctx *ctx, const float *x, int64_t n, int d, const int64_t *assign, int64_t m,
                                float *sums, int64_t *counts, int mem);
QK_API int qk_kmeans_accumulate_blocked(qk_ctx *ctx, const float *x, int64_t n, int d, const int64_t *assign, int64_t m,
                                        float *sums, int64_t *counts, int mem);
/* kmeans_refine_partitions() (clustering.cpp:99-182) together with the partition replacement of
 * PartitionManager::refine_partitions (partition_manager.cpp:446-487), applied to the device store: the vectors of the m
 * lists `list_nos` (host array) are re-assigned to the nearest of the m centroids [m][d] (in `mem`; row c = centroid of
 * list_nos[c]) for max(refinement_iterations, 1) passes, centroids recomputed between passes; on return list_nos[c] holds
 * the vectors assigned to centroid c (append order of the reference) and `centroids` the ones used for the last pass.
 * A cluster that holds no row when its centroid is recomputed (possible from the second pass on) would get the centroid 0 / 0:
 * the call then fails with QK_ERR_INVALID and leaves the store and `centroids` as they were. */
QK_API int qk_store_refine_lists(qk_store *s, const int64_t *list_nos, int64_t m, float *centroids, int metric,
                                 int refinement_iterations, int mem);
/* kmeans() (clustering.cpp:13-97): Lloyd iterations on the GPU.  x [n][d] (IP: normalised IN PLACE, as the
 * reference stores the normalised copy, clustering.cpp:25-26,71); centroids [m][d] out; assign [n] out =
 * final full assignment.  seed drives the documented splitmix64 initialisation. */
QK_API int qk_kmeans(qk_ctx *ctx, float *x, int64_t n, int d, int64_t m, int metric, int niter, uint64_t seed,
                     float *centroids, int64_t *assign, int mem);

/* The pieces of kmeans() a multi-GPU build needs between its collectives (local assign + local partial sums,
 * all-reduce of [m][d] sums + [m] counts per iteration; quake_amd/sharded.py):
 *   qk_normalize_rows   x /= ||x|| row by row, canonical norm (clustering.cpp:25-26,59-60), in place
 *   qk_kmeans_update    centroids = sums / counts for non-empty clusters, previous centroid kept for empty ones, then the
 *                       empty-cluster split of faiss::Clustering restated deterministically (largest cluster first, pair
 *                       perturbed by 1 +/- 1/1024); counts are updated by the split
 *   qk_rand_perm        first m entries of the splitmix64 Fisher-Yates permutation of [0, n) (host array out): the
 *                       subsample / initial centroids of qk_kmeans */
QK_API int qk_normalize_rows(qk_ctx *ctx, float *x, int64_t n, int d, int mem);
QK_API int qk_kmeans_update(qk_ctx *ctx, const float *sums, int64_t *counts, int64_t m, int d, float *centroids, int mem);
QK_API int qk_rand_perm(int64_t n, int64_t m, uint64_t seed, int64_t *perm_out_host);
/* Kernel-side durations (HIP events on the context's stream) of the LAST Lloyd iteration of the last qk_kmeans on this context: the
 * assign step (k_assign + its centroid re-tiling) and the update step (bucketing + k_accumulate) over `rows` training rows and `m`
 * centroids -- what a harness prices against the MFMA / HBM roofs (no reference counterpart: faiss::Clustering prints its own
 * per-iteration times under `verbose`, clustering.cpp:41).  Zeros before the first qk_kmeans. */
QK_API int qk_kmeans_last_timing(qk_ctx *ctx, float *assign_ms, float *update_ms, int64_t *rows, int64_t *m);

#ifdef __cplusplus
}
#endif
#endif /* QUAKE_HIP_H */
