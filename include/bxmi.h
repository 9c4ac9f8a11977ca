/*
 * bxmi.h -- C ABI of libbxmi.so, the MI355X (gfx950) engine behind
 *   bx.intervals.intersection.IntervalTree / Intersecter   (insert, find)
 *   bx.bitset.BinnedBitSet                                 (set_range, iand, ior, count_range, ...)
 *
 * Plain C, opaque handles, plain pointers and sizes; no torch / Python types.
 * Every function returns a status (BXMI_OK == 0); bxmi_last_error() gives the
 * text of the last failure on the calling thread.
 *
 * Pointer convention: arguments are HOST pointers unless the function name ends
 * in `_dev`, in which case every array argument is a DEVICE pointer (HBM) and
 * `stream` is a hipStream_t passed as void* (NULL = the null stream).  Host
 * variants stage through the library's own stream and return when the result
 * is in the caller's buffer.
 *
 * Reference interfaces replaced (bx-python 0.14.0, paths under the reference):
 *   src/binBits.h:15-26          the 12 binBits* functions  -> bxmi_bits_*
 *   lib/bx/bitset.pyx:198-241    BinnedBitSet methods        -> call bxmi_bits_*
 *   lib/bx/intervals/intersection.pyx:388-406,428-435
 *                                IntervalTree.insert/find    -> bxmi_ivl_*
 *   scripts/bnMapper.py:83-193   transform, the choice between chains, union_elements -> bxmi_chainmap_*
 *   scripts/aggregate_scores_in_intervals.py:107-134, lib/bx/binned_array.py:72-100
 *                                the per-base loop over a BinnedArray of scores      -> bxmi_scores_*
 *   scripts/bed_bigwig_profile.py:27-41   totals += values; valid += ~isnan per site   -> bxmi_scores_profile*
 *   lib/bx/bbi/bbi_file.pyx:66-111,187-260, bigwig_file.pyx:93-108,176-185
 *                                BigWigFile.summarize_from_full / query over full data -> bxmi_spans_*
 *   lib/bx/bbi/bigwig_file.pyx:122-137,200-211
 *                                BigWigFile.get_as_array, a batch of regions per call   -> bxmi_spans_arrays*
 *   lib/bx/bbi/bbi_file.pyx:296-432, cirtree_file.pyx:5-20,49-105
 *                                ZoomLevel._summarize: summarize / query from a zoom level -> bxmi_zoom_*
 *   lib/bx/bbi/bigbed_file.pyx:57-76,104-113
 *                                BigBedFile.summarize_from_full / query over full data -> bxmi_beds_*
 *   lib/bx/seq/_twobit.pyx:22-137, twobit.py:34-56
 *                                TwoBitSequence.get / __getitem__, a batch of regions per call -> bxmi_twobit_*
 *   lib/bx/motif/_pwm.pyx:23-55, pwm.py:141-149
 *                                ScoringMatrix.score_string over the sequence of a batch of regions -> bxmi_pwm_*, bxmi_twobit_pwm_*
 *   lib/bx/intseq/ngramcount.pyx:34-85, seqmapping.py:36-48, _seqmapping.pyx:24-67
 *                                count_ngrams(mapping.translate(...)) over the sequence of a batch of regions -> bxmi_twobit_kmer_*
 *   lib/bx/seq/seq.py:108-109, DNA_COMP at seq.py:9-14
 *                                SeqFile.reverse_complement: text.translate(DNA_COMP)[::-1] of a row -> bxmi_twobit_*_strand
 *   (intersection.pyx has no C ABI of its own: its cdef classes are the
 *    interface, so the entry points below are what a Cython/ctypes shim of
 *    those classes binds; see INTEGRATION.md.)
 */
#ifndef BXMI_H
#define BXMI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BXMI_OK 0
#define BXMI_EINVAL 1 /* bad argument (NULL handle, negative count, size > 2^31-1, ...) */
#define BXMI_ENOMEM 2 /* host or device allocation failed */
#define BXMI_EHIP 3   /* a HIP runtime call or kernel launch failed */
#define BXMI_ESTATE 4 /* call not valid in the handle's state (e.g. query before seal) */
#define BXMI_ERANGE 5 /* caller's output buffer too small; the needed size is reported */

typedef struct bxmi_ivl bxmi_ivl_t;   /* one interval index == one IntervalTree */
typedef struct bxmi_bits bxmi_bits_t; /* one binned bitset  == one BinnedBitSet */

/* ---- library / device ---------------------------------------------------- */
int bxmi_version(void);
const char *bxmi_last_error(void);
int bxmi_device_count(int *n);
int bxmi_set_device(int device);
int bxmi_get_device(int *device);
int bxmi_device_info(int device, char *name, int name_len, int *compute_units, int64_t *hbm_bytes);
/* Free and total bytes of the current device's memory (hipMemGetInfo): what the host side sizes group launches against
 * (a group makes every member allocate its whole word array).  No reference counterpart. */
int bxmi_mem_info(int64_t *free_bytes, int64_t *total_bytes);
int bxmi_synchronize(void *stream);

/* Raw HBM staging for hosts that do not bring their own allocator. */
int bxmi_malloc(void **dptr, size_t bytes);
int bxmi_free(void *dptr);
int bxmi_memcpy_h2d(void *dst_dev, const void *src_host, size_t bytes);
int bxmi_memcpy_d2h(void *dst_host, const void *src_dev, size_t bytes);
int bxmi_memset(void *dst_dev, int value, size_t bytes);

/* Tuning / A-B knobs (process-wide), key -> value.  Results never depend on them (the GPU tests run both sides).  The
 * authoritative list with the defaults is what bxmi_option_at enumerates (the IVL_OPTS table of csrc/intervals.hip);
 * the ones a caller may want:
 *   ivl.partition      -1 auto (batches >= 4 Mi queries take the large-batch passes), 0 never, 1 always
 *   ivl.sorted_path    1 (default): a batch whose starts are already non-decreasing is answered as it lies
 *   ivl.sorted_cells   1 (default): ... from the cell images, stretch by stretch (count_dense.hpp, bs_*); 0: first-generation kernel
 *   ivl.bitmap         -1 (default): large batches take the exchange (tile sort -> search on unit images -> un-permute)
 *                      when the index qualifies; 0 never (round 1's bucketed pass)
 *   ivl.bitmap_min     smallest batch that takes the exchange (default 2 Mi queries)
 *   ivl.flat / ivl.dense / ivl.slice / ivl.sparse   force (1), forbid (0) or leave to the index's shape (-1, default) the
 *                      search stage: bitmap-cell images / dense unit images / staged key slices / offset-cell images
 *   ivl.bo_cell_log2   offset cells: coordinates per cell (6..8, 0 = from the density)
 *   ivl.bm_variant     tile shape of the exchange (-1 auto, 0 = 512 x 32, 1 = 1024 x 16, 2 = 1024 x 32 queries per tile)
 *   ivl.bd_chunk       queries per search work item (0 = default)
 *   ivl.bd_w8          8-bit counts between the search and the un-permute kernel (-1 auto from the density + feedback)
 *   ivl.order_skip     1 (default): the exact order check is dropped after two shuffled batches (a probe stands in)
 *   ivl.find_sliced    1 (default): find() on large unsorted batches goes through the exchange (count_slices.hpp)
 *   ivl.fx_direct      the exchange's fill writes straight into the CSR list (1) or into scratch, followed by a copy (0); -1 (default):
 *                      straight while the list the handle expects (hits per query of its previous batch) stays under 400 MB
 *   ivl.sl_f, ivl.sl_lanes, ivl.sl_flat, ivl.sl_run_cap   geometry of the slice stage (tests, A/B tools)
 *   ivl.bd_table_from  dense images: duplicated coordinates from which a cell gets a rank table (0 = 2 where the LDS has the room, else 6)
 *   ivl.bm_hard_ppm, ivl.bd_blocks   thresholds / shapes of the unit images (tests)
 *   ivl.host_chunk, ivl.host_touchers   the host-pointer count: queries per chunk of its pipeline (default 8 Mi; 0 = one piece) and
 *                      the host threads that touch an output array's pages ahead of the downloads (default 2; bxmi_ivl_find too)
 *   bits.grid          grid of the per-bitset kernels
 *   core.poll          1 (default): the one-call paths (bxmi_ivl_find_one, short bxmi_bits_count_range) poll a completion
 *                      word their kernel writes to host memory; 0: they wait for the stream
 *   scores.wave_min_len  bxmi_scores_aggregate: intervals with at least this many bases inside the track get a wave each
 *                      (default 8192; 0 = all of them), shorter ones share a wave 64 at a time
 *   scores.profile_chain  bxmi_scores_profile: 0 (default) = a column takes the ordered float64 chain where the parallel sum is
 *                      not provably the same bits; 1 = every column takes it (what exactness costs at most); -1 = no column
 *                      does and the failing ones keep their parallel sums: WRONG ON PURPOSE, for the test that shows the
 *                      chain is what makes the totals right
 * Unknown keys return BXMI_EINVAL. */
int bxmi_set_option(const char *key, int64_t value);
/* The current value of an option, and every option in turn (i = 0, 1, ... until BXMI_EINVAL): what the tests and A/B tools
 * read the defaults from.  (No reference counterpart: bx-python has no tuning knobs.) */
int bxmi_get_option(const char *key, int64_t *value);
int bxmi_option_at(int i, const char **key, int64_t *value);

/* ---- interval index  (intersection.pyx) ---------------------------------- */
/* IntervalTree()                                   intersection.pyx:380-382 */
int bxmi_ivl_create(bxmi_ivl_t **out);
int bxmi_ivl_destroy(bxmi_ivl_t *h);
/* IntervalTree.insert(start, end, value) x n, in insertion order; the payload
 * of interval i is its insertion index (the host keeps the objects).
 * Any int32 pair is accepted, like the reference (start > end, negatives).
 *                                                  intersection.pyx:388-397 */
int bxmi_ivl_append(bxmi_ivl_t *h, const int32_t *start, const int32_t *end, int64_t n);
int bxmi_ivl_append_dev(bxmi_ivl_t *h, const int32_t *start, const int32_t *end, int64_t n, void *stream);
/* Build the device index over everything appended so far: radix sort into the
 * treap's in-order (key start, end<=start first, -i/+i), sorted ends, prefix
 * max of ends, and the 32-ary search levels.  Re-callable after more appends. */
int bxmi_ivl_seal(bxmi_ivl_t *h, void *stream);
int bxmi_ivl_size(const bxmi_ivl_t *h, int64_t *n);
/* 1 if some stored interval has end < start (forces the general count path). */
int bxmi_ivl_has_reversed(const bxmi_ivl_t *h, int *flag);
/* In-order sequence of insertion indices == IntervalTree.traverse order.
 *                                                  intersection.pyx:262-268 */
int bxmi_ivl_order(const bxmi_ivl_t *h, int32_t *idx_out);
int bxmi_ivl_order_dev(const bxmi_ivl_t *h, const int32_t **idx_dev, const int32_t **start_dev, const int32_t **end_dev);

/* len(IntervalTree.find(qs[i], qe[i])) for a batch.  counts (int32[nq]) and
 * total (sum, int64) are each optional (NULL).  Exact for ANY query/target,
 * including zero-length, reversed and negative ones.
 * Host arrays; BLOCKS until counts / total are written.  Batches of >= 2 * ivl.host_chunk (default 2 * 8 Mi) queries go up, through
 * the pass and down in chunks, PCIe busy in both directions: the call starts one host thread for the downloads and
 * ivl.host_touchers (default 2) that touch the pages of `counts` ahead of them, all joined before it returns; `counts` must
 * not be read or written by anyone else meanwhile.  100 M queries: 16 ms (0.8 GB up at 56 GB/s is 14.3) against 32-74 ms in
 * one piece.  Not thread-safe per handle, like every call that takes a bxmi_ivl_t.
 *                                                  intersection.pyx:169-189,400-406 */
int bxmi_ivl_count(bxmi_ivl_t *h, const int32_t *qs, const int32_t *qe, int64_t nq, int32_t *counts, int64_t *total);
/* Device variant: *total_dev (device int64) is ACCUMULATED into (zero it first).  counts = NULL: the total only -- nothing is
 * stored per query.  Stream-ordered, with ONE exception: a handle's FIRST large batch (>= ivl.bitmap_min queries) builds the
 * index's unit images and answers the order probe synchronously -- it waits for `stream` once (and cannot be captured into a
 * hipGraph); every later call only enqueues.  qs, qe and counts must be 16-byte aligned (every allocator's boundary; the passes
 * read and write them 16 bytes per lane): a pointer that is not -- a slice of a device array at an odd offset -- returns
 * BXMI_EINVAL before anything is written (nq == 0 returns BXMI_OK first).  counts = NULL and total_dev = NULL: BXMI_OK, nothing
 * launched. */
int bxmi_ivl_count_dev(bxmi_ivl_t *h, const int32_t *qs, const int32_t *qe, int64_t nq, int32_t *counts,
                       int64_t *total_dev, void *stream);
/* A dict of per-chromosome trees queried in one go (scripts/interval_join.py:21-28 keeps {chrom: Intersecter}; a genome-wide
 * batch asks every tree with its own chromosome's queries): exactly n calls of bxmi_ivl_count_dev -- hs[i] with
 * qs[i][0..nq[i]), counts[i] and totals_dev[i] (each optional / accumulated as there) -- but the indexes that qualify for
 * the bitmap-cell pass share ONE pass: a fixed handful of launches for the whole genome instead of one set per chromosome.
 * The same 16-byte alignment of qs[i], qe[i] and counts[i]: one array that is not aligned refuses the whole call with
 * BXMI_EINVAL before anything is launched. */
int bxmi_ivl_count_multi_dev(bxmi_ivl_t *const *hs, int n, const int32_t *const *qs, const int32_t *const *qe, const int64_t *nq,
                             int32_t *const *counts, int64_t *const *totals_dev, void *stream);
/* Which search stage of the large-batch count pass can serve this sealed index -- the slice search stage (count_slices.hpp: sorted keys staged per unit of 2^f buckets; serves sparse
 * indexes and spans whose bucket image outgrows the LDS): *state = 0 not decided yet, 1 = usable, -1 = one bucket's
 * keys alone do not fit; unit_keys[0..6] = the most keys a unit of 2^f buckets stages.  Introspection only. */
int bxmi_ivl_slice_state(const bxmi_ivl_t *h, int *state, int64_t *unit_keys);
/* The same for the dense-image search stage (count_dense.hpp: one bit per coordinate, units of 2^19 coordinates; serves
 * dense indexes, duplicated coordinates included): *state = 0 not decided yet, 1 = usable, -1 = the index does not fit
 * the format; worst[0] = most keys of one block (the unit, or 2^17 coordinates: limit 32767), worst[1] = most 16-bit
 * overflow entries of one unit (lists of duplicated coordinates and the 129-entry rank tables of clumped cells; limit
 * 32704 with units of 2^18 coordinates).  Introspection only. */
int bxmi_ivl_dense_state(const bxmi_ivl_t *h, int *state, int64_t *worst);
/* The same for the flat walk on cell images (count_dense.hpp, bp_*: the cells of the bitmap pass laid out per unit of
 * 2^18 coordinates, records walked 16 bytes at a time, 16-bit counts): *state = 0 not decided yet, 1 = usable, -1 = the
 * index does not qualify (span wider than 2^29, reversed targets, too many cells with several duplicated coordinates:
 * *hard_cells of them).  This is the stage a dense index takes first.  Introspection only. */
int bxmi_ivl_flat_state(const bxmi_ivl_t *h, int *state, int64_t *hard_cells);
/* The same for the cell images of SPARSE indexes (offset_cells.hpp: a cell of 2^k coordinates, k = 6..8 from the index's
 * density, holds the offsets of up to five keys; units of up to 2^20 coordinates on the same persistent walk, two workgroups per CU): *state = 0
 * not decided yet, 1 = usable, -1 = the index does not qualify (too dense, reversed targets, too many cells with more than
 * five keys: *hard_cells of them); *cell_log2 = k when usable.  A sparse index takes this stage when a batch brings enough
 * queries per unit image (4096), key slices otherwise.  Introspection only. */
int bxmi_ivl_sparse_state(const bxmi_ivl_t *h, int *state, int64_t *hard_cells, int *cell_log2);
/* The width of the counts a flat-walk pass over cell images hands from its search to its un-permute kernel: *bits = 8
 * while the index is sparse enough for small counts (fewer than 128 targets per 2048 coordinates) and fewer than one count
 * in 64 of the passes so far came back as "does not fit" (*wide_counts of them, as last mirrored to the host; such counts
 * are recomputed, the results are exact either way), else 16.  Introspection only. */
int bxmi_ivl_count_width(const bxmi_ivl_t *h, int *bits, int64_t *wide_counts);
/* Whether large count batches on this index currently go without the order check (bm_sorted_check_kernel + the
 * stand-down of the sorted-batch kernel): *skipping = 1 after the checks of two batches in a row found the starts NOT sorted
 * -- a probe of 8192 consecutive starts then rides on every batch, and the first one without a descent brings the check back --
 * *answers_seen = order reports the host has read so far (they arrive through host memory, a pass or more late).
 * Introspection only: a sorted batch met without the check goes through the exchange, with the same counts. */
int bxmi_ivl_order_state(const bxmi_ivl_t *h, int *skipping, int64_t *answers_seen);

/* IntervalTree.find for a batch, as CSR: offsets[nq+1] (int64) and, for query
 * i, hits[offsets[i]..offsets[i+1]) = insertion indices in the reference's
 * result order.  If the hit list needs more than `cap` entries the call
 * returns BXMI_ERANGE with offsets and *total valid and hits untouched.
 * Host arrays; BLOCKS until offsets / hits are written.  From 8 Mi queries (or 16 Mi hits) on, ivl.host_touchers (default 2)
 * host threads touch the pages of `offsets` while the queries go up and the device works, those of `hits` while the
 * offsets come down; they are joined before the call returns.  configs[4] (50 M x 50 M, 250 M hits) into fresh numpy
 * arrays: 39 ms against 67 without them (0.4 GB up + 1.4 GB down at 56 GB/s is 32). */
int bxmi_ivl_find(bxmi_ivl_t *h, const int32_t *qs, const int32_t *qe, int64_t nq, int64_t *offsets,
                  int32_t *hits, int64_t cap, int64_t *total);
/* bxmi_ivl_find_dev: device pointers of any natural alignment (4 bytes for qs / qe / hits, 8 for offsets) are legal; the
 * batch passes need qs, qe and offsets on 16-byte boundaries (what every allocator hands out) and a slice that is not is
 * answered by the direct tree kernels instead -- same results, ~8 x slower.  Blocks until the offsets and the total are
 * known (one stream synchronisation); the hits may still be in flight on `stream` when it returns. */
int bxmi_ivl_find_dev(bxmi_ivl_t *h, const int32_t *qs, const int32_t *qe, int64_t nq, int64_t *offsets,
                      int32_t *hits, int64_t cap, int64_t *total_host, void *stream);

/* IntervalTree.find for ONE query: one launch + one stream sync (the latency path of the per-call
 * drop-in API).  *n_hits = number of hits; BXMI_ERANGE if it exceeds cap. */
int bxmi_ivl_find_one(bxmi_ivl_t *h, int32_t qs, int32_t qe, int32_t *hits, int64_t cap, int64_t *n_hits);

/* IntervalNode.left / right candidate collection for before()/after():
 * dir < 0: reverse in-order, keep 0 <= (position-1) - end   < max_dist
 * dir > 0: in-order,         keep 0 <= start - (position+1) < max_dist
 * Writes up to cap insertion indices; *n_out = number of candidates.
 * An index that holds REVERSED intervals (start > end) reports, for dir < 0, every interval whose end qualifies: the
 * reference prunes by subtree (`minstart > position`), so which of those it reports depends on its treap's random shape;
 * this is the superset of every such run, found by one scan of the candidates above the window's lower end (O(n) for
 * such an index; proper indexes scan the window only).
 *                                                  intersection.pyx:192-260 */
int bxmi_ivl_neighbors(bxmi_ivl_t *h, int32_t position, int32_t max_dist, int dir, int32_t *out, int64_t cap,
                       int64_t *n_out);

/* before()/after() for a whole array of positions: for each i < nq, IntervalNode.left(pos[i], k, max_dist) (dir < 0) or
 * right(pos[i], k, max_dist) (dir > 0) as insertion indices, the reference's "sort, keep n" rule included:
 *   dir > 0: candidates 0 <= start - (pos+1) < max_dist, in in-order; their first min(k, count) (sorted by start already).
 *   dir < 0: candidates 0 <= (pos-1) - end < max_dist, in REVERSE in-order; exactly k of them: that list as it stands
 *            (intersection.pyx:242-245), otherwise the first min(k, count) by end descending, the later in in-order first
 *            among equal ends (a stable sort of the reversed list).
 * pos +/- 1 and the distance window are computed in 64 bits, as bxmi_ivl_neighbors does.  Indexes with reversed intervals
 * take the superset rule of bxmi_ivl_neighbors for dir < 0 (same results, slower).
 * out is an [nq, k] slab: out[i*k .. i*k + n_out[i]) holds the answer, the rest of the row is -1; n_out[i] <= k.
 * n_cand (optional, NULL = not wanted) receives the candidate count before the cut.
 * k outside 1..64 -> BXMI_EINVAL (larger k: bxmi_ivl_neighbors per position); nq above 2^31-1 -> BXMI_EINVAL.
 * Host arrays, natural alignment; BLOCKS until every output is written.
 *                                                  intersection.pyx:192-260 */
int bxmi_ivl_neighbors_batch(bxmi_ivl_t *h, const int32_t *pos, int64_t nq, int32_t k, int32_t max_dist, int dir, int32_t *out,
                             int32_t *n_out, int64_t *n_cand);
/* Device variant: device pointers of natural alignment (4 bytes, 8 for n_cand).  Stream-ordered on `stream`, no host
 * synchronisation; the handle's query scratch is in use until the work completes (one batch per handle at a time). */
int bxmi_ivl_neighbors_batch_dev(bxmi_ivl_t *h, const int32_t *pos, int64_t nq, int32_t k, int32_t max_dist, int dir, int32_t *out,
                                 int32_t *n_out, int64_t *n_cand, void *stream);

/* ClusterTree (lib/bx/intervals/cluster.pyx:57-121, src/cluster.c:112-260): groups of intervals chained by gaps of at
 * most max_dist (>= 0).  All clusters in ascending start order: starts[c], ends[c], and members[offsets[c] ..
 * offsets[c+1]) = the member ids in ascending order, where an interval's id is ids[insertion index] (or the insertion
 * index itself when ids is NULL).  starts/ends/members need n entries, offsets n + 1 (n = bxmi_ivl_size).  The caller
 * applies ClusterTree's min_intervals filter.  max_dist = -1 is accepted when no interval is empty (the reference is
 * deterministic there: tests/golden/cluster_negative_distance.txt); -1 with an empty interval and every max_dist < -1
 * -> BXMI_EINVAL (the reference's result then depends on the insertion order and on unseeded rand() priorities). */
int bxmi_ivl_clusters(bxmi_ivl_t *h, const int32_t *ids, int32_t max_dist, int64_t *n_clusters, int32_t *starts, int32_t *ends,
                      int64_t *offsets, int32_t *members);

/* ---- liftover through chain alignments  (scripts/bnMapper.py) ---------------
 * One bxmi_chainmap_t holds the chains of ONE source chromosome, resident on the device: an interval index over their
 * spans [t_start, t_end) in the order given (bnMapper.py:417-420 inserts them in file order) and their block tables.
 * All coordinates are forward-strand (bnMapper.py:299-305 converts a '-' side in the header); block tables are relative
 * to their chain's start and cumulative (lib/bx/align/epo.py:19-43): chain c owns blocks block_off[c] .. block_off[c+1],
 * block j aligns target [blk_t_start[j], blk_t_end[j]) + t_start[c] with query [blk_q_start[j], blk_q_start[j] + its length),
 * the latter relative to q_start[c] before the strand flip.  q_span[c] = qEnd - qStart (the Sz of bnMapper.py:121),
 * q_minus[c] != 0 = query strand '-'.
 * Empty blocks are legal (chains made from EPO alignments have them).  Refused with BXMI_EINVAL: a chain without blocks,
 * a block of negative length, a block that starts before the one before it ends on either side (a negative gap) or
 * reaches outside its chain's span, t_end - t_start or q_start + q_span beyond 2^31-1, more than 2^31-1 blocks.  (The
 * reference takes such tables and answers by whole-table scans; no chain file has them.) */
typedef struct bxmi_chainmap bxmi_chainmap_t;
int bxmi_chainmap_create(bxmi_chainmap_t **out, int64_t n_chains, const int32_t *t_start, const int32_t *t_end, const int32_t *q_start,
                         const int32_t *q_span, const uint8_t *q_minus, const int64_t *block_off, const int32_t *blk_t_start,
                         const int32_t *blk_t_end, const int32_t *blk_q_start);
int bxmi_chainmap_destroy(bxmi_chainmap_t *m);
/* Each optional (NULL): number of chains, number of blocks, blocks of the longest chain. */
int bxmi_chainmap_info(const bxmi_chainmap_t *m, int64_t *n_chains, int64_t *n_blocks, int64_t *max_chain_blocks);

#define BXMI_LIFT_MAPPED 0  /* rows offsets[i] .. offsets[i+1] hold the result */
#define BXMI_LIFT_NOCHAIN 1 /* no chain met, or every chain met yields nothing (gap region, gap rule)  bnMapper.py:169 */
#define BXMI_LIFT_SPLIT 2   /* more than one chain yields something and select == 0                    bnMapper.py:180 */
#define BXMI_LIFT_BELOW 3   /* (fe - fs) * threshold > mapped bases                                    bnMapper.py:187 */
#define BXMI_LIFT_EMPTY 4   /* the union left nothing                                                  bnMapper.py:193 */
/* transform_by_chrom (bnMapper.py:153-193) for nf features [fs[i], fe[i]) of this chromosome:
 *   max_gap    -g: < 0 = no gap rule; the rule looks at the junctions si .. ei-2 only, as bnMapper.py:102-107 does
 *   select     what to do when several chains yield something: 0 = drop the feature (the default of the script),
 *              1 = the first chain with the strictly largest (last slice's end - first slice's end), the first chain if none
 *                  is positive (-k, bnMapper.py:172-179), 2 = the first chain in find order (the summit lookup, :222-242)
 *   threshold  -t, compared in double arithmetic as the reference does
 * A chain whose span reaches beyond its blocks yields nothing for a feature that meets only that part (the reference
 * raises IndexError there, bnMapper.py:95-96).
 * Out, per feature: chain[i] = the chosen chain (its position in the arrays given to create) or -1, status[i] = BXMI_LIFT_*;
 * offsets[nf + 1] and, for feature i, rows offsets[i] .. offsets[i+1] of out_start / out_end: the unioned slices in query
 * coordinates, ascending (union_elements + sorted, :126-142,192).  *total = offsets[nf].  More rows than `cap`: BXMI_ERANGE
 * with chain, status, offsets and *total valid and out_start / out_end untouched.  Some fs[i] > fe[i]: BXMI_EINVAL, nothing
 * written.  Host arrays; BLOCKS until everything is written. */
int bxmi_chainmap_map(bxmi_chainmap_t *m, const int32_t *fs, const int32_t *fe, int64_t nf, int32_t max_gap, int select, double threshold,
                      int32_t *chain, int32_t *status, int64_t *offsets, int32_t *out_start, int32_t *out_end, int64_t cap,
                      int64_t *total);
/* Device variant: device pointers of natural alignment (4 bytes, 8 for offsets); total_host is a HOST pointer.  Everything is
 * enqueued on `stream`; the call waits for it twice -- inside bxmi_ivl_find_dev for the number of (feature, chain) pairs, and
 * at its end for the row total that decides between BXMI_OK and BXMI_ERANGE (the rows are written by then).  One batch per
 * handle at a time (the handle owns the scratch between the passes). */
int bxmi_chainmap_map_dev(bxmi_chainmap_t *m, const int32_t *fs, const int32_t *fe, int64_t nf, int32_t max_gap, int select,
                          double threshold, int32_t *chain, int32_t *status, int64_t *offsets, int32_t *out_start, int32_t *out_end,
                          int64_t cap, int64_t *total_host, void *stream);

/* ---- binned bitset  (binBits.h:15-26, bitset.pyx:198-241) ----------------- */
/* binBitsAlloc(size, granularity): bin_size and nbins use the reference's
 * float32 arithmetic; size > 2^31-1 or size < 1 -> BXMI_EINVAL.
 * granularity == 0 creates a FLAT set (bitset.pyx:107-173 BitSet over
 * kent/bits.h: no bins, so no ALL_ONE arithmetic). */
int bxmi_bits_create(int64_t size, int64_t granularity, bxmi_bits_t **out);
int bxmi_bits_destroy(bxmi_bits_t *h); /* binBitsFree */
int bxmi_bits_info(const bxmi_bits_t *h, int32_t *size, int32_t *bin_size, int32_t *nbins);
/* Device view: dense LSB-first uint64 words covering [0, nbins*bin_size). */
int bxmi_bits_words_dev(bxmi_bits_t *h, uint64_t **words_dev, int64_t *nwords);
/* Per-bin state as the reference would hold it: 0 = ALL_ZERO, 1 = ALL_ONE, 2 = allocated. */
int bxmi_bits_bin_states(bxmi_bits_t *h, uint8_t *out);

int bxmi_bits_get(bxmi_bits_t *h, int32_t pos, int *bit); /* binBitsReadOne  */
int bxmi_bits_set(bxmi_bits_t *h, int32_t pos);           /* binBitsSetOne   */
int bxmi_bits_clear(bxmi_bits_t *h, int32_t pos);         /* binBitsClearOne */
/* binBitsSetRange x n.  Ranges must satisfy 0 <= start, 0 <= len,
 * start+len <= size (the wrapper raises bitset.pyx's IndexErrors first). */
int bxmi_bits_set_ranges(bxmi_bits_t *h, const int32_t *start, const int32_t *len, int64_t n);
int bxmi_bits_set_ranges_dev(bxmi_bits_t *h, const int32_t *start, const int32_t *len, int64_t n, void *stream);
/* binBitsCountRange x n (including the reference's ALL_ONE-bin arithmetic). */
int bxmi_bits_count_ranges(bxmi_bits_t *h, const int32_t *start, const int32_t *len, int64_t n, int32_t *out);
int bxmi_bits_count_ranges_dev(bxmi_bits_t *h, const int32_t *start, const int32_t *len, int64_t n, int32_t *out,
                               void *stream);
/* binBitsCountRange for one (possibly chromosome-long) range, grid-wide reduction. */
int bxmi_bits_count_range(bxmi_bits_t *h, int32_t start, int32_t len, int32_t *out);
/* binBitsFindSet (val=1) / binBitsFindClear (val=0): first such bit >= start, else size. */
int bxmi_bits_next(bxmi_bits_t *h, int32_t start, int val, int32_t *out);
int bxmi_bits_and(bxmi_bits_t *h, const bxmi_bits_t *other); /* binBitsAnd */
int bxmi_bits_or(bxmi_bits_t *h, const bxmi_bits_t *other);  /* binBitsOr  */
int bxmi_bits_not(bxmi_bits_t *h);                           /* binBitsNot */
int bxmi_bits_xor(bxmi_bits_t *h, const bxmi_bits_t *other); /* bitXor (flat sets only, bits.h:56) */
/* Fused  h &= other  and  popcount(h[0,size))  in one pass over HBM. */
int bxmi_bits_and_count(bxmi_bits_t *h, const bxmi_bits_t *other, int64_t *count);
/* Stream-ordered forms used by the bench (no host sync; *count_dev accumulated). */
int bxmi_bits_and_dev(bxmi_bits_t *h, const bxmi_bits_t *other, void *stream);
int bxmi_bits_or_dev(bxmi_bits_t *h, const bxmi_bits_t *other, void *stream);
int bxmi_bits_and_count_dev(bxmi_bits_t *h, const bxmi_bits_t *other, int64_t *count_dev, void *stream);
int bxmi_bits_popcount_dev(bxmi_bits_t *h, int64_t *count_dev, void *stream);
/* Genome-scale batches: the per-chromosome loops of bed_intersect_basewise.py:25-28
 * (iand) and bed_coverage.py:27-29 (count_range(0, size)) as ONE launch over all
 * members.  counts_dev, when given, is int64[n_members] in HBM and is accumulated
 * into (zero it first): popcount of each member's result inside [0, size). */
typedef struct bxmi_bits_group bxmi_bits_group_t;
int bxmi_bits_group_create(bxmi_bits_t *const *members, int n, bxmi_bits_group_t **out);
int bxmi_bits_group_destroy(bxmi_bits_group_t *g);
int bxmi_bits_group_and_dev(bxmi_bits_group_t *g, const bxmi_bits_group_t *other, int64_t *counts_dev, void *stream);
int bxmi_bits_group_or_dev(bxmi_bits_group_t *g, const bxmi_bits_group_t *other, void *stream);
int bxmi_bits_group_popcount_dev(bxmi_bits_group_t *g, int64_t *counts_dev, void *stream);

/* Maximal runs of set bits inside [from, size), i.e. the pairs the loop
 * start=next_set(end); end=next_clear(start) of bed_intersect_basewise.py:32-38
 * produces.  Writes up to cap pairs; *n_runs = number of runs (BXMI_ERANGE if > cap). */
int bxmi_bits_runs(bxmi_bits_t *h, int32_t from, int32_t *run_start, int32_t *run_end, int64_t cap, int64_t *n_runs);

/* ---- per-base score tracks  (scripts/aggregate_scores_in_intervals.py, lib/bx/binned_array.py) ----------
 * One bxmi_scores_t is the BinnedArray of ONE chromosome as a dense float32 array [0, size) in HBM, size <= 2^31-1; NaN = no
 * score (BinnedArray's default), positions outside [0, size) have none. */
typedef struct bxmi_scores bxmi_scores_t;
int bxmi_scores_create(int64_t size, bxmi_scores_t **out); /* every position NaN */
int bxmi_scores_destroy(bxmi_scores_t *h);
int bxmi_scores_info(const bxmi_scores_t *h, int64_t *size);
/* Device view: float32[*n], *n = size. */
int bxmi_scores_values_dev(bxmi_scores_t *h, float **values_dev, int64_t *n);
/* values[offset .. offset + n) from / into a host array; a window that leaves [0, size) -> BXMI_EINVAL. */
int bxmi_scores_write(bxmi_scores_t *h, int64_t offset, const float *values, int64_t n);
int bxmi_scores_read(bxmi_scores_t *h, int64_t offset, float *out, int64_t n);
/* values[start[i] .. end[i]) = value[i] for i = 0 .. n-1, as if applied in that order: where spans overlap the later one wins
 * (load_scores_wiggle, :61-71, assigns position by position in file order).  Spans are clipped to the track; one that is clipped
 * to nothing, empty or inverted is legal and does nothing.  Spans in ascending order without overlaps -- a wiggle file -- are
 * one launch; every descent or overlap starts another.  Host arrays; BLOCKS until the track is written. */
int bxmi_scores_set_spans(bxmi_scores_t *h, const int32_t *start, const int32_t *end, const float *value, int64_t n);
/* The loop of aggregate_scores_in_intervals.py:110-126 for n intervals [start[i], end[i]).  A base is VALID when its score
 * is not NaN, not +-0 (:115 skips falsy scores) and its bit in `mask_or_null` is clear (as bxmi_bits_get answers; positions at or
 * beyond the mask's size are not masked).  Per interval:
 *   count[i]  the valid bases
 *   sum[i]    their float32 sum IN POSITION ORDER, one rounding per add: bit for bit the reference's `total` (numpy.float32 from
 *             the first add on); +0.0 when count[i] == 0
 *   min[i], max[i]  the smallest / largest valid score; +inf / -inf when count[i] == 0.  (The reference's sentinels -- its
 *             minimum starts as the int 100000000 -- are the caller's: bxmi.scores.format_row.)
 * start >= end gives count 0; negative starts and ends beyond the track are legal.  Because the sum of one interval is a
 * serial chain of adds, an interval costs its length times the add latency however many CUs there are.
 * Host arrays; BLOCKS until the four outputs are written. */
int bxmi_scores_aggregate(bxmi_scores_t *h, const bxmi_bits_t *mask_or_null, const int32_t *start, const int32_t *end, int64_t n,
                          int32_t *count, float *sum, float *min, float *max);
/* Device variant: device pointers of natural alignment (4 bytes).  Stream-ordered on `stream`, no host synchronisation; the
 * handle's list of long intervals is in use until the work completes (one batch per handle at a time).  The mask's words must
 * be complete before the work on `stream` starts (the host forms of bxmi_bits_* return with them written). */
int bxmi_scores_aggregate_dev(bxmi_scores_t *h, const bxmi_bits_t *mask_or_null, const int32_t *start, const int32_t *end, int64_t n,
                              int32_t *count, float *sum, float *min, float *max, void *stream);
/* Site profile (scripts/bed_bigwig_profile.py:27-41): n windows of `width` bases, window i over positions win_start[i] + j
 * (j = 0 .. width-1, computed in int64: any int32 start is legal) of tracks[track_of[i]]; track_of[i] == -1 = no track.  A
 * position outside [0, size) of its track, or a NaN there, has no score (the reference crashes on a negative window start and
 * on an unknown chromosome; here such positions simply have no data).  +-0 IS a score.  Per column j:
 *   totals[j]  float64: +0.0, then += (double)score for i = 0 .. n-1 IN INPUT ORDER, one rounding per add, +0.0 for a missing
 *              score -- bit for bit the reference's `totals`, chromosomes interleaved as the input interleaves them
 *   valid[j]   the windows that have a score at offset j
 * Columns whose parallel sum is provably exact (csrc/profile.hpp; e.g. any realistic batch of three-decimal scores) never
 * run the chain; the others do, and a chain costs n dependent float64 adds however many CUs there are.
 * *chain_columns_or_null = the columns that took the chain.  width < 1, n outside [0, 2^31-1], n_tracks < 0 or a
 * track_of[i] >= n_tracks -> BXMI_EINVAL; n == 0 gives zeros.  All tracks live on the current device.  The pass's scratch
 * belongs to the library: one profile call at a time per process.  Host arrays; BLOCKS until the outputs are written. */
int bxmi_scores_profile(bxmi_scores_t *const *tracks, int32_t n_tracks, const int32_t *track_of, const int32_t *win_start, int64_t n,
                        int32_t width, double *totals, int32_t *valid, int64_t *chain_columns_or_null);
/* Device variant: `tracks` stays a host array of handles; track_of, win_start, totals, valid and chain_columns_or_null are device
 * pointers of natural alignment.  Stream-ordered on `stream`, no host synchronisation; the library's scratch is in use until the
 * work completes.  The entries of track_of cannot be checked without a synchronisation: one outside [0, n_tracks) is no track. */
int bxmi_scores_profile_dev(bxmi_scores_t *const *tracks, int32_t n_tracks, const int32_t *track_of, const int32_t *win_start, int64_t n,
                            int32_t width, double *totals, int32_t *valid, int64_t *chain_columns_or_null, void *stream);

/* ---- span tracks and their binned summaries  (lib/bx/bbi/bbi_file.pyx, bigwig_file.pyx) ----------
 * One bxmi_spans_t is ONE chromosome's bigWig items -- [start[i], end[i]) with value[i] -- in HBM, IN FILE ORDER (the order the
 * reference's block handler meets them; bxmi.bigwig.read_spans_file returns it).  The dense bxmi_scores_t cannot serve summaries:
 * the reference weights each ITEM, by size * (overlap / size) in float64, which is not always the integer overlap.
 * A negative coordinate -> BXMI_EINVAL.  *ordered (bxmi_spans_info) = 1 when starts AND ends are both non-decreasing, as in every
 * real bigWig: the items that overlap a range are then one contiguous run and summaries take the fast path (csrc/summary.hpp);
 * any other track is legal and takes the general path, which walks the whole track for every region. */
typedef struct bxmi_spans bxmi_spans_t;
int bxmi_spans_create(const int32_t *start, const int32_t *end, const float *value, int64_t n, bxmi_spans_t **out);
int bxmi_spans_destroy(bxmi_spans_t *h);
int bxmi_spans_info(const bxmi_spans_t *h, int64_t *n, int *ordered);
/* BigWigFile.summarize_from_full (bbi_file.pyx:80-111, bigwig_file.pyx:176-185) for n regions [start[i], end[i]) of
 * tracks[track_of[i]], `size` bins each.  step = (end - start) / size; bin j = [start + step * j, start + step * (j + 1)); the last
 * (end - start) % size bases belong to no bin; step == 0 leaves every bin empty.  Items are clipped to the region; per bin, over the
 * items that overlap it IN FILE ORDER, with n = the clipped length and w = (double)n * ((double)overlap / n):
 *   valid += w, sum += (double)value * w, sumsq += (double)(value * value) * w  (the square in float32), one rounding per operation,
 *   never fused; max / min take the value where it is larger / smaller (compared in double: a NaN value changes neither);
 *   valid is rounded half to even at the end.  Start values: 0, +inf (min), -inf (max), 0, 0.
 * The five outputs are [n, size] float64 planes, row-major (64-bit offsets: n * size may pass 2^31), bit for bit the reference's
 * valid_count, min_val, max_val, sum_data, sum_squares.  track_of[i] < 0 (unknown chromosome) or start[i] >= end[i] (the
 * reference answers None) is an EMPTY ROW: 0, +inf, -inf, 0, 0 in every bin.  Zoom levels are not involved.
 * size < 1, n outside [0, 2^31-1], n_tracks < 0, a track_of[i] >= n_tracks, a negative start[i] or end[i] -> BXMI_EINVAL; n == 0
 * succeeds without a launch.  All tracks live on the current device.  The track table and the staging belong to the library: one
 * summary call at a time per process.  Host arrays; BLOCKS until the outputs are written. */
int bxmi_spans_summarize(bxmi_spans_t *const *tracks, int32_t n_tracks, const int32_t *track_of, const int32_t *start, const int32_t *end,
                         int64_t n, int32_t size, double *valid, double *min, double *max, double *sum, double *sumsq);
/* Device variant: `tracks` stays a host array of handles; the other arrays are device pointers of natural alignment.  Stream-ordered
 * on `stream`, no host synchronisation.  The entries cannot be checked without a synchronisation: a track_of[i] outside
 * [0, n_tracks) or a negative coordinate gives an empty row. */
int bxmi_spans_summarize_dev(bxmi_spans_t *const *tracks, int32_t n_tracks, const int32_t *track_of, const int32_t *start, const int32_t *end,
                             int64_t n, int32_t size, double *valid, double *min, double *max, double *sum, double *sumsq, void *stream);

/* BigWigFile.get_as_array (bigwig_file.pyx:122-137, 200-211) for a batch of n rows: row i has L_i float32 elements, element j the
 * value of tracks[track_of[i]] at position p = start[i] + j (taken in 64 bits): value[k] of the LARGEST k in file order with
 * start[k] <= p < end[k] -- the reference assigns item after item, so where items overlap the later one wins -- its 32 bits copied
 * unchanged (a NaN value keeps its payload).  The element is NaN, bit pattern 0x7FC00000 as numpy's, where no item covers p, where p
 * is outside [0, 2^31-1), where track_of[i] is outside [0, n_tracks) and where the track is empty.  Zero-length and inverted items
 * cover nothing.  The rows lie one after another in `out`, which has `total` elements:
 *   row_off_or_null == NULL: width >= 1, every row has `width` elements and total must be n * width -- the matrix [n, width];
 *   else: width must be 0, row_off has n + 1 entries and row i is out[row_off[i] .. row_off[i + 1]).  It must start at 0, never
 *   descend and end at `total`, and no row may be longer than 2^31-1: else BXMI_EINVAL, the message naming the condition.
 * n outside [0, 2^31-1], n_tracks < 0, a track_of[i] >= n_tracks -> BXMI_EINVAL (a negative track_of[i] names no track: a NaN row;
 * a negative start[i] is legal).  n == 0 or total == 0 succeeds without a launch.  The work is cut into tiles of the OUTPUT, not
 * into rows (csrc/span_arrays.hpp): rows of one base and rows of millions cost their bases.  An ordered track costs a row's own
 * items; any other track is legal and walks the whole track for every piece of a row.  The table and the staging are those of
 * bxmi_spans_summarize: one summary call of any kind -- these calls included -- at a time per process.  Host arrays; goes through
 * the device in slabs of output and BLOCKS until `out` is written. */
int bxmi_spans_arrays(bxmi_spans_t *const *tracks, int32_t n_tracks, const int32_t *track_of, const int32_t *start, int64_t n, int32_t width,
                      const int64_t *row_off_or_null, int64_t total, float *out);
/* Device variant: `tracks` stays a host array of handles; track_of, start, row_off and out are device pointers of natural
 * alignment.  Where `out` is 16-byte aligned every group of 4 elements is written by one 16-byte store; any other float-aligned
 * `out` is written element by element: the same result, more slowly.  Stream-ordered on `stream`, no host synchronisation.  The
 * entries cannot be checked without one: a track_of[i] outside [0, n_tracks) gives a NaN row, and row_off is the caller's to get
 * right (whatever it holds, nothing outside out[0 .. total) is written and nothing outside the n rows is read; but offsets that
 * do not cover out, such as row_off[n] < total, make every element left over a piece of its own with its own searches: very slow). */
int bxmi_spans_arrays_dev(bxmi_spans_t *const *tracks, int32_t n_tracks, const int32_t *track_of, const int32_t *start, int64_t n, int32_t width,
                          const int64_t *row_off_or_null, int64_t total, float *out, void *stream);

/* ---- zoom tracks and the binned summaries answered from them  (lib/bx/bbi/bbi_file.pyx:296-432) ----------
 * One bxmi_zoom_t is ONE chromosome's part of ONE zoom level of a bigWig file (bxmi.bigwig.read_zoom_file returns it): the n
 * summary records -- [start[i], end[i]) with valid[i], min[i], max[i], sum[i], sumsq[i] -- IN LOAD ORDER, and the level's n_leaves
 * leaf entries for that chromosome: leaf k covers the bases between leaf_lo[k] and leaf_hi[k] as the reference's overlap test sees
 * them (-1: the entry starts on an earlier chromosome; 2^31-1: it ends on a later one) and holds records [leaf_first[k],
 * leaf_first[k + 1]); leaf_first has n_leaves + 1 entries, from 0 to n.  Only an ORDERED level is accepted: record starts and record
 * ends both non-decreasing, start <= end for every record, leaf_lo and leaf_hi both non-decreasing, no negative coordinate (a
 * leaf_lo of -1 apart); anything else -> BXMI_EINVAL, the message naming the condition.  All of it is checked before the first
 * device call. */
typedef struct bxmi_zoom bxmi_zoom_t;
int bxmi_zoom_create(const int32_t *start, const int32_t *end, const uint32_t *valid, const float *min, const float *max, const float *sum,
                     const float *sumsq, int64_t n, const int32_t *leaf_lo, const int32_t *leaf_hi, const int64_t *leaf_first, int64_t n_leaves,
                     bxmi_zoom_t **out);
int bxmi_zoom_destroy(bxmi_zoom_t *h);
int bxmi_zoom_info(const bxmi_zoom_t *h, int64_t *n, int64_t *n_leaves);
/* ZoomLevel._summarize (bbi_file.pyx:355-432) for n regions [start[i], end[i]) of tracks[track_of[i]], `size` bins each; the bins
 * are those of bxmi_spans_summarize.  A region loads the records of every leaf with start < leaf_hi and end > leaf_lo, in order.
 * Per bin [b0, b1): the records at the front of that list that end at or before b0 are passed over; if none is left the bin is
 * valid = sum = sumsq = 0, min = max = NaN; else min and max start from the front record's (whether or not it overlaps the bin)
 * and the records are walked until one starts at or after b1, each with overlap > 0 adding
 *   f = (float)((double)overlap / (end - start));  valid = (float)((double)valid + (double)rec.valid * (double)f), sum and sumsq
 * likewise -- float accumulators, every product and sum rounded in double first, never fused -- and widening max / min (a NaN
 * changes neither).  The five outputs are [n, size] float64 planes as for bxmi_spans_summarize, bit for bit the reference's;
 * valid is NOT rounded to an integer.  track_of[i] < 0 or start[i] >= end[i] (the reference answers None) is the same EMPTY ROW:
 * 0, +inf, -inf, 0, 0.  Arguments, errors, n == 0, the library's table and staging: as bxmi_spans_summarize, with which these
 * calls share them -- one summary call of either kind at a time per process.  Host arrays; BLOCKS until the outputs are written. */
int bxmi_zoom_summarize(bxmi_zoom_t *const *tracks, int32_t n_tracks, const int32_t *track_of, const int32_t *start, const int32_t *end,
                        int64_t n, int32_t size, double *valid, double *min, double *max, double *sum, double *sumsq);
/* Device variant, as bxmi_spans_summarize_dev. */
int bxmi_zoom_summarize_dev(bxmi_zoom_t *const *tracks, int32_t n_tracks, const int32_t *track_of, const int32_t *start, const int32_t *end,
                            int64_t n, int32_t size, double *valid, double *min, double *max, double *sum, double *sumsq, void *stream);

/* ---- bed tracks and their coverage summaries  (lib/bx/bbi/bigbed_file.pyx) ----------
 * One bxmi_beds_t is ONE chromosome's bigBed records -- [start[i], end[i]) -- in HBM, IN FILE ORDER (bxmi.bigbed.read_items_file
 * returns it).  There is no value array: the reference accumulates every record with the value 1.  bigBed records are sorted by
 * start and their ends descend wherever features nest or overlap; creation also builds, on the host, the running maxima of the
 * ends that the kernel searches and skips by (csrc/bed_summary.hpp).  A negative coordinate -> BXMI_EINVAL.  *sorted
 * (bxmi_beds_info) = 1 when the starts never descend, as in every real bigBed: a region then costs its own records plus one test
 * per chunk of records between the first record that reaches it and them; any other track is legal and takes a general walk over
 * the whole track for every region. */
typedef struct bxmi_beds bxmi_beds_t;
int bxmi_beds_create(const int32_t *start, const int32_t *end, int64_t n, bxmi_beds_t **out);
int bxmi_beds_destroy(bxmi_beds_t *h);
int bxmi_beds_info(const bxmi_beds_t *h, int64_t *n, int *sorted);
/* BigBedFile.summarize_from_full (bigbed_file.pyx:104-113) for n regions [start[i], end[i]) of tracks[track_of[i]], `size` bins each:
 * bxmi_spans_summarize over the same records with every value 1.  The bins, the clipping and the weight w are those of
 * bxmi_spans_summarize; per bin, over the records that overlap it IN FILE ORDER, acc += w in float64, one rounding per operation;
 * then valid = acc rounded half to even, sum = sumsq = acc, min = max = 1 where a record overlaps the bin, else +inf and -inf.
 * The five outputs are [n, size] float64 planes, bit for bit the reference's.  Empty rows, arguments, errors, n == 0, the
 * library's table and staging: as bxmi_spans_summarize, with which these calls share them -- one summary call of any kind at a
 * time per process.  Host arrays; BLOCKS until the outputs are written. */
int bxmi_beds_summarize(bxmi_beds_t *const *tracks, int32_t n_tracks, const int32_t *track_of, const int32_t *start, const int32_t *end,
                        int64_t n, int32_t size, double *valid, double *min, double *max, double *sum, double *sumsq);
/* Device variant, as bxmi_spans_summarize_dev. */
int bxmi_beds_summarize_dev(bxmi_beds_t *const *tracks, int32_t n_tracks, const int32_t *track_of, const int32_t *start, const int32_t *end,
                            int64_t n, int32_t size, double *valid, double *min, double *max, double *sum, double *sumsq, void *stream);

/* ---- 2bit tracks: the sequence under batches of rows and its base counts  (lib/bx/seq/twobit.py, _twobit.pyx) ----------
 * One bxmi_twobit_t is ONE sequence of a .2bit file in HBM (bxmi.twobit.read_file returns its arrays): `size` bases packed 4 to a
 * byte, the first base in the two most significant bits, codes T=0 C=1 A=2 G=3; n_blocks N blocks [n_start[i], n_start[i] +
 * n_size[i]) and m_blocks mask blocks likewise.  _create accepts only what every real file holds and refuses anything else with
 * BXMI_EINVAL, the message naming the condition, before the first device call: 0 <= size <= 2^31-1 and, within each list, blocks
 * sorted, non-empty, disjoint and inside [0, size].  Under those conditions the reference's bisect-and-walk over the blocks
 * (_twobit.pyx:100-133: it starts one block before the first that starts after the region and stops at the first that starts past
 * it) is plain coverage -- a position is N, or masked, exactly where a block covers it -- and that is why the condition is there:
 * with overlapping or unsorted blocks the walk can miss a block that covers the region, which no kernel should imitate.
 * Creation also builds, on the device, the running code counts per checkpoint block of 1024 bases and under the N blocks that
 * bxmi_twobit_composition answers from (csrc/twobit.hpp). */
typedef struct bxmi_twobit bxmi_twobit_t;
int bxmi_twobit_create(const uint8_t *packed, int64_t size, const int32_t *n_start, const int32_t *n_size, int64_t n_blocks,
                       const int32_t *m_start, const int32_t *m_size, int64_t m_blocks, bxmi_twobit_t **out);
/* A track from its LETTERS, built on the device (csrc/twobit_build.hpp): what the reference reads through the same SeqFile.get as
 * 2bit -- FASTA (lib/bx/seq/fasta.py) and nib (nib.py, _nib.pyx) -- and letters that are already in HBM.  `size` symbols: ASCII
 * bytes (_letters), or nib nibbles, (size + 1) / 2 bytes, the first symbol of a byte in its high half, codes 0-3 = T C A G, 4 = N,
 * 5-7 = the reference's 'X', bit 3 = lower case (_nib).  The track holds what a .2bit file of the same sequence holds: the N blocks
 * are the MAXIMAL runs of N / n, the mask blocks the maximal runs of lower case (an n lies in both), the packed code is 0 under N
 * and the bits after the last base are 0; the results are the same on every run.  A symbol that is none of TCAGNtcagn (nib codes
 * 5-7) is "other": with other == BXMI_TB_OTHER_REFUSE the call returns BXMI_EINVAL, the message naming the LOWEST such position
 * and its value, *out stays NULL and nothing is kept; with BXMI_TB_OTHER_N it becomes N, masked too if it is lower case (ASCII
 * a-z, the nib's bit 3).  Refused with BXMI_EINVAL before the first device call: out == NULL, `other` neither of the two, size
 * outside [0, 2^31-1], a NULL input with size > 0.  size == 0 makes a valid empty track.
 * The host forms upload the WHOLE input into a temporary device buffer of its size (freed on return) and block.  The _dev form
 * takes `letters` on the device (any alignment; 16-byte aligned it is read by 16-byte loads), reads none of it on the host, queues
 * its kernels on `stream`, synchronises that stream once in the middle to read the two block counts (and the refused position), and
 * RETURNS AFTER SYNCHRONISING IT: the track is complete and `letters` may be changed or freed. */
#define BXMI_TB_OTHER_REFUSE 0
#define BXMI_TB_OTHER_N 1
int bxmi_twobit_create_letters(const uint8_t *letters, int64_t size, int32_t other, bxmi_twobit_t **out);
int bxmi_twobit_create_letters_dev(const uint8_t *letters, int64_t size, int32_t other, bxmi_twobit_t **out, void *stream);
int bxmi_twobit_create_nib(const uint8_t *nibbles, int64_t size, int32_t other, bxmi_twobit_t **out);
/* The file-order arrays of a track, copied back: packed[(size + 3) / 4], the N blocks and the mask blocks as starts and sizes (the
 * counts from bxmi_twobit_info).  Any pointer may be NULL.  For a track from bxmi_twobit_create they are its inputs, for a built one
 * the derived arrays.  Blocks. */
int bxmi_twobit_arrays(const bxmi_twobit_t *h, uint8_t *packed, int32_t *n_start, int32_t *n_size, int32_t *m_start, int32_t *m_size);
int bxmi_twobit_destroy(bxmi_twobit_t *h);
int bxmi_twobit_info(const bxmi_twobit_t *h, int64_t *size, int64_t *n_blocks, int64_t *m_blocks);
/* _twobit.read for a batch of n rows, the contract of bxmi_spans_arrays with bytes for floats: element j of row i is position p =
 * start[i] + j (taken in 64 bits) of tracks[track_of[i]] and holds the ASCII letter the reference's string has there: "TCAG" by
 * code, 'N' inside an N block, lower case inside a mask block when do_mask != 0 (so 'n' inside both).  It holds the byte `pad`
 * (0 .. 255) where p is outside [0, size) and where track_of[i] is outside [0, n_tracks).  Matrix form (row_off_or_null == NULL,
 * width >= 1, total == n * width) and ragged form (width == 0, row_off[n + 1] from 0 to total, never descending, no row longer than
 * 2^31-1), the argument errors, n == 0 and total == 0: exactly as bxmi_spans_arrays.  The work is cut into tiles of the OUTPUT:
 * rows of one base and rows of a whole chromosome cost their bases.  The track table and the staging belong to the library: one
 * 2bit call (bases or composition) at a time per process; the summaries' calls are not involved.  Host arrays; goes through the
 * device in slabs of output and BLOCKS until `out` is written. */
int bxmi_twobit_bases(bxmi_twobit_t *const *tracks, int32_t n_tracks, const int32_t *track_of, const int32_t *start, int64_t n, int32_t width,
                      const int64_t *row_off_or_null, int64_t total, int do_mask, int pad, uint8_t *out);
/* Device variant: `tracks` stays a host array of handles; track_of, start, row_off and out are device pointers.  Where `out` is
 * 16-byte aligned every full group of 16 bytes is written by one 16-byte store; any other `out` gives the same bytes, more slowly.
 * Stream-ordered on `stream`, no host synchronisation.  Unchecked entries as bxmi_spans_arrays_dev: a track_of[i] outside
 * [0, n_tracks) gives a row of `pad`; whatever row_off holds, nothing outside out[0 .. total) is written. */
int bxmi_twobit_bases_dev(bxmi_twobit_t *const *tracks, int32_t n_tracks, const int32_t *track_of, const int32_t *start, int64_t n, int32_t width,
                          const int64_t *row_off_or_null, int64_t total, int do_mask, int pad, uint8_t *out, void *stream);
/* Base counts of n rows: counts is [n, 6] int32 = A, C, G, T, N, masked of [start[i], end[i]) clipped to [0, size) of
 * tracks[track_of[i]].  N = the bases inside N blocks; A, C, G, T = the bases by code OUTSIDE N blocks (a file may pack anything
 * under an N); masked = the bases inside mask blocks, 0 when do_mask == 0: what counting the characters of the reference's string
 * gives, case folded for the first five, the lower-case ones for the sixth.  track_of[i] outside [0, n_tracks) (the host form
 * refuses one >= n_tracks) or an empty row gives six zeros.  A row costs two searches per list of blocks, two 16-byte checkpoint
 * loads and a few edge pieces of at most 256 packed bytes, WHATEVER ITS LENGTH.  n outside [0, 2^31-1], n_tracks < 0 ->
 * BXMI_EINVAL; n == 0 succeeds without a launch.  Table, staging and the one-call-at-a-time rule: as bxmi_twobit_bases. */
int bxmi_twobit_composition(bxmi_twobit_t *const *tracks, int32_t n_tracks, const int32_t *track_of, const int32_t *start, const int32_t *end,
                            int64_t n, int do_mask, int32_t *counts);
/* Device variant: device pointers of natural alignment, stream-ordered on `stream`, no host synchronisation. */
int bxmi_twobit_composition_dev(bxmi_twobit_t *const *tracks, int32_t n_tracks, const int32_t *track_of, const int32_t *start, const int32_t *end,
                                int64_t n, int do_mask, int32_t *counts, void *stream);

/* ---- position weight matrices scored over 2bit rows  (lib/bx/motif/pwm.py:141-149, _pwm.pyx:23-55) ------------------------
 * One bxmi_pwm_t is a set of n_mats matrices over ONE alphabet of n_cols columns, in HBM: `values` is float32 [mat_off[n_mats]]
 * [n_cols], matrix m its rows [mat_off[m], mat_off[m + 1]) (widths may differ); letter_col[10] gives, for the ten letters a 2bit
 * string can hold, in the order T C A G N t c a g n, the column of that letter or -1 (the reference's char_to_index at those ten
 * characters).  _create refuses with BXMI_EINVAL, naming the condition, before any device call: n_mats outside [1, 32], n_cols
 * outside [1, 16], a width outside [1, 256], mat_off[0] != 0, mat_off descending, a letter_col entry outside [-1, n_cols), NULLs.
 * The values are taken as they are: -inf entries are legitimate and exact. */
typedef struct bxmi_pwm bxmi_pwm_t;
int bxmi_pwm_create(const float *values, const int32_t *mat_off, int32_t n_mats, int32_t n_cols, const int8_t *letter_col, bxmi_pwm_t **out);
int bxmi_pwm_destroy(bxmi_pwm_t *h);
int bxmi_pwm_info(const bxmi_pwm_t *h, int32_t *n_mats, int32_t *n_cols, int32_t *max_width);
/* score_string for a batch of n rows described exactly as for bxmi_twobit_bases (matrix form: width >= 1, row_off NULL, total ==
 * n * width; ragged form: width == 0 and row_off[n + 1]); `out` is float32 [n_mats][total].  Row i is the string of the letters
 * bxmi_twobit_bases gives (TCAG by code, 'N' in an N block, lower case in a mask block when do_mask != 0); element j of row i of
 * plane m is ((0.0f + v[0][c(j)]) + v[1][c(j + 1)]) + ... + v[W - 1][c(j + W - 1)], float32 additions in that order, bit for bit
 * the reference's, when all W letters have a column and lie in the row; every other element -- the last W - 1 of a row, all of a
 * row shorter than W, windows over a letter without a column, over a position outside [0, size), rows that name no track -- is
 * the float32 NaN 0x7FC00000 (numpy's nan).  A NaN that the arithmetic itself produces (inf - inf, a NaN entry) is a NaN of
 * unspecified sign and payload.  Refused with BXMI_EINVAL before any device call: everything bxmi_twobit_bases refuses about the
 * rows (there is no pad), a NULL matrix set, total * n_mats beyond what the output index holds.  These calls use the track table
 * and the scratch of the 2bit calls: one 2bit call (bases, composition, pwm) at a time per process.  Host arrays; goes through
 * the device in slabs of output and BLOCKS until `out` is written. */
int bxmi_twobit_pwm_scores(bxmi_twobit_t *const *tracks, int32_t n_tracks, const int32_t *track_of, const int32_t *start, int64_t n, int32_t width,
                           const int64_t *row_off_or_null, int64_t total, int do_mask, const bxmi_pwm_t *pwm, float *out);
/* Device variant: `tracks` and `pwm` stay host handles; track_of, start, row_off and out are device pointers.  A thread's four
 * elements of a plane are written by one 16-byte store where their address is 16-byte aligned, else element by element, with the
 * same result (total % 4 != 0 misaligns the planes after the first).  Nothing outside out[0 .. n_mats * total) is written.
 * Stream-ordered on `stream`, no host synchronisation; unchecked entries as bxmi_twobit_bases_dev. */
int bxmi_twobit_pwm_scores_dev(bxmi_twobit_t *const *tracks, int32_t n_tracks, const int32_t *track_of, const int32_t *start, int64_t n, int32_t width,
                               const int64_t *row_off_or_null, int64_t total, int do_mask, const bxmi_pwm_t *pwm, float *out, void *stream);
/* The best hit per row, no per-base output: best_score float32 [n_mats][n] is the greatest score of the row's elements that are
 * not NaN (a NaN is never a candidate), best_pos int32 [n_mats][n] the FIRST offset within the row that holds it; a row with no
 * scored element gives NaN (0x7FC00000) and -1.  Rows, refusals (but for the one about the output index: there are no planes)
 * and the one-call-at-a-time rule as bxmi_twobit_pwm_scores.  The device variant reads where the rows end from row_off[n] itself:
 * in its ragged form `total` may be any bound >= row_off[n], so a caller whose offsets were computed on the device need not wait
 * for them.  A row's cost is its bases, whatever its length. */
int bxmi_twobit_pwm_best(bxmi_twobit_t *const *tracks, int32_t n_tracks, const int32_t *track_of, const int32_t *start, int64_t n, int32_t width,
                         const int64_t *row_off_or_null, int64_t total, int do_mask, const bxmi_pwm_t *pwm, float *best_score, int32_t *best_pos);
int bxmi_twobit_pwm_best_dev(bxmi_twobit_t *const *tracks, int32_t n_tracks, const int32_t *track_of, const int32_t *start, int64_t n, int32_t width,
                             const int64_t *row_off_or_null, int64_t total, int do_mask, const bxmi_pwm_t *pwm, float *best_score, int32_t *best_pos,
                             void *stream);
/* The hits of a scan: every element of the planes of bxmi_twobit_pwm_scores that is scored, whose score is not a NaN and is >=
 * threshold[m] (float32 comparison; m its matrix), as one compact list -- the planes themselves are never written.  In the
 * reference's terms, numpy.nonzero(pwms[m].score_string(row i) >= threshold[m]) and the scores there.  An unscoreable element and
 * an arithmetic NaN are never hits; a -inf score is a hit only under a -inf threshold.  hit_row int32 (the row), hit_pos int32
 * (the offset within the row, as best_pos) and hit_score float32 (bit for bit the plane's element) are parallel arrays holding
 * all hits in ascending (matrix, row, offset), the same on every run; matrix m's hits are [mat_hits[m], mat_hits[m + 1]) of
 * them, mat_hits int64 [n_mats + 1], mat_hits[0] == 0.  threshold[n_mats] and mat_hits are HOST arrays in both forms.  Rows as
 * for bxmi_twobit_pwm_scores, `total` exact.  The hit arrays hold `cap` entries: with mat_hits[n_mats] > cap the call returns
 * BXMI_ERANGE with mat_hits valid and the hit arrays untouched (the contract of bxmi_ivl_find); cap == 0 with NULL hit arrays
 * asks for the counts alone.  n == 0 or total == 0: no launch, mat_hits all zero.  Refused with BXMI_EINVAL, naming the
 * condition, before any device call: everything bxmi_twobit_pwm_scores refuses about the rows (n above 2^31-1 among it: hit_row
 * is int32), NULL threshold, NULL mat_hits, cap < 0, a NULL hit array with cap > 0, a NULL matrix set, a NaN threshold (its
 * index is named), total * n_mats beyond what the hit index holds.  The work is two scoring passes, one that counts per (matrix,
 * tile of 1024 elements) and one that places; the scratch is 12 bytes per (matrix, tile).  Table, scratch and rule of the other
 * 2bit calls: bases, composition, pwm scores, best hits and these hits, one at a time per process.  Host arrays; BLOCKS until
 * everything is written. */
int bxmi_twobit_pwm_hits(bxmi_twobit_t *const *tracks, int32_t n_tracks, const int32_t *track_of, const int32_t *start, int64_t n, int32_t width,
                         const int64_t *row_off_or_null, int64_t total, int do_mask, const bxmi_pwm_t *pwm, const float *threshold, int64_t cap,
                         int64_t *mat_hits, int32_t *hit_row, int32_t *hit_pos, float *hit_score);
/* Device variant: track_of, start, row_off and the three hit arrays are device pointers; threshold and mat_hits stay host arrays.
 * It BLOCKS once, on `stream`, until the counts are known (as bxmi_ivl_find_dev); the hits are then queued on `stream` and may
 * still be in flight when it returns.  Nothing outside [0, mat_hits[n_mats]) of the hit arrays is written. */
int bxmi_twobit_pwm_hits_dev(bxmi_twobit_t *const *tracks, int32_t n_tracks, const int32_t *track_of, const int32_t *start, int64_t n, int32_t width,
                             const int64_t *row_off_or_null, int64_t total, int do_mask, const bxmi_pwm_t *pwm, const float *threshold, int64_t cap,
                             int64_t *mat_hits, int32_t *hit_row, int32_t *hit_pos, float *hit_score, void *stream);

/* ---- k-mer counts over 2bit rows  (lib/bx/intseq/ngramcount.pyx:34-85 over lib/bx/seqmapping.py:36-48, _seqmapping.pyx:24-67) ----
 * The reference's count_ngrams(mapping.translate(twobit[chrom].get(s, e)), k, radix) for a batch of n rows described exactly as
 * for bxmi_twobit_pwm_best (matrix form: width >= 1, row_off NULL, total == n * width; ragged form: width == 0 and row_off[n + 1];
 * track_of, start, do_mask).  Row i is the string of the letters bxmi_twobit_bases gives.  `digits` is int8[8], indexed by
 * 4 * lower_case + code with codes T=0, C=1, A=2, G=3: the digit of that letter in [0, radix), or -1 for no digit; several letters
 * may share a digit (purine/pyrimidine words are radix 2).  'N', positions outside [0, size) and rows that name no track have no
 * digit; with do_mask == 0 nothing is lower case.  2 <= radix <= 4, k >= 1, bins = radix^k <= 16384 (KM_BINS_MAX of csrc/kmer.hpp:
 * k = 7 at radix 4, k = 14 at radix 2).  The window at offset j of row i counts if and only if all k letters j .. j + k - 1 lie in
 * the row and have a digit; its index is sum(digit[j + t] * radix^t for t in 0 .. k - 1), the first letter least significant
 * (ngramcount.pyx:73-82).  `counts` is int32 [n][bins], written whole whatever it held.  EVERY window of a row is counted, the
 * last one included; the reference's loop stops one window early (`for i from 0 <= i < (n_ints - n)`, ngramcount.pyx:71), which is
 * reproduced by the caller shortening every row by one base (bxmi.kmers: drop_last=True), not here.  Integer work: the counts are
 * the reference's bit for bit.  Refused with BXMI_EINVAL, naming the condition, before any device call: everything
 * bxmi_twobit_pwm_best refuses about the rows; k < 1; radix outside [2, 4]; bins above 16384; a digit outside [-1, radix); NULL
 * digits, NULL counts with n > 0; n * bins beyond what the output index holds.  n == 0 succeeds without a launch.  These calls use
 * the track table and the scratch of the 2bit calls: one 2bit call (bases, composition, pwm, kmer) at a time per process.  Host
 * arrays; goes through the device in slabs of rows and BLOCKS until `counts` is written. */
int bxmi_twobit_kmer_counts(bxmi_twobit_t *const *tracks, int32_t n_tracks, const int32_t *track_of, const int32_t *start, int64_t n, int32_t width,
                            const int64_t *row_off_or_null, int64_t total, int do_mask, int k, int radix, const int8_t *digits, int32_t *counts);
/* Device variant: `tracks` stay host handles and `digits` a host array; track_of, start, row_off and counts are device pointers.
 * `counts` is zeroed and filled on `stream`: stream-ordered, no host synchronisation.  It reads where the rows end from
 * row_off[n] itself: in its ragged form `total` may be any bound >= row_off[n], as for bxmi_twobit_pwm_best_dev.  Unchecked
 * entries as bxmi_twobit_bases_dev.  A row's cost is its bases, whatever its length. */
int bxmi_twobit_kmer_counts_dev(bxmi_twobit_t *const *tracks, int32_t n_tracks, const int32_t *track_of, const int32_t *start, int64_t n, int32_t width,
                                const int64_t *row_off_or_null, int64_t total, int do_mask, int k, int radix, const int8_t *digits, int32_t *counts,
                                void *stream);
/* For measurements and tests: how the calls after this one accumulate, whatever csrc/kmer.hpp's km_use_lds would choose -- 0 its
 * choice (the default), 1 the LDS histogram wherever bins allow it, 2 straight to HBM.  The counts are the same. */
int bxmi_twobit_kmer_force(int way);

/* ---- strand-aware 2bit rows  (lib/bx/seq/seq.py:108-109: reverse_complement = text.translate(DNA_COMP)[::-1], seq.py:9-14) ----
 * Each call is its unstranded sibling with `strand_or_null` after `start`: int8 [n], 0 = the row as stored (plus), 1 = its reverse
 * complement (minus).  NULL means all plus and gives exactly what the sibling gives.  For a minus row i of len elements (matrix
 * form: width; ragged form: row_off[i + 1] - row_off[i]):
 *   letters   element j is taken at position p = start[i] + (len - 1 - j), in 64 bits.  Where p is in [0, size) of a named track it
 *             is the COMPLEMENT of the letter the plus call writes for p: A<->T, C<->G, a<->t, c<->g, N->N, n->n (the case follows
 *             the base; the code is complemented: T=0 C=1 A=2 G=3, code ^ 2).  Elsewhere it is `pad`, untouched: pad is never
 *             complemented, even if it is a letter.  So a minus row is the plus row reversed and complemented, the pad mirrored.
 *   counts    A, C, G, T of a minus row are T, G, C, A of the plus row; N and masked are unchanged.
 *   k-mers    the row's string is the one the stranded letters call gives; everything else of bxmi_twobit_kmer_counts holds as
 *             written (EVERY window, the first letter least significant, any digits[8]: the table need not be closed under
 *             complement).  A caller that reproduces the reference's loop (drop_last) drops the last window of the STRAND's string,
 *             that is, shortens a minus row at its start: start + 1, one element fewer.
 * Every refusal of the sibling applies unchanged.  The host forms also refuse, with BXMI_EINVAL naming the row, before any device
 * call and with the output untouched, a strand entry other than 0 or 1.  The device forms take `strand_or_null` as a device pointer
 * and do not check it, like track_of: ANY NON-ZERO ENTRY IS MINUS.  Track table, scratch, slabs and the one-call-at-a-time rule:
 * as the siblings.
 *   pwm       (bxmi_twobit_pwm_scores_strand, _best_strand, _hits_strand and their _dev forms; the reference's
 *             matrix.score_string(reverse_complement(text)), lib/bx/motif/pwm.py:141-149 over _pwm.pyx:23-55.)  The string of a minus
 *             row is the one the stranded letters call gives with no pad: letter k is the complement (code ^ 2; the case is kept, N
 *             stays N) of the letter at p = start[i] + (len - 1 - k), p in 64 bits; a p outside [0, size) has no column, and neither
 *             has any position of a row that names no track.  Everything of the three pwm contracts above holds AS WRITTEN, ON
 *             THAT STRING: element j of plane m is ((0.0f + v[0][c(j)]) + v[1][c(j + 1)]) + ... + v[W - 1][c(j + W - 1)] in ascending
 *             matrix row, c the column of the strand string's letter -- letter_col is applied to the COMPLEMENTED letter, and the
 *             alphabet need not be closed under complement; NaN 0x7FC00000 where a letter has no column or the window passes the
 *             string's end: the last W - 1 elements of the strand's string, which are the FIRST W - 1 genomic positions of the
 *             row.  best_pos and hit_pos are offsets in the strand's string -- the genomic start of the site is start + len - W -
 *             pos; the best hit is the greatest score at its FIRST offset in the strand's string; hits come in ascending (matrix,
 *             row, offset in the strand's string).  This is NOT the reverse-complement matrix on the plus string mirrored: that
 *             adds the same terms in descending matrix row, which float32 does not round alike. */
int bxmi_twobit_bases_strand(bxmi_twobit_t *const *tracks, int32_t n_tracks, const int32_t *track_of, const int32_t *start,
                             const int8_t *strand_or_null, int64_t n, int32_t width,
                      const int64_t *row_off_or_null, int64_t total, int do_mask, int pad, uint8_t *out);
int bxmi_twobit_bases_strand_dev(bxmi_twobit_t *const *tracks, int32_t n_tracks, const int32_t *track_of, const int32_t *start,
                                 const int8_t *strand_or_null, int64_t n, int32_t width,
                          const int64_t *row_off_or_null, int64_t total, int do_mask, int pad, uint8_t *out, void *stream);
int bxmi_twobit_composition_strand(bxmi_twobit_t *const *tracks, int32_t n_tracks, const int32_t *track_of, const int32_t *start,
                                   const int8_t *strand_or_null, const int32_t *end,
                            int64_t n, int do_mask, int32_t *counts);
int bxmi_twobit_composition_strand_dev(bxmi_twobit_t *const *tracks, int32_t n_tracks, const int32_t *track_of, const int32_t *start,
                                       const int8_t *strand_or_null, const int32_t *end,
                                int64_t n, int do_mask, int32_t *counts, void *stream);
int bxmi_twobit_kmer_counts_strand(bxmi_twobit_t *const *tracks, int32_t n_tracks, const int32_t *track_of, const int32_t *start,
                                   const int8_t *strand_or_null, int64_t n, int32_t width,
                            const int64_t *row_off_or_null, int64_t total, int do_mask, int k, int radix, const int8_t *digits, int32_t *counts);
int bxmi_twobit_kmer_counts_strand_dev(bxmi_twobit_t *const *tracks, int32_t n_tracks, const int32_t *track_of, const int32_t *start,
                                       const int8_t *strand_or_null, int64_t n, int32_t width,
                                const int64_t *row_off_or_null, int64_t total, int do_mask, int k, int radix, const int8_t *digits, int32_t *counts,
                                void *stream);
int bxmi_twobit_pwm_scores_strand(bxmi_twobit_t *const *tracks, int32_t n_tracks, const int32_t *track_of, const int32_t *start,
                                  const int8_t *strand_or_null, int64_t n, int32_t width,
                           const int64_t *row_off_or_null, int64_t total, int do_mask, const bxmi_pwm_t *pwm, float *out);
int bxmi_twobit_pwm_scores_strand_dev(bxmi_twobit_t *const *tracks, int32_t n_tracks, const int32_t *track_of, const int32_t *start,
                                      const int8_t *strand_or_null, int64_t n, int32_t width,
                               const int64_t *row_off_or_null, int64_t total, int do_mask, const bxmi_pwm_t *pwm, float *out, void *stream);
int bxmi_twobit_pwm_best_strand(bxmi_twobit_t *const *tracks, int32_t n_tracks, const int32_t *track_of, const int32_t *start,
                                const int8_t *strand_or_null, int64_t n, int32_t width,
                         const int64_t *row_off_or_null, int64_t total, int do_mask, const bxmi_pwm_t *pwm, float *best_score, int32_t *best_pos);
int bxmi_twobit_pwm_best_strand_dev(bxmi_twobit_t *const *tracks, int32_t n_tracks, const int32_t *track_of, const int32_t *start,
                                    const int8_t *strand_or_null, int64_t n, int32_t width,
                             const int64_t *row_off_or_null, int64_t total, int do_mask, const bxmi_pwm_t *pwm, float *best_score, int32_t *best_pos,
                             void *stream);
int bxmi_twobit_pwm_hits_strand(bxmi_twobit_t *const *tracks, int32_t n_tracks, const int32_t *track_of, const int32_t *start,
                                const int8_t *strand_or_null, int64_t n, int32_t width,
                         const int64_t *row_off_or_null, int64_t total, int do_mask, const bxmi_pwm_t *pwm, const float *threshold, int64_t cap,
                         int64_t *mat_hits, int32_t *hit_row, int32_t *hit_pos, float *hit_score);
int bxmi_twobit_pwm_hits_strand_dev(bxmi_twobit_t *const *tracks, int32_t n_tracks, const int32_t *track_of, const int32_t *start,
                                    const int8_t *strand_or_null, int64_t n, int32_t width,
                             const int64_t *row_off_or_null, int64_t total, int do_mask, const bxmi_pwm_t *pwm, const float *threshold, int64_t cap,
                             int64_t *mat_hits, int32_t *hit_row, int32_t *hit_pos, float *hit_score, void *stream);

/* ---- BED text -> SoA columns on the host (the step before the hot path) ------
 * Strict single-pass parser for what lib/bx/bitset_builders.py:33-46 and
 * scripts/bed_intersect.py:46-50 do per line in Python: skip '#' and blank lines,
 * split on whitespace runs, int() the start/end columns.  It STOPS at the first line
 * that is not plain ASCII BED (stop_line/stop_off), so the caller can hand the rest to
 * the reference's own semantics; it never reinterprets or repairs input. */
typedef struct bxmi_bed bxmi_bed_t;
int bxmi_bed_parse(const char *data, int64_t len, int chrom_col, int start_col, int end_col, bxmi_bed_t **out);
int bxmi_bed_destroy(bxmi_bed_t *b);
int bxmi_bed_info(const bxmi_bed_t *b, int64_t *n_rows, int32_t *n_chroms, int64_t *stop_line, int64_t *stop_off,
                  int64_t *lines_seen);
/* Borrowed views, valid until bxmi_bed_destroy: chromosome id (first-appearance order), start, end,
 * and each row's line as (offset, length incl. newline) into the parsed buffer. */
int bxmi_bed_columns(const bxmi_bed_t *b, const int32_t **chrom_id, const int64_t **start, const int64_t **end,
                     const int64_t **line_off, const int32_t **line_len);
const char *bxmi_bed_chrom_name(const bxmi_bed_t *b, int32_t id);
/* Write the lines with mask[row] != 0, each followed by `suffix`, to file descriptor fd. */
int bxmi_bed_emit_lines(const bxmi_bed_t *b, const char *data, const uint8_t *mask, const char *suffix, int fd);

/* ---- delimited interval text -> SoA columns (the reader side of the operations layer) --------
 * What lib/bx/intervals/io.py:106-216 (GenomicIntervalReader over tabular/io.py:86-156) does per line, for the lines
 * whose outcome is certain: blank lines, comment / header lines (first line starting with one of `comment_prefixes`),
 * and rows whose TAB-separated chromosome / start / end / strand fields are already in the normal form the reader writes
 * back (stripped name, canonical integers, "+" or "-", start <= end).  It STOPS at the first other line (stop_off); the
 * caller continues from there with the reference's own per-line semantics.  strand_col < 0 or beyond the row: no strand. */
typedef struct bxmi_tab bxmi_tab_t;
int bxmi_tab_parse(const char *data, int64_t len, int chrom_col, int start_col, int end_col, int strand_col,
                   const char *const *comment_prefixes, int n_prefixes, bxmi_tab_t **out);
int bxmi_tab_destroy(bxmi_tab_t *b);
int bxmi_tab_info(const bxmi_tab_t *b, int64_t *n_lines, int32_t *n_chroms, int64_t *stop_off);
/* Borrowed per-LINE views, valid until bxmi_tab_destroy: kind (0 row, 1 blank, 2 comment, 3 header), the line's offset and
 * length (without its newline) in the parsed buffer, and for rows the chromosome id (first-appearance order), start, end
 * and strand byte ('+', '-', 0 = no strand field). */
int bxmi_tab_columns(const bxmi_tab_t *b, const uint8_t **kind, const int64_t **line_off, const int32_t **line_len, const int32_t **chrom_id,
                     const int64_t **start, const int64_t **end, const uint8_t **strand);
const char *bxmi_tab_chrom_name(const bxmi_tab_t *b, int32_t id);

/* ---- the path's only collective (multi-GPU, one process per GPU) ---------------------------
 * Intervals on different chromosomes never meet (scripts/interval_join.py:21-28 keeps one tree per chromosome,
 * lib/bx/bitset_builders.py:31-45 one bitset), so a genome is sharded by chromosome with NO data-path exchange; what
 * the ranks do exchange is the vector of per-chromosome overlap totals: an int64 sum all-reduce, RCCL over xGMI.
 * rank 0 makes the 128-byte id and hands it to the others through whatever launched them; every rank then creates
 * its communicator on its CURRENT device.  bxmi_allreduce_i64 works in place on device memory, ordered on `stream`;
 * n must be the same on every rank (n == 0 returns at once without entering the collective).
 * librccl.so is opened on first use; without it these four calls fail with BXMI_EHIP and nothing else is affected. */
typedef struct bxmi_comm bxmi_comm_t;
int bxmi_comm_unique_id(void *id128);
int bxmi_comm_create(bxmi_comm_t **out, const void *id128, int rank, int world);
int bxmi_comm_destroy(bxmi_comm_t *c);
int bxmi_allreduce_i64(bxmi_comm_t *c, int64_t *buf_dev, int64_t n, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* BXMI_H */
