// count_plan.hpp -- every decision of the large-batch count pass (bm_count_segments in intervals.hip) that does not need the
// device: tile shape, padding, item size, the total-only walk, 8-bit counts, the folded parameter block, order check or probe,
// the sorted-batch path, slice lanes, the tile numbering and the size of every scratch buffer.  bm_plan_pass takes plain values
// and returns a BmPassPlan; the launcher reads the feedback words, plans, reserves what the plan sizes, updates the handle's
// bookkeeping from it and launches.
//
// This header is plain C++ (no HIP header): tests/test_host_logic.py compiles tests/cpp/count_plan_test.cpp with g++ and checks
// the rules below on the CPU.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace bxmi {

// What a search workgroup keeps in LDS; every index of a batch must have qualified for the batch's stage (bm_choose_stage).
enum class Stage {
    None,         // the index takes the older paths
    Slices,       // key slices (count_slices.hpp)
    Dense,        // dense unit images (count_dense.hpp)
    Cells,        // bitmap-cell images of units (count_dense.hpp, bp_*: the flat walk, counts out of place)
    OffsetCells,  // offset-cell images of units (offset_cells.hpp: sparse indexes, or the clumped layout)
};
constexpr int N_STAGES = 5;

// The layout constants of the device headers the sizes depend on (intervals.hip asserts that they agree).
constexpr int PLAN_NB = 2048;           // BM_NB
constexpr int PLAN_GROUP_TILES = 64;    // BM_GROUP_TILES
constexpr int PLAN_CHUNK = 65536;       // BM_CHUNK
constexpr int PLAN_PAR_CHUNK = 16;      // BM_PAR_CHUNK
constexpr int PLAN_PAD_ROOM = 4096 + 544;  // BM_PAD_ROOM
constexpr int PLAN_PART_Q = 1024;       // BM_PART_Q
constexpr int PLAN_SLOTS = 64;          // PT_SLOTS
constexpr int PLAN_WALK_THREADS = 1024;  // BD_THREADS
constexpr int PLAN_NBK = 2 * PLAN_NB;   // FX_NBK
constexpr int PLAN_BOUNDS_ROW = PLAN_NB + 2;  // BS_BOUNDS_ROW
constexpr size_t PLAN_ITEM_BYTES = 16;  // sizeof(int4)

// The option values the plan reads (see the option comments in intervals.hip), by value: nothing global is read in here.
struct BmPlanKnobs {
    int64_t bm_variant = -1;
    int64_t sl_flat = 1;
    int64_t bd_chunk = 0;
    int64_t bm_chunk = 0;
    int64_t sl_lanes = 0;
    int64_t bd_w8 = -1;
    int64_t tot_walk = 1;
    int64_t sorted_path = 1;
    int64_t sorted_cells = 1;
    int64_t order_skip = -1;
};

// One segment (a sealed index with its queries) as the plan sees it.
struct BmPlanSegIn {
    int64_t nq = 0;
    int f = 0, shift = 0, stride = 0;  // the geometry of the stage's images (slices: the f that sl_geom picked, stride 0)
    bool want_counts = true, want_total = false;
    bool bd_blocks = false;  // dense images with block-relative ranks
    int bo_state = 0;        // 2 = the offset cells are in the clumped layout
    bool w8_off = false;     // the index has switched 8-bit counts off
    int64_t n = 0, span = 1;  // targets, and the coordinates they span (cmax - cmin + 1)
    size_t sl_lds = 0;       // slices: what sl_geom says a unit stages ...
    int64_t sl_run = 0;      // ... and the (tile, unit) run it expects of a uniform batch
};

struct BmPlanIn {
    Stage stage = Stage::None;
    std::vector<BmPlanSegIn> seg;
    bool find = false, sub = false, direct = false;  // find()'s count half (BmFindCtx), ordered by half buckets, offsets as query-order prefixes
    BmPlanKnobs knobs;
    size_t seg_bytes = 0;  // sizeof(BmSeg): the parameter block holds one per segment
    // the first handle's feedback words as read before planning, and its bookkeeping
    unsigned long long fb_wide_counts = 0;  // [0] counts that did not fit 8 bits so far
    unsigned long long fb_order = 0;        // [1] (sequence number << 1) | "not sorted" of the latest order check answered
    int64_t w8_queries = 0;
    unsigned long long order_seq = 0, order_seen = 0;
    int unsorted_streak = 0;
    bool order_skip = false;
};

enum class BmPlanError { None, TooManyQueries, TooManySegments, FindNeedsOneSliceIndex };

struct BmPlanSegOut {
    int64_t tile0, ntiles, tile_end;  // first tile in the batch's numbering, tiles that hold queries, first tile of the next segment
};

struct BmPassPlan {
    BmPlanError error = BmPlanError::None;
    bool empty = false;  // no queries: nothing to launch
    int n = 0;
    int64_t nq_all = 0;
    // stage
    bool wide = false, slices = false, cells = false, fxsub = false;
    bool slices_flat = false;  // count-only passes on key slices: the flat 16-byte walk
    bool dense = false;        // counts out of place (16 bits), unit run table: dense images, cell images, the flat walk on slices
    // tile shape
    int variant = 0;           // 0 = 512 threads x 32 queries, 1 = 1024 x 16, 2 = 1024 x 32
    int tile_log2 = 14;
    bool pad = false;          // every unit's run of a tile on whole 16-byte slots
    int64_t tile_stride = 0;
    // tile numbering
    std::vector<BmPlanSegOut> seg;
    int64_t ntp = 0;           // tiles in the padded numbering (a multiple of PLAN_GROUP_TILES)
    int ngroups = 0;
    // search items
    int chunk = 0;             // queries per search work item
    int64_t max_items = 0;
    unsigned sgrid = 0;
    size_t search_lds = 0;
    bool big = false;          // offset cells in the clumped layout: a unit image beyond what the 512-thread walk loads
    bool any_blocks = false, any_total = false;
    int lanes = -1;            // slices without the flat walk of count_dense.hpp: 0 = the flat walk of count_slices.hpp, 16 or 64 lanes per run
    bool tot_walk = false;     // total-only batch on cell images: the walk keeps the totals
    // 8-bit counts
    bool w8_asked = false;     // the layout allows them: the feedback word was weighed (the launcher keeps the feedback memory ready)
    bool w8 = false;
    bool w8_trip = false;      // the feedback says too many counts did not fit: the first index keeps 16-bit counts from now on
    // order
    bool multi_sorted = false;     // several indexes whose sorted batches are answered in one walk over the segments
    bool order_aware = false;      // the pass watches the order of the starts (exact check, or the probe)
    bool sorted_on_cells = false;  // one index: a sorted batch is answered from the cell images stretch by stretch
    unsigned long long order_seen = 0;  // the handle's bookkeeping after the feedback word was weighed
    int unsorted_streak = 0;
    bool order_skip = false;
    bool probe_first = false;      // the handle's first batch: the launcher asks the probe alone and waits (bm_plan_set_order_skip with its answer)
    bool order_check = false;      // the exact check is launched in front of the pass, every kernel behind it stands down on a sorted batch
    bool probe_rides = false;      // no check: the probe rides on the parameter block's writer
    bool fold_params = false;      // the tile sort's first workgroup writes the parameter block (no parameter kernel)
    unsigned sorted_chunk = 0;     // the sorted walk: queries per item, and the most items
    size_t sorted_items = 0;
    size_t bounds_bytes = 0;       // ... its unit bounds in front of the items
    // parameter block: [segments][totals pointers][tile -> segment]
    size_t seg_bytes = 0, tile_off = 0;
    int n_zero = 0;                // 64-bit words zeroed in front of the pass: the partial totals, the order flag, the item counters
    // scratch, in bytes (0 = the pass does not use the buffer)
    struct Bytes {
        size_t tesc = 0, recs = 0, tend = 0, slots = 0, tbl = 0, runT = 0, unitT = 0, grpcnt = 0, unitcnt = 0, cnt16 = 0, items = 0;
        size_t sl_cnt = 0, sl_loff = 0;
        size_t fx_tbl2 = 0, fx_runT2 = 0, fx_hc = 0, fx_svq = 0, fx_parts = 0, fx_tile_tot = 0, fx_tile_base = 0;
        size_t params = 0, p_slots = 0, bs_plan = 0;
    } bytes;
};

inline int64_t plan_div_up(int64_t a, int64_t b) { return (a + b - 1) / b; }

// What depends on whether the exact order check is launched.  The order check and the stand-down of the sorted-batch kernel
// cost a shuffled batch 24 us (of 750).  What the order checks find is mirrored into host memory (ivl_local_count_kernel,
// bs_walk_kernel or the workgroup that runs the probe write it, nobody waits for it): after two batches in a row that were NOT
// sorted the check is no longer launched -- every kernel of the exchange runs unconditionally -- and a PROBE rides on the
// parameter kernel instead: 8192 consecutive starts; a descent among them says "shuffled" for certain, none brings the exact
// check back with the next call.  A sorted batch that arrives in between goes through the exchange (0.78 instead of 0.62 ms
// per 100 M), exact as ever.  (Watching the order exactly inside the tile sort, which has every start in registers, cost that
// kernel 13-19 us -- what the check costs.)
inline void bm_plan_set_order_skip(BmPassPlan &P, bool skip, const BmPlanKnobs &k)
{
    P.order_skip = skip;
    P.probe_rides = P.order_aware && skip && k.order_skip != 0;
    P.order_check = P.order_aware && !P.probe_rides;
    // Folded: whenever the tile sort is the batch's first kernel.  With the order check in front (a handle's first batches, sorted
    // input) or more than PLAN_PAR_CHUNK segments (a whole genome on one GPU) the parameter kernel stays a launch of its own.
    P.fold_params = P.n <= PLAN_PAR_CHUNK && !P.order_check;
    // the sorted walk's plan: [unit bounds][item count][items]
    P.bytes.bs_plan = 0;
    if (P.order_check && (P.multi_sorted || P.sorted_on_cells)) P.bytes.bs_plan = P.bounds_bytes + (P.sorted_items + 1) * PLAN_ITEM_BYTES;
}

// The tile shape alone (the slice geometry of a segment depends on the tile size: the launcher asks this first, evaluates
// sl_geom, then plans).  Reads of a segment only nq and, on cell images, f.
inline int bm_plan_variant(const BmPlanIn &in)
{
    const BmPlanKnobs &k = in.knobs;
    const int n = (int)in.seg.size();
    const bool wide = in.stage == Stage::OffsetCells, cells = in.stage == Stage::Cells || wide;
    int64_t nq_all = 0;
    for (const BmPlanSegIn &s : in.seg) nq_all += s.nq;
    // tile shape: 32768-query tiles halve the number of (tile, bucket) runs the search has to fetch, but their sort
    // kernel runs one workgroup per CU and wants a grid of several hundred full tiles
    // (a batch over several indexes: every segment starts on a group of 64 tiles, so the big tiles only where the segments are
    // big too -- a genome of 100 M queries, not its eighth on one of eight GPUs)
    int variant = k.bm_variant >= 0 ? (int)k.bm_variant : (nq_all >= ((int64_t)32 << 20) * (n == 1 ? 1 : 2) ? 2 : 0);
    // cell images are searched on padded runs only: a unit of two buckets needs a tile sort whose threads own two buckets each
    // (the 1024-thread shapes), the 512-thread shape owns four
    // ... and the 1024-thread shape is the faster sort for cell images whatever the unit (a rank's share of a genome, offset cells,
    // f >= 2: 0.413 / 0.241 / 0.138 ms for 50 / 25 / 13 M queries against 0.432 / 0.259 / 0.147 with 512 threads x 32 queries)
    if (cells && variant == 0 && k.bm_variant < 0) variant = 1;
    if (cells && variant == 0)
        for (const BmPlanSegIn &s : in.seg)
            if (s.f < 2) variant = 1;
    if (in.find && in.sub && variant == 0) variant = 1;  // (the half-bucket tile sort has the 1024-thread shapes only)
    return variant;
}

inline BmPassPlan bm_plan_pass(const BmPlanIn &in)
{
    BmPassPlan P;
    const BmPlanKnobs &k = in.knobs;
    const int n = P.n = (int)in.seg.size();
    const Stage stage = in.stage;
    const bool wide = P.wide = stage == Stage::OffsetCells;  // offset cells: the cell images of sparse indexes
    const bool slices = P.slices = stage == Stage::Slices, cells = P.cells = stage == Stage::Cells || wide;
    const bool fx = in.find, fxsub = P.fxsub = in.find && in.sub;
    // (find() needs 32-bit counts apart from the records and the tile-sorted offsets: the flat walk has that form for find_exchange.hpp only)
    const bool slices_flat = P.slices_flat = slices && !fx && k.sl_flat != 0;
    const bool dense = P.dense = stage == Stage::Dense || cells || slices_flat /* the flat walk */;
    int64_t nq_all = 0;
    for (const BmPlanSegIn &s : in.seg) nq_all += s.nq;
    P.nq_all = nq_all;
    if (nq_all >= ((int64_t)1 << 31)) return P.error = BmPlanError::TooManyQueries, P;
    if (n > 4096) return P.error = BmPlanError::TooManySegments, P;
    if (fxsub && (n != 1 || !slices)) return P.error = BmPlanError::FindNeedsOneSliceIndex, P;
    const int variant = P.variant = bm_plan_variant(in);
    const int tile_log2 = P.tile_log2 = variant == 2 ? 15 : 14;
    const int64_t tile = (int64_t)1 << tile_log2;

    // the batch's tile numbering: every segment starts on a plan-group boundary
    P.seg.resize((size_t)n);
    int64_t ntp = 0;
    size_t max_stride = 0, sl_lds = 0;
    int64_t sl_run = INT64_MAX;  // shortest expected (tile, unit) run of the batch
    for (int i = 0; i < n; i++) {
        const BmPlanSegIn &s = in.seg[(size_t)i];
        BmPlanSegOut &o = P.seg[(size_t)i];
        P.any_blocks |= stage == Stage::Dense && s.bd_blocks;
        if (slices) {
            if (s.sl_lds > sl_lds) sl_lds = s.sl_lds;
            if (s.sl_run < sl_run) sl_run = s.sl_run;
        }
        o.tile0 = ntp;
        o.ntiles = plan_div_up(s.nq, tile);
        ntp += plan_div_up(o.ntiles, PLAN_GROUP_TILES) * PLAN_GROUP_TILES;
        o.tile_end = ntp;
        if ((size_t)s.stride > max_stride) max_stride = (size_t)s.stride;
        P.any_total |= s.want_total;
    }
    P.ntp = ntp;
    if (ntp == 0) return P.empty = true, P;
    const int ngroups = P.ngroups = (int)(ntp / PLAN_GROUP_TILES);

    // item size
    int chunk = dense ? (k.bd_chunk ? (int)k.bd_chunk : (cells || slices_flat ? 2 : 4) * PLAN_CHUNK) : k.bm_chunk ? (int)k.bm_chunk : PLAN_CHUNK;
    // a small batch (one rank's share of a genome on eight GPUs: 13 M queries) cut into items of 128 Ki queries is a hundred
    // workgroups on 256 CUs (measured: search 154 us of a 255 us pass); items of nq / 512, at least a tile
    // (every item stages its unit's keys again: at 25 M queries, 192 items, the smaller items already cost more than
    // the idle CUs did -- 0.33 -> 0.38 ms -- so only batches that leave a third of the chip idle are cut finer)
    if (!(dense ? k.bd_chunk : k.bm_chunk) && !(stage == Stage::Dense || cells) && nq_all / chunk < 160) {
        const int64_t c = nq_all / 512;
        chunk = (int)(c < 16384 ? 16384 : c);
    }
    P.chunk = chunk;
    int64_t max_items = (int64_t)n * (PLAN_NB + 2) + 2 * (nq_all / chunk) + 2;
    if (dense) {  // every segment has at most PLAN_NB >> f units; empty workgroups of 157 KB of LDS are not free
        // (the padded layout counts up to three more slots per tile and unit as "queries" of the unit)
        int64_t pad_slots = 0;
        for (int i = 0; i < n; i++) pad_slots += 3 * (int64_t)(PLAN_NB >> in.seg[(size_t)i].f) * (P.seg[(size_t)i].tile_end - P.seg[(size_t)i].tile0);
        max_items = 2 * ((nq_all + pad_slots) / chunk) + 2;
        for (int i = 0; i < n; i++) max_items += (PLAN_NB >> in.seg[(size_t)i].f) + 2;
    }
    P.max_items = max_items;
    P.sgrid = (unsigned)(plan_div_up(max_items, 8) * 8);

    // PAD: every unit's run of a tile on whole 16-byte slots (the search's load ring needs one store per pass); the tile
    // sort's scan keeps a unit inside one thread or a few neighbouring lanes
    bool pad = stage == Stage::Dense || cells;
    for (int i = 0; i < n && pad; i++) pad = (1 << in.seg[(size_t)i].f) >= (variant == 0 ? 4 : 2);
    P.pad = pad;
    const int64_t tile_stride = P.tile_stride = tile + (pad ? PLAN_PAD_ROOM : 0);

    // nobody wants counts, only totals, and the persistent walk serves the batch: it keeps the totals itself (bw_search_kernel<.., TOT>)
    bool tot_walk = k.tot_walk != 0 && cells && pad && !fx && P.any_total;
    for (int i = 0; i < n && tot_walk; i++) tot_walk = !in.seg[(size_t)i].want_counts;
    P.tot_walk = tot_walk;

    P.search_lds = slices ? sl_lds : max_stride * 16;
    if (slices_flat && P.search_lds < 4096) P.search_lds = 4096;
    P.big = wide && max_stride * 16 > (size_t)10 * (PLAN_WALK_THREADS / 2) * 16;  // (beyond what the 512-thread walk loads: 80 KB)
    if (slices && !slices_flat) {
        // long runs (sparse index, big units): the flat walk; else L lanes per run
        P.lanes = k.sl_lanes < 0 ? 0 : (k.sl_lanes ? (int)k.sl_lanes : (sl_run >= 96 ? 0 : (sl_run >= 40 ? 64 : 16)));
        if (fx && P.lanes == 0) P.lanes = 64;  // (the fill half has no flat walk)
    }

    // 8-bit counts (0xFF = recomputed by the un-permute kernel, exact either way): half the bytes of the second exchange
    // when the counts are small.  Cell images only serve indexes without piled-up coordinates, so the density says what to
    // expect: fewer than 128 targets per 2048 coordinates (configs[1]: 82; a count of 255 needs a query of ~6000).  What the
    // prediction misses -- long queries, targets crowded into part of the span -- the feedback catches: once more than one
    // count in 64 did not fit, the index keeps 16-bit counts (worst case before that: every count recomputed, ~2 x the pass).
    // (a batch over several indexes -- a genome -- keeps the feedback with its first index: every index has to be sparse enough,
    // none may have switched the narrow counts off)
    if (pad && cells && k.bd_w8 != 0 && !tot_walk) {  // (a total-only walk stores no counts at all)
        P.w8_asked = true;
        P.w8_trip = (int64_t)in.fb_wide_counts * 64 > in.w8_queries && in.fb_wide_counts > 4096;
        bool narrow = true;
        for (int i = 0; i < n; i++) {
            const BmPlanSegIn &s = in.seg[(size_t)i];
            narrow = narrow && !(s.w8_off || (i == 0 && P.w8_trip)) && s.n * 2048 < s.span * 128;
            if (wide && s.bo_state == 2) narrow = false;  // (the clumped layout: hundreds of targets around every hot spot -- its first pass on 8-bit counts recomputed all of them: 24 ms)
        }
        P.w8 = k.bd_w8 > 0 || narrow;
    }

    // order
    // (several indexes: only the walk on cell images has a sorted-batch form over segments)
    bool multi_sorted = n > 1 && !fx && k.sorted_path && k.sorted_cells != 0 && cells && pad;
    for (int i = 0; i < n && multi_sorted; i++) multi_sorted = in.seg[(size_t)i].nq < ((int64_t)1 << 32) - 8;
    P.multi_sorted = multi_sorted;
    P.order_aware = k.sorted_path && (n == 1 || multi_sorted) && !fx;
    P.order_seen = in.order_seen, P.unsorted_streak = in.unsorted_streak;
    bool skip = in.order_skip;
    if (P.order_aware) {
        if ((in.fb_order >> 1) > in.order_seen) {
            P.unsorted_streak = (in.fb_order & 1ull) ? in.unsorted_streak + 1 : 0;
            P.order_seen = in.fb_order >> 1;
            skip = P.unsorted_streak >= 2;
        }
        // The handle's first large batch: nothing is known about the caller's order yet, and this call has waited for the
        // device already (it built the index's images) -- so the probe is asked alone and its answer read back: a descent
        // among its 8192 starts drops the exact check from this very pass (a cold pass paid 24 us of 700 for it).
        P.probe_first = in.order_seq == 0 && k.order_skip != 0;
        // Cell images (bitmap or offset cells): a sorted batch is answered straight from them, stretch by stretch (count_dense.hpp,
        // bs_*): the order check leaves where every unit's queries begin, a plan cuts long stretches, the walk loads a unit's
        // image and answers its queries as they lie.  Other stages keep the first-generation kernel for sorted batches.
        P.sorted_on_cells = !multi_sorted && cells && pad && k.sorted_cells != 0 && in.seg[0].nq < ((int64_t)1 << 32) - 8;
        P.sorted_chunk = (unsigned)(k.bd_chunk ? k.bd_chunk : (wide ? 1 : 2) * PLAN_CHUNK);
        if (multi_sorted) {
            // a batch over several indexes: order check and plan per segment, one walk (count_dense.hpp, bs_*_multi)
            P.sorted_items = 4;
            for (int i = 0; i < n; i++) P.sorted_items += (size_t)(PLAN_NB >> in.seg[(size_t)i].f) + 4 + (size_t)(in.seg[(size_t)i].nq / P.sorted_chunk);
            P.bounds_bytes = ((size_t)n * PLAN_BOUNDS_ROW * 4 + 16 + 15) & ~(size_t)15;
        } else if (P.sorted_on_cells) {
            const int units = PLAN_NB >> in.seg[0].f;
            P.sorted_items = (size_t)units + 4 + (size_t)(in.seg[0].nq / P.sorted_chunk);
            P.bounds_bytes = (size_t)(units + 2) * 4 + 16;  // (the items start on the next 16-byte boundary)
        }
    }
    bm_plan_set_order_skip(P, skip, k);

    // parameter block in HBM: [segments][totals pointers][tile -> segment]
    P.seg_bytes = (size_t)n * in.seg_bytes;
    const size_t tot_bytes = (size_t)n * sizeof(void *);
    P.tile_off = (P.seg_bytes + tot_bytes + 15) & ~(size_t)15;
    P.n_zero = n * PLAN_SLOTS + 8;

    BmPassPlan::Bytes &b = P.bytes;
    const size_t T = (size_t)ntp;
    if (tot_walk) b.tesc = T * 4;  // the tiles that hold escape records
    b.recs = T * (size_t)tile_stride * 4;
    if (pad) b.tend = T * 4;
    b.slots = T * (size_t)tile * 2;
    b.tbl = T * PLAN_NB * 2;
    if (!dense) b.runT = T * PLAN_NB * 4;
    if (dense) b.unitT = T * (PLAN_NB + 1) * 2;  // (+ the row behind the last unit)
    b.grpcnt = (size_t)ngroups * PLAN_NB * 4;
    b.unitcnt = (size_t)ngroups * PLAN_NB * 4;
    if (dense && !fxsub) b.cnt16 = T * (size_t)tile_stride * 2;
    b.items = (size_t)(max_items + 2) * PLAN_ITEM_BYTES;  // [0] = the item count, items from [1]
    if (fx) {  // find(): counts apart from the records, and the tile-sorted offsets
        b.sl_cnt = T * (size_t)tile * 4;
        b.sl_loff = T * (size_t)tile * 4;
    }
    if (fxsub) {  // ... and what find_exchange.hpp's fill and copy read
        b.fx_tbl2 = T * PLAN_NBK * 2;
        b.fx_runT2 = T * PLAN_NBK * 4;
        b.fx_hc = T * (size_t)tile * 4;
        b.fx_svq = T * (size_t)tile * 4;
        b.fx_parts = T * (size_t)(tile / PLAN_PART_Q) * 8;
        b.fx_tile_tot = T * 8;
        b.fx_tile_base = (T + 2) * 8;  // (+ the grand total, + the largest tile total)
    }
    b.params = P.tile_off + T * sizeof(unsigned short);
    // [segments][PLAN_SLOTS partial totals], then the flag: 1 = the starts are NOT sorted
    // ([+0] the order flag, [+4 .. +8) the search's item counters)
    b.p_slots = ((size_t)n * PLAN_SLOTS + 8) * sizeof(unsigned long long);
    return P;
}

}  // namespace bxmi
