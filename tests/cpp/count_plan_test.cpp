// CPU check of bx-python_amd/csrc/count_plan.hpp (compiled by tests/test_host_logic.py with g++): the decisions of the
// large-batch count pass -- tile shape, padding, item size, the total-only walk, 8-bit counts, the folded parameter block,
// order check or probe, the sorted paths, slice lanes, the tile numbering and the scratch sizes -- against the rules the
// comments of count_plan.hpp and DESIGN.md 3.1 state.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "count_plan.hpp"

using namespace bxmi;

#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            std::printf("%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                    \
        }                                                                    \
    } while (0)

constexpr int64_t M = 1000000;
constexpr size_t SEG_BYTES = 200;  // (any size: the parameter block scales with it)

// a sparse-enough index (fewer than 128 targets per 2048 coordinates) on images of 2^f buckets
static BmPlanSegIn seg(int64_t nq, int f, bool counts = true, bool total = false)
{
    BmPlanSegIn s;
    s.nq = nq, s.f = f, s.shift = 10, s.stride = 4096;
    s.want_counts = counts, s.want_total = total;
    s.n = 1 * M, s.span = 100 * M;
    s.sl_lds = 30000, s.sl_run = 20;
    return s;
}

// a handle that has answered batches before and is not watching the order (two shuffled batches seen)
static BmPlanIn batch(Stage stage, std::vector<BmPlanSegIn> segs)
{
    BmPlanIn in;
    in.stage = stage;
    in.seg = std::move(segs);
    in.seg_bytes = SEG_BYTES;
    in.order_seq = 7, in.order_seen = 7, in.unsorted_streak = 2, in.order_skip = true;
    in.fb_order = (7ull << 1) | 1ull;
    return in;
}

static void tile_shape_and_padding()
{
    // one index, cell images with f >= 2, 100 M queries, counts wanted, order check skipped
    BmPlanIn in = batch(Stage::Cells, {seg(100 * M, 3)});
    BmPassPlan P = bm_plan_pass(in);
    CHECK(P.error == BmPlanError::None && !P.empty);
    CHECK(P.variant == 2 && P.tile_log2 == 15);
    CHECK(P.pad && P.tile_stride == 32768 + PLAN_PAD_ROOM);
    CHECK(P.order_aware && !P.order_check && P.probe_rides && P.fold_params);
    CHECK(P.w8_asked && P.w8 && !P.w8_trip);  // 1 M targets on 100 M coordinates: 20 per 2048
    CHECK(P.dense && !P.tot_walk && !P.slices_flat && P.lanes == -1);
    // ... the density rule: fewer than 128 targets per 2048 coordinates
    in.seg[0].n = 6250000;  // exactly 128 per 2048
    CHECK(!bm_plan_pass(in).w8);
    in.seg[0].n = 6249999;
    CHECK(bm_plan_pass(in).w8);
    // the same at 13 M queries: 1024 x 16
    in = batch(Stage::Cells, {seg(13 * M, 3)});
    P = bm_plan_pass(in);
    CHECK(P.variant == 1 && P.tile_log2 == 14 && P.pad && P.fold_params);
    in.stage = Stage::OffsetCells;
    CHECK(bm_plan_pass(in).variant == 1);
    // the other stages keep the 512-thread shape for small batches, the 32768-query tiles from 32 Mi queries (twice that over several indexes)
    CHECK(bm_plan_pass(batch(Stage::Dense, {seg(13 * M, 3)})).variant == 0);
    CHECK(bm_plan_pass(batch(Stage::Slices, {seg(13 * M, 3)})).variant == 0);
    CHECK(bm_plan_pass(batch(Stage::Dense, {seg(((int64_t)32 << 20) - 1, 3)})).variant == 0);
    CHECK(bm_plan_pass(batch(Stage::Dense, {seg((int64_t)32 << 20, 3)})).variant == 2);
    CHECK(bm_plan_pass(batch(Stage::Dense, {seg((int64_t)16 << 20, 3), seg((int64_t)16 << 20, 3)})).variant == 0);
    CHECK(bm_plan_pass(batch(Stage::Dense, {seg((int64_t)32 << 20, 3), seg((int64_t)32 << 20, 3)})).variant == 2);
    // f < 2 forces a 1024-thread shape on cell images, even against the knob
    in = batch(Stage::Cells, {seg(13 * M, 3), seg(13 * M, 1)});
    in.knobs.bm_variant = 0;
    CHECK(bm_plan_pass(in).variant == 1);
    in.seg[1].f = 2;
    CHECK(bm_plan_pass(in).variant == 0);
    // pad: every segment's 2^f at least the shape's buckets per thread (512 threads: 4, 1024 threads: 2); never on key slices
    CHECK(bm_plan_pass(batch(Stage::Dense, {seg(13 * M, 2)})).pad);
    CHECK(!bm_plan_pass(batch(Stage::Dense, {seg(13 * M, 1)})).pad);
    CHECK(!bm_plan_pass(batch(Stage::Dense, {seg(13 * M, 2), seg(13 * M, 1)})).pad);
    CHECK(bm_plan_pass(batch(Stage::Dense, {seg(40 * M, 1)})).pad);  // (1024 x 32)
    CHECK(bm_plan_pass(batch(Stage::Cells, {seg(13 * M, 1)})).pad);
    CHECK(!bm_plan_pass(batch(Stage::Cells, {seg(13 * M, 0)})).pad);
    CHECK(!bm_plan_pass(batch(Stage::Cells, {seg(13 * M, 3), seg(13 * M, 0)})).pad);
    P = bm_plan_pass(batch(Stage::Slices, {seg(13 * M, 5)}));
    CHECK(!P.pad && P.tile_stride == 16384 && P.bytes.tend == 0);
    // without padded runs: no 8-bit counts, no walk from the cell images for sorted batches
    P = bm_plan_pass(batch(Stage::Cells, {seg(13 * M, 0)}));
    CHECK(!P.w8_asked && !P.w8 && !P.sorted_on_cells);
}

static void total_only_walk()
{
    BmPlanIn in = batch(Stage::Cells, {seg(13 * M, 3, false, true)});
    BmPassPlan P = bm_plan_pass(in);
    CHECK(P.tot_walk && P.any_total && !P.w8_asked && !P.w8);
    CHECK(P.bytes.tesc == (size_t)P.ntp * 4);
    in.stage = Stage::OffsetCells;
    CHECK(bm_plan_pass(in).tot_walk);
    // one segment wants counts: the counts pass
    in = batch(Stage::Cells, {seg(13 * M, 3, false, true), seg(13 * M, 3, true, true)});
    P = bm_plan_pass(in);
    CHECK(!P.tot_walk && P.bytes.tesc == 0 && P.w8);
    in.seg[1].want_counts = false;
    CHECK(bm_plan_pass(in).tot_walk);
    // nobody wants a total: nothing to keep
    in.seg[0].want_total = in.seg[1].want_total = false;
    CHECK(!bm_plan_pass(in).tot_walk);
    // dense images, key slices, packed runs: the counts pass without its stores
    CHECK(!bm_plan_pass(batch(Stage::Dense, {seg(13 * M, 3, false, true)})).tot_walk);
    CHECK(!bm_plan_pass(batch(Stage::Slices, {seg(13 * M, 3, false, true)})).tot_walk);
    CHECK(!bm_plan_pass(batch(Stage::Cells, {seg(13 * M, 0, false, true)})).tot_walk);
    // the knob
    in = batch(Stage::Cells, {seg(13 * M, 3, false, true)});
    in.knobs.tot_walk = 0;
    P = bm_plan_pass(in);
    CHECK(!P.tot_walk && P.bytes.tesc == 0 && P.w8);
}

static void multi_index_batches()
{
    std::vector<BmPlanSegIn> many(17, seg(1 * M, 3));
    BmPassPlan P = bm_plan_pass(batch(Stage::Dense, many));
    CHECK(!P.order_aware && !P.order_check && !P.fold_params);  // (beyond PLAN_PAR_CHUNK segments)
    many.resize(16);
    CHECK(bm_plan_pass(batch(Stage::Dense, many)).fold_params);
    // refusals
    CHECK(bm_plan_pass(batch(Stage::Cells, std::vector<BmPlanSegIn>(4097, seg(1000, 3)))).error == BmPlanError::TooManySegments);
    CHECK(bm_plan_pass(batch(Stage::Cells, std::vector<BmPlanSegIn>(4096, seg(1000, 3)))).error == BmPlanError::None);
    CHECK(bm_plan_pass(batch(Stage::Cells, {seg((int64_t)1 << 30, 3), seg((int64_t)1 << 30, 3)})).error == BmPlanError::TooManyQueries);
    CHECK(bm_plan_pass(batch(Stage::Cells, {seg((int64_t)1 << 30, 3), seg(((int64_t)1 << 30) - 1, 3)})).error == BmPlanError::None);
    // no queries at all: nothing to launch
    CHECK(bm_plan_pass(batch(Stage::Cells, {seg(0, 3), seg(0, 3)})).empty);
    // the sorted-batch form over segments: several indexes on padded cells only
    BmPlanIn in = batch(Stage::Cells, {seg(5 * M, 3), seg(5 * M, 2)});
    P = bm_plan_pass(in);
    CHECK(P.multi_sorted && P.order_aware && !P.sorted_on_cells);
    in.stage = Stage::OffsetCells;
    CHECK(bm_plan_pass(in).multi_sorted);
    CHECK(!bm_plan_pass(batch(Stage::Cells, {seg(5 * M, 3)})).multi_sorted);
    CHECK(!bm_plan_pass(batch(Stage::Cells, {seg(5 * M, 3), seg(5 * M, 0)})).multi_sorted);  // (packed runs)
    for (Stage s : {Stage::Dense, Stage::Slices}) {
        P = bm_plan_pass(batch(s, {seg(5 * M, 3), seg(5 * M, 3)}));
        CHECK(!P.multi_sorted && !P.order_aware && !P.order_check && !P.probe_rides && P.fold_params);
    }
    in = batch(Stage::Cells, {seg(5 * M, 3), seg(5 * M, 3)});
    in.knobs.sorted_cells = 0;
    CHECK(!bm_plan_pass(in).multi_sorted);
    in.knobs.sorted_cells = 1, in.knobs.sorted_path = 0;
    P = bm_plan_pass(in);
    CHECK(!P.multi_sorted && !P.order_aware);
    // with the order check in front, the walk's plan is sized: a row of bounds per segment, items per unit and per chunk
    in = batch(Stage::Cells, {seg(5 * M, 3), seg(5 * M, 2)});
    in.order_skip = false, in.unsorted_streak = 0;
    P = bm_plan_pass(in);
    CHECK(P.order_check && !P.fold_params && P.sorted_chunk == 2u * PLAN_CHUNK);
    CHECK(P.sorted_items == 4 + (size_t)(PLAN_NB >> 3) + 4 + 5 * M / (2 * PLAN_CHUNK) + (size_t)(PLAN_NB >> 2) + 4 + 5 * M / (2 * PLAN_CHUNK));
    CHECK(P.bounds_bytes % 16 == 0 && P.bounds_bytes >= 2 * (size_t)PLAN_BOUNDS_ROW * 4 + 4);
    CHECK(P.bytes.bs_plan == P.bounds_bytes + (P.sorted_items + 1) * 16);
    // 8-bit counts over several indexes: every one sparse enough, none switched off
    in = batch(Stage::Cells, {seg(5 * M, 3), seg(5 * M, 3)});
    CHECK(bm_plan_pass(in).w8);
    in.seg[1].n = 50 * M;
    CHECK(!bm_plan_pass(in).w8);
    in.seg[1].n = 1 * M, in.seg[1].w8_off = true;
    CHECK(!bm_plan_pass(in).w8);
}

static void finds_count_half()
{
    BmPlanIn in = batch(Stage::Slices, {seg(8 * M, 4)});
    in.find = in.sub = true;
    in.seg[0].sl_run = 200;
    BmPassPlan P = bm_plan_pass(in);
    CHECK(P.error == BmPlanError::None && P.fxsub);
    CHECK(P.variant == 1);                            // never the 512-thread shape
    CHECK(!P.slices_flat && !P.dense && !P.pad);      // the flat walk of count_dense.hpp is off
    CHECK(P.lanes == 64);                             // a long run, and still no flat walk
    CHECK(!P.order_aware && !P.order_check && !P.probe_rides && P.fold_params && !P.tot_walk && !P.w8);
    const size_t T = (size_t)P.ntp, tile = 16384;
    CHECK(P.bytes.sl_cnt == T * tile * 4 && P.bytes.sl_loff == T * tile * 4);
    CHECK(P.bytes.fx_tbl2 == T * PLAN_NBK * 2 && P.bytes.fx_runT2 == T * PLAN_NBK * 4);
    CHECK(P.bytes.fx_hc == T * tile * 4 && P.bytes.fx_svq == T * tile * 4 && P.bytes.fx_parts == T * (tile / PLAN_PART_Q) * 8);
    CHECK(P.bytes.fx_tile_tot == T * 8 && P.bytes.fx_tile_base == (T + 2) * 8);
    CHECK(P.bytes.cnt16 == 0 && P.bytes.unitT == 0 && P.bytes.runT == T * PLAN_NB * 4);
    in.knobs.bm_variant = 0;
    CHECK(bm_plan_pass(in).variant == 1);
    in.knobs.bm_variant = 2;
    P = bm_plan_pass(in);
    CHECK(P.variant == 2 && P.bytes.fx_parts == (size_t)P.ntp * 32 * 8);
    in.knobs.bm_variant = -1;
    for (int64_t lanes_knob : {(int64_t)-1, (int64_t)0, (int64_t)16, (int64_t)64})
        for (int64_t run : {(int64_t)10, (int64_t)50, (int64_t)500}) {
            in.knobs.sl_lanes = lanes_knob, in.seg[0].sl_run = run;
            const int lanes = bm_plan_pass(in).lanes;
            CHECK(lanes == 16 || lanes == 64);
        }
    in.knobs.sl_lanes = 0;
    // slices only, one index only
    for (Stage s : {Stage::Dense, Stage::Cells, Stage::OffsetCells}) {
        in.stage = s;
        CHECK(bm_plan_pass(in).error == BmPlanError::FindNeedsOneSliceIndex);
    }
    in.stage = Stage::Slices;
    in.seg.push_back(in.seg[0]);
    CHECK(bm_plan_pass(in).error == BmPlanError::FindNeedsOneSliceIndex);
    // a count pass leaves none of find's buffers behind
    P = bm_plan_pass(batch(Stage::Slices, {seg(8 * M, 4)}));
    CHECK(P.bytes.sl_cnt == 0 && P.bytes.sl_loff == 0 && P.bytes.fx_tbl2 == 0 && P.bytes.fx_runT2 == 0 && P.bytes.fx_hc == 0 && P.bytes.fx_svq == 0 &&
          P.bytes.fx_parts == 0 && P.bytes.fx_tile_tot == 0 && P.bytes.fx_tile_base == 0);
}

static void slices_without_find()
{
    // the flat walk: items of 2 * PLAN_CHUNK queries, unless fewer than 160 of them result -- then nq / 512, at least 16384
    struct { int64_t nq; int chunk; } flat[] = {{4 * M, 16384}, {8388608, 16384}, {8388608 + 512, 16385}, {16 * M, 31250}, {160ll * 2 * PLAN_CHUNK - 1, 40959},
                                                {160ll * 2 * PLAN_CHUNK, 2 * PLAN_CHUNK}, {100 * M, 2 * PLAN_CHUNK}};
    for (const auto &c : flat) {
        const BmPassPlan P = bm_plan_pass(batch(Stage::Slices, {seg(c.nq, 4)}));
        CHECK(P.slices_flat && P.dense && P.lanes == -1 && P.chunk == c.chunk);
        CHECK(P.search_lds == 30000 && P.sgrid % 8 == 0 && (int64_t)P.sgrid >= P.max_items);
        // (the item bound counts three slots of padding per tile and unit, padded or not)
        CHECK(P.max_items == 2 * ((c.nq + 3 * (int64_t)(PLAN_NB >> 4) * P.ntp) / c.chunk) + 2 + (PLAN_NB >> 4) + 2);
    }
    // (the cell and dense stages keep their item size whatever the batch)
    CHECK(bm_plan_pass(batch(Stage::Cells, {seg(4 * M, 3)})).chunk == 2 * PLAN_CHUNK);
    CHECK(bm_plan_pass(batch(Stage::Dense, {seg(4 * M, 3)})).chunk == 4 * PLAN_CHUNK);
    // the lanes-per-run kernels (ivl.sl_flat = 0): items of PLAN_CHUNK queries under the same rule, lanes by the shortest expected run
    BmPlanIn in = batch(Stage::Slices, {seg(8 * M, 4)});
    in.knobs.sl_flat = 0;
    BmPassPlan P = bm_plan_pass(in);
    CHECK(!P.slices_flat && !P.dense && P.chunk == 16384 && P.bytes.cnt16 == 0 && P.bytes.runT != 0);
    CHECK(P.max_items == (PLAN_NB + 2) + 2 * (8 * M / 16384) + 2);
    in.seg[0].nq = 160ll * PLAN_CHUNK;
    CHECK(bm_plan_pass(in).chunk == PLAN_CHUNK);
    struct { int64_t run; int lanes; } by_run[] = {{1000, 0}, {96, 0}, {95, 64}, {40, 64}, {39, 16}, {1, 16}};
    for (const auto &c : by_run) {
        in.seg[0].sl_run = c.run;
        CHECK(bm_plan_pass(in).lanes == c.lanes);
    }
    in.seg[0].sl_run = 1000;
    in.seg.push_back(seg(8 * M, 4));  // (sl_run 20: the batch's shortest run decides)
    CHECK(bm_plan_pass(in).lanes == 16);
    // a small unit still gets the flat walk's 4 KB
    in = batch(Stage::Slices, {seg(8 * M, 4)});
    in.seg[0].sl_lds = 1000;
    CHECK(bm_plan_pass(in).search_lds == 4096);
    in.knobs.sl_flat = 0;
    CHECK(bm_plan_pass(in).search_lds == 1000);
}

static void tile_numbering()
{
    for (int64_t big : {13 * M, 70 * M}) {
        const std::vector<int64_t> nqs = {1, 64 * 16384 + 1, 0, big, 16384 * 64, 5};
        std::vector<BmPlanSegIn> segs;
        for (int64_t nq : nqs) segs.push_back(seg(nq, 3));
        const BmPassPlan P = bm_plan_pass(batch(Stage::Cells, segs));
        const int64_t tile = (int64_t)1 << P.tile_log2;
        CHECK((big == 70 * M) == (P.tile_log2 == 15));
        int64_t sum = 0;
        for (size_t i = 0; i < nqs.size(); i++) {
            const BmPlanSegOut &o = P.seg[i];
            CHECK(o.tile0 % PLAN_GROUP_TILES == 0 && o.tile_end % PLAN_GROUP_TILES == 0);
            CHECK(o.ntiles == (nqs[i] + tile - 1) / tile && o.tile0 + o.ntiles <= o.tile_end && o.tile_end - o.tile0 - o.ntiles < PLAN_GROUP_TILES);
            CHECK(o.tile0 == (i ? P.seg[i - 1].tile_end : 0));
            sum += o.tile_end - o.tile0;
        }
        CHECK(P.ntp == sum && P.ntp == P.seg.back().tile_end && P.ngroups * (int64_t)PLAN_GROUP_TILES == P.ntp);
        // what is sized by the tiles
        const size_t T = (size_t)P.ntp, n = nqs.size();
        CHECK(P.pad && P.bytes.recs == T * (size_t)(tile + PLAN_PAD_ROOM) * 4 && P.bytes.cnt16 == T * (size_t)(tile + PLAN_PAD_ROOM) * 2);
        CHECK(P.bytes.tend == T * 4 && P.bytes.slots == T * (size_t)tile * 2 && P.bytes.tbl == T * PLAN_NB * 2 && P.bytes.unitT == T * (PLAN_NB + 1) * 2);
        CHECK(P.bytes.runT == 0 && P.bytes.grpcnt == (size_t)P.ngroups * PLAN_NB * 4 && P.bytes.unitcnt == P.bytes.grpcnt);
        CHECK(P.bytes.items == (size_t)(P.max_items + 2) * 16);
        CHECK(P.seg_bytes == n * SEG_BYTES && P.tile_off % 16 == 0 && P.tile_off >= n * (SEG_BYTES + 8) && P.tile_off < n * (SEG_BYTES + 8) + 16);
        CHECK(P.bytes.params == P.tile_off + T * 2);
        CHECK(P.n_zero == (int)n * PLAN_SLOTS + 8 && P.bytes.p_slots == (size_t)P.n_zero * 8);
    }
    // the clumped layout's unit image is beyond what the 512-thread walk loads (80 KB)
    BmPlanIn in = batch(Stage::OffsetCells, {seg(13 * M, 3)});
    in.seg[0].stride = 5120;
    BmPassPlan P = bm_plan_pass(in);
    CHECK(!P.big && P.search_lds == 81920);
    in.seg[0].stride = 5121;
    CHECK(bm_plan_pass(in).big);
    in.stage = Stage::Cells;
    CHECK(!bm_plan_pass(in).big);
}

static void order_and_feedback()
{
    // one index: the order is watched; the feedback word moves the streak when it answers a later pass than the last one seen
    BmPlanIn in = batch(Stage::Cells, {seg(13 * M, 3)});
    in.order_seq = 9, in.order_seen = 3, in.unsorted_streak = 1, in.order_skip = false;
    in.fb_order = (4ull << 1) | 1ull;  // pass 4 was not sorted: the second in a row
    BmPassPlan P = bm_plan_pass(in);
    CHECK(P.order_aware && P.order_seen == 4 && P.unsorted_streak == 2 && P.order_skip && P.probe_rides && !P.order_check && P.fold_params && !P.probe_first);
    CHECK(P.bytes.bs_plan == 0);
    in.fb_order = 4ull << 1;  // pass 4 was sorted: the exact check stays, with the walk from the cell images behind it
    P = bm_plan_pass(in);
    CHECK(P.order_seen == 4 && P.unsorted_streak == 0 && !P.order_skip && P.order_check && !P.probe_rides && !P.fold_params);
    CHECK(P.sorted_on_cells && !P.multi_sorted);
    const size_t units = PLAN_NB >> 3;
    CHECK(P.sorted_items == units + 4 + 13 * M / (2 * PLAN_CHUNK) && P.bytes.bs_plan == (units + 2) * 4 + 16 + (P.sorted_items + 1) * 16);
    in.order_skip = true, in.unsorted_streak = 2;  // a sorted answer brings the check back
    CHECK(bm_plan_pass(in).order_check);
    in.fb_order = (3ull << 1) | 1ull;  // an answer the handle has seen already changes nothing
    P = bm_plan_pass(in);
    CHECK(P.order_seen == 3 && P.unsorted_streak == 2 && P.order_skip && P.probe_rides);
    // offset cells walk sorted batches in items of PLAN_CHUNK; other stages have no walk from images
    in = batch(Stage::OffsetCells, {seg(13 * M, 3)});
    in.order_skip = false, in.unsorted_streak = 0, in.fb_order = 0;
    P = bm_plan_pass(in);
    CHECK(P.order_check && P.sorted_on_cells && P.sorted_chunk == (unsigned)PLAN_CHUNK);
    in.stage = Stage::Dense;
    P = bm_plan_pass(in);
    CHECK(P.order_check && !P.sorted_on_cells && P.bytes.bs_plan == 0);
    // a handle's first batch: the probe is asked alone, and a descent among its starts drops the check from this very pass
    in = batch(Stage::Cells, {seg(13 * M, 3)});
    in.order_seq = in.order_seen = 0, in.unsorted_streak = 0, in.order_skip = false, in.fb_order = 0;
    P = bm_plan_pass(in);
    CHECK(P.probe_first && P.order_check && !P.fold_params && P.bytes.bs_plan != 0);
    bm_plan_set_order_skip(P, true, in.knobs);
    CHECK(!P.order_check && P.probe_rides && P.fold_params && P.bytes.bs_plan == 0);
    // ivl.order_skip = 0: always check
    in = batch(Stage::Cells, {seg(13 * M, 3)});
    in.knobs.order_skip = 0;
    P = bm_plan_pass(in);
    CHECK(P.order_check && !P.probe_rides && !P.fold_params);
    in.order_seq = 0;
    CHECK(!bm_plan_pass(in).probe_first);
    // ivl.sorted_path = 0: nobody watches
    in = batch(Stage::Cells, {seg(13 * M, 3)});
    in.knobs.sorted_path = 0;
    P = bm_plan_pass(in);
    CHECK(!P.order_aware && !P.order_check && !P.probe_rides && P.fold_params && P.unsorted_streak == 2);
    // ivl.sorted_cells = 0: the first-generation kernel behind the check
    in = batch(Stage::Cells, {seg(13 * M, 3)});
    in.order_skip = false, in.unsorted_streak = 0, in.knobs.sorted_cells = 0;
    P = bm_plan_pass(in);
    CHECK(P.order_check && !P.sorted_on_cells && P.bytes.bs_plan == 0);

    // 8-bit counts: once more than one count in 64 (and more than 4096) did not fit, the first index keeps 16-bit counts
    in = batch(Stage::Cells, {seg(13 * M, 3)});
    in.w8_queries = 100 * M, in.fb_wide_counts = 100 * M / 64;
    P = bm_plan_pass(in);
    CHECK(P.w8 && !P.w8_trip);
    in.fb_wide_counts = 100 * M / 64 + 1;
    P = bm_plan_pass(in);
    CHECK(!P.w8 && P.w8_trip);
    in.w8_queries = 1000, in.fb_wide_counts = 4096;
    CHECK(bm_plan_pass(in).w8);
    in.fb_wide_counts = 4097;
    CHECK(!bm_plan_pass(in).w8);
    in.fb_wide_counts = 0, in.seg[0].w8_off = true;
    P = bm_plan_pass(in);
    CHECK(P.w8_asked && !P.w8 && !P.w8_trip);
    // the clumped layout never predicts narrow counts
    in = batch(Stage::OffsetCells, {seg(13 * M, 3)});
    CHECK(bm_plan_pass(in).w8);
    in.seg[0].bo_state = 2;
    CHECK(!bm_plan_pass(in).w8);
    // ivl.bd_w8: 0 = never, 1 = whenever the layout allows
    in.knobs.bd_w8 = 1;
    CHECK(bm_plan_pass(in).w8);
    in = batch(Stage::Cells, {seg(13 * M, 3)});
    in.knobs.bd_w8 = 0;
    P = bm_plan_pass(in);
    CHECK(!P.w8 && !P.w8_asked);
    in.knobs.bd_w8 = 1, in.seg[0].n = 90 * M, in.seg[0].w8_off = true;
    CHECK(bm_plan_pass(in).w8);
    in.seg[0].f = 0;  // (packed runs: the layout does not allow them)
    CHECK(!bm_plan_pass(in).w8);
    in.seg[0].f = 3, in.seg[0].want_counts = false, in.seg[0].want_total = true;  // (the total-only walk stores no counts)
    CHECK(!bm_plan_pass(in).w8);
    CHECK(!bm_plan_pass(batch(Stage::Dense, {seg(13 * M, 3)})).w8_asked);
}

static void forced_knobs()
{
    // ivl.bm_variant: the tile shape whatever the batch size
    for (int v = 0; v <= 2; v++) {
        BmPlanIn in = batch(Stage::Slices, {seg(v == 2 ? 3 * M : 100 * M, 4)});
        in.knobs.bm_variant = v;
        const BmPassPlan P = bm_plan_pass(in);
        CHECK(P.variant == v && P.tile_log2 == (v == 2 ? 15 : 14) && bm_plan_variant(in) == v);
    }
    BmPlanIn in = batch(Stage::Cells, {seg(100 * M, 3)});
    in.knobs.bm_variant = 0;
    BmPassPlan P = bm_plan_pass(in);
    CHECK(P.variant == 0 && P.pad);  // (units of 8 buckets; a thread of the 512-thread shape owns four)
    in.knobs.bm_variant = 1;
    CHECK(bm_plan_pass(in).variant == 1);
    // ivl.bd_chunk: the item size of every walk with counts out of place, the sorted walk included; the small-batch rule stands back
    in = batch(Stage::Slices, {seg(4 * M, 4)});
    in.knobs.bd_chunk = 100000;
    CHECK(bm_plan_pass(in).chunk == 100000);
    in = batch(Stage::Cells, {seg(13 * M, 3)});
    in.knobs.bd_chunk = 30000, in.order_skip = false, in.unsorted_streak = 0, in.fb_order = 0;
    P = bm_plan_pass(in);
    CHECK(P.chunk == 30000 && P.sorted_chunk == 30000u && P.sorted_items == (size_t)(PLAN_NB >> 3) + 4 + 13 * M / 30000);
    in = batch(Stage::Slices, {seg(4 * M, 4)});
    in.knobs.sl_flat = 0, in.knobs.bd_chunk = 100000;  // (not a walk with counts out of place)
    CHECK(bm_plan_pass(in).chunk == 16384);
    // ivl.sl_lanes: 16 or 64 lanes per run, -1 = the flat walk, whatever the run length
    in.seg[0].sl_run = 1000;
    in.knobs.sl_lanes = 16;
    CHECK(bm_plan_pass(in).lanes == 16);
    in.knobs.sl_lanes = 64, in.seg[0].sl_run = 3;
    CHECK(bm_plan_pass(in).lanes == 64);
    in.knobs.sl_lanes = -1;
    CHECK(bm_plan_pass(in).lanes == 0);
}

int main()
{
    tile_shape_and_padding();
    total_only_walk();
    multi_index_batches();
    finds_count_half();
    slices_without_find();
    tile_numbering();
    order_and_feedback();
    forced_knobs();
    std::printf("count plan ok\n");
    return 0;
}
