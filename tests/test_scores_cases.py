"""
CPU-only: the inputs of tests/test_gpu_scores_scale.py (tests/scores_cases.py) have the properties that keep those tests from
passing vacuously.  Every condition is one on tests/scores_model.py alone; a seed that misses one is a reason to change the
generator, not the bound.
"""
import numpy as np
import pytest

import scores_cases as SC
import scores_model as M


@pytest.fixture(scope="module")
def W():
    return SC.world()


@pytest.mark.parametrize("track, starts, ends", [("track", "s", "e"), ("dense", "short_s", "short_e")])
def test_pools_are_order_sensitive(W, track, starts, ends):
    """an ordered float32 chain differs from a tree and from a wide accumulator on at least half of the pool's intervals"""
    s, e = W[starts], W[ends]
    assert len(s) == SC.MAX_UNIQUE
    assert M.fraction_order_sensitive(W[track], s, e) >= 0.5


def test_shared_track_holds_what_the_kernels_must_tell_apart(W):
    t = W["track"]
    assert (t == np.inf).sum() == 12 and (t == -np.inf).sum() == 12 and np.isnan(t).mean() > 0.1
    assert (t == 0).any() and np.signbit(t[t == 0]).any() and SC.is_subnormal(t).any()
    total = M.aggregate(t, W["s"], W["e"])[1]
    assert np.isnan(total).sum() >= 100 and np.isinf(total).sum() >= 20   # sums that turn NaN or infinite on the way
    assert len(W["mask"]) < len(t) < len(W["mask_b"])
    # the short pool: under 130 bases, but for the rows random_intervals stretches to a far end (a thirteenth and a seventeenth)
    assert (SC.clipped_lengths(W["short_s"], W["short_e"]) < 130).mean() > 0.85


def test_one_bucket_pool_is_order_sensitive(W):
    s, e, idx = SC.one_bucket_case()
    assert len(s) <= SC.MAX_UNIQUE and len(idx) == SC.ONE_BUCKET_N
    assert len(set(SC.clipped_lengths(s, e).tolist())) == 1
    assert M.fraction_order_sensitive(W["track"], s, e) >= 0.5


def test_every_large_batch_uses_every_unique_interval():
    batches = list(SC.scatter_batches().items()) + list(SC.wave_stride_batches().items())
    batches += [(SC.count_stride_n(), SC.count_stride_batch()), (SC.ONE_BUCKET_N, SC.one_bucket_case()[2])]
    batches += [(n, idx) for n, idx, _, _ in SC.handle_sequence()]
    assert sorted(n for n, _ in batches)[-1] == SC.CAP_MI355X * 1024 + 3
    for n, idx in batches:
        assert len(idx) == n
        assert np.array_equal(np.unique(idx), np.arange(min(n, SC.MAX_UNIQUE))), n


def test_structural_sizes():
    """the batch sizes against the kernels' geometry (csrc/scores.hpp, csrc/scores.hip), for the cap of an MI355X"""
    cap = SC.CAP_MI355X
    assert {1023, 1024, 1025} <= set(SC.SCATTER_NS) and {2047, 2048, 2049} <= set(SC.SCATTER_NS)  # count: 1024, scatter: 2048 a workgroup
    assert max(SC.SCATTER_NS) > 2048 * 2 and max(SC.SCATTER_NS) % 2048 != 0
    assert SC.count_stride_n(cap) > cap * 1024
    ns = SC.wave_stride_ns(cap)
    assert ns[0] > cap * 4 * 2 and {n % 4 for n in ns[1:]} == {1, 2, 3}
    assert SC.fill_run_n(cap) > cap * 256
    assert len(SC.all_intervals()[0]) == 20301 > cap * 4


def test_bucket_edge_case_holds_every_edge(W):
    s, e = SC.bucket_edge_case()
    clipped, raw = SC.clipped_lengths(s, e), e - s
    have = set(clipped.tolist())
    want = {0, 1, 63, 64, 65, 127, 128, 129} | {k * 64 + d for k in (509, 510, 511, 512) for d in (-1, 0, 1)}
    assert want <= have, sorted(want - have)
    assert max(have) >= 65_000
    for L in SC.KNOB_EDGES:
        assert {L - 1, L, L + 1} <= have, L
        short = (raw >= L) & (clipped < L) & (clipped > 0)
        assert (short & (s < 0)).any() and (short & (e > W["size"])).any(), L
    assert (clipped < 100).sum() >= 300 and (clipped >= 8192).sum() >= 100  # long and short rows, shuffled
    assert M.fraction_order_sensitive(W["dense"], s, e) >= 0.5


def _without_subnormals(track):
    t = track.copy()
    t[SC.is_subnormal(t)] = 0.0
    return t


def test_subnormal_segment_a_depends_on_its_subnormals():
    track, s, e = SC.subnormal_segment("A")
    assert (e - s).min() == 1 and (e - s).max() == 399
    assert SC.is_subnormal(track).mean() >= 0.5
    full, flushed = M.aggregate(track, s, e), M.aggregate(_without_subnormals(track), s, e)
    both = (full[0] != flushed[0]) & (full[1].view(np.uint32) != flushed[1].view(np.uint32))
    assert both.mean() >= 0.9
    assert M.fraction_order_sensitive(track, s, e) >= 0.5


def test_subnormal_segment_b_has_subnormal_sums():
    track, s, e = SC.subnormal_segment("B")
    assert (e - s).min() == 1 and (e - s).max() == 39
    assert SC.is_subnormal(M.aggregate(track, s, e)[1]).mean() >= 0.5


def test_mask_geometry_inputs():
    v = SC.geometry_track()
    assert len(v) == SC.GEOMETRY_SIZE and not np.isnan(v).any() and (v != 0).all()
    for size in SC.MASK_SIZES:
        m = SC.geometry_mask(size)
        assert len(m) == size and m[0] and m[-1] and m[size // 2]
        assert size < 63 or (not m.all() and (~m).any())
    s, e = SC.all_intervals()
    assert (s <= e).all() and s.min() == 0 and e.max() == SC.GEOMETRY_SIZE and len(set(zip(s.tolist(), e.tolist()))) == 20301


def test_fill_case_is_one_long_run_and_a_hundred_short_ones():
    """the host cuts a span list where a span starts before the end of the one before (csrc/scores.hip: bxmi_scores_set_spans)"""
    size, s, e, v = SC.fill_case()
    m = SC.fill_run_n()
    assert len(s) == m + 100 and s[0] < 0 and e[m - 1] > size
    assert (s[1:m] >= e[:m - 1]).all() and (e[:m] - s[:m]).max() >= 64 and set((e[:m] - s[:m])[1:999].tolist()) == {0, 1, 2, 3}
    assert (s[m + 1:m + 50] < s[m:m + 49]).all() and (e[m + 1:m + 50] <= s[m:m + 49]).all()  # descending, disjoint
    assert (s[m + 51:] > s[m + 50:-1]).all() and (s[m + 51:] < e[m + 50:-1]).all()           # ascending, overlapping
    assert np.isnan(v).any() and (v == 0).any()
