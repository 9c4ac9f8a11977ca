"""
What tests/test_pwm_hits_kernel_host.py and tests/test_gpu_pwm_hits.py share (a helper: no tests here, no GPU): the expected
list of hits from the planes of the existing models, and the comparison.  The planes are those of pwm_model.Scores.scores or of
pwm_cases.MODEL.planes; an element is a hit when it is scored, its score is not a NaN and score >= threshold[m] in float32.
"""
import numpy as np

import pwm_model as P

INF = np.float32(np.inf)


def offsets_of(lengths):
    return np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)


def thresholds_of(n_mats, t):
    return np.broadcast_to(np.asarray(t, dtype=np.float32), (n_mats,)).copy()


def expected(planes, offsets, thresholds, ok=None):
    """planes float32 [n_mats, total] (NaN where unscoreable), offsets int64 [n + 1]; ok: where the model keeps the sum and the
    scoreable flag apart (pwm_cases.MODEL.planes) -> (mat_hits int64 [n_mats + 1], rows int32, pos int32, score float32)"""
    thresholds = thresholds_of(len(planes), thresholds)
    offsets = np.asarray(offsets, dtype=np.int64)
    rows, pos, score, mat_hits = [], [], [], [0]
    for m, plane in enumerate(planes):
        with np.errstate(invalid="ignore"):
            hit = ~np.isnan(plane) & (plane >= thresholds[m])
        if ok is not None:
            hit &= ok[m]
        at = np.flatnonzero(hit)
        r = np.searchsorted(offsets, at, side="right") - 1  # (the last row that begins at or before: empty rows before it are skipped)
        rows.append(r), pos.append(at - offsets[r]), score.append(plane[at])
        mat_hits.append(mat_hits[-1] + len(at))
    cat = lambda parts, dtype: np.concatenate(parts).astype(dtype) if parts else np.zeros(0, dtype=dtype)  # noqa: E731
    return np.array(mat_hits, dtype=np.int64), cat(rows, np.int32), cat(pos, np.int32), cat(score, np.float32)


def assert_hits(got, want, where=""):
    """counts, rows and positions exactly, scores by their 32 bits"""
    for k, name in enumerate(("mat_hits", "rows", "pos")):
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), (where, name, got[k][:8], want[k][:8], len(got[k]), len(want[k]))
    assert got[3].dtype == np.float32 and np.array_equal(P.bits(got[3]), P.bits(want[3])), (where, "score")


def occurring(planes):
    """per matrix a score that occurs in its plane (the median of those that are numbers; -inf where there is none), so that the
    >= boundary is a hit"""
    out = []
    for plane in planes:
        v = np.sort(plane[~np.isnan(plane)])
        out.append(v[len(v) // 2] if len(v) else -INF)
    return np.array(out, dtype=np.float32)
