"""Numpy float64 restatement of the BEAT evaluation metrics (scripts_beat/utils/metric.py): SRGR.run (:27-51), L1div.run (:12-24),
alignment.load_pose (:76-98) with the minima of scipy.signal.argrelextrema(x, np.less, order) in mode='clip', GAHR (:162-174) and the
per-clip score of calculate_align (:176-193), plus what fixture G21 (tests/golden/make_golden_beat_metrics.py) and its tests share.
Not a test module.  Pinned to the reference's own classes by tests/test_beat_metrics_host.py before anything on the GPU is compared
with it; it loops over clips as the reference's scripts do.
"""
import os

import numpy as np

T, V = 34, 33
SERIES_JOINTS = (4, 3, 5, 26, 25, 27)     # load_pose's return order: right arm, shoulder, wrist, left arm, shoulder, wrist
SRGR_THRESHOLD, SRGR_SCALE = 4.0, 1 / 0.165
SIGMA, ORDER, FPS = 0.3, 2, 15
SEED_TARGET, SEED_SEMANTIC, SEED_ONSETS = 20, 21, 22
TARGET_NOISE = 0.04
# a comparison fp32 rounding can flip is left out of the entrywise checks
SRGR_MARGIN = 0.03        # degrees: six angles at the 5e-3 degree Euler tolerance of tests/test_post.py
BEAT_MARGIN = 0.035       # degrees: twice sqrt(3) * 1e-2, the velocity tolerance on either side of a compared pair
VEL_TOL = 0.0175          # degrees: sqrt(3) * 1e-2
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "beat_metrics_golden.npz")


def fixture_inputs(sample):
    """The seeded inputs of G21 from the committed sampler output [4, 47, 6, 34]: the target in the reference layout, the semantic
    weights [4, 34] and the ragged onset times."""
    B = sample.shape[0]
    target = (sample + TARGET_NOISE * np.random.default_rng(SEED_TARGET).standard_normal(sample.shape)).astype(np.float32)
    semantic = (np.random.default_rng(SEED_SEMANTIC).integers(0, 11, size=(B, T)) / 10.0).astype(np.float32)
    rng = np.random.default_rng(SEED_ONSETS)
    onsets = [np.sort(rng.uniform(0.0, 2.2, size=int(rng.integers(3, 9)))).astype(np.float32) for _ in range(B)]
    return target, semantic, onsets


def srgr_success(pred, target, threshold=SRGR_THRESHOLD, joints=47):
    """(success [rows, J] bool, diff [rows, J]) of Euler planes [..., J*3]."""
    p = np.asarray(pred, np.float64).reshape(-1, joints, 3)
    t = np.asarray(target, np.float64).reshape(-1, joints, 3)
    diff = np.abs(p - t).sum(2)
    return diff < threshold, diff


def srgr_rate(success, semantic, scale=SRGR_SCALE):
    return float((success * np.asarray(semantic, np.float64).reshape(-1)[:, None] * scale).mean())


def srgr_clip_sums(success, semantic, scale=SRGR_SCALE):
    """Per clip, the sum over (frame, joint) of success * semantic * scale: what srgr_sum holds."""
    w = success.reshape(-1, T, success.shape[-1]) * np.asarray(semantic, np.float64).reshape(-1, T)[:, :, None] * scale
    return w.sum((1, 2))


def l1div_sum(rows):
    x = np.asarray(rows, np.float64)
    return float(np.abs(x - x.mean(0)).sum())


def velocities(euler, joints=SERIES_JOINTS):
    """euler [34, J*3] -> [6, 33]: the norm of the frame-to-frame difference of each series joint's three angles."""
    e = np.asarray(euler, np.float64)
    return np.stack([np.linalg.norm(np.diff(e[:, 3 * j:3 * j + 3], axis=0), axis=1) for j in joints])


def minima(x, order=ORDER):
    """Indices i with x[i] < x[clip(i - k)] and x[i] < x[clip(i + k)] for k = 1..order."""
    x = np.asarray(x)
    n = len(x)
    keep = np.ones(n, bool)
    idx = np.arange(n)
    for k in range(1, order + 1):
        keep &= (x < x[np.clip(idx - k, 0, n - 1)]) & (x < x[np.clip(idx + k, 0, n - 1)])
    return np.nonzero(keep)[0]


def minima_margin(x, order=ORDER):
    """Per frame, the smallest |x[i] - x[neighbour]| over the pairs the test compares (end frames, compared with themselves: 0)."""
    x = np.asarray(x, np.float64)
    n = len(x)
    idx = np.arange(n)
    m = np.full(n, np.inf)
    for k in range(1, order + 1):
        m = np.minimum(m, np.minimum(np.abs(x - x[np.clip(idx - k, 0, n - 1)]), np.abs(x - x[np.clip(idx + k, 0, n - 1)])))
    return m


def beat_masks(vel, order=ORDER):
    out = np.zeros(vel.shape, bool)
    for s, x in enumerate(vel):
        out[s, minima(x, order)] = True
    return out


def gahr(beat_times, onset_times, sigma=SIGMA):
    """GAHR(a, b, sigma): mean over b of exp(-min_a |a - b|^2 / (2 sigma^2)); no a leaves the minimum infinite (0)."""
    a = np.asarray(beat_times, np.float64).reshape(-1)
    total = 0.0
    for b in np.asarray(onset_times, np.float64).reshape(-1):
        d = np.abs(a - b).min() if a.size else np.inf
        total += np.exp(-(d * d) / (2 * sigma * sigma))
    return total / len(onset_times)


def score_batch(pred, target, semantic, onsets, joints=47, series=SERIES_JOINTS, order=ORDER, sigma=SIGMA, fps=FPS, align_series=2,
                threshold=SRGR_THRESHOLD, scale=SRGR_SCALE):
    """One batch through all of it, clip by clip: what ls_beat_metrics returns, in float64."""
    B = len(pred)
    out = {"vel": np.zeros((B, 6, V)), "beat_mask": np.zeros((B, 6, V), bool), "align": np.zeros(B)}
    if target is not None:
        out["success"], out["diff"] = (a.reshape(B, T, joints) for a in srgr_success(pred, target, threshold, joints))
        sem = np.ones((B, T)) if semantic is None else semantic
        out["srgr_sum"] = srgr_clip_sums(out["success"], sem, scale)
        out["rate"] = srgr_rate(out["success"].reshape(-1, joints), sem, scale)
    for b in range(B):
        out["vel"][b] = velocities(pred[b], series)
        out["beat_mask"][b] = beat_masks(out["vel"][b], order)
        if onsets is not None:
            out["align"][b] = gahr(np.nonzero(out["beat_mask"][b, align_series])[0] / fps, onsets[b], sigma)
    return out
