"""Restatement of the post-processing and the scores of a stitched timeline of N frames: the reference's loop bodies with the clip
length 34 replaced by N (scripts/test_RAG_ted.py:84-123, scripts_beat/utils/metric.py).  Not a test module.  Everything that is
already length-generic is taken from where it is pinned to the reference -- ``oracle.rag_oracle.ted_post`` / ``beat_post`` (G9, G10) and
the functions of tests/beat_metrics_restatement.py (G21) -- and only what holds a literal 34 is restated here: the TED beat loop, the
per-clip SRGR sums and ``score_batch``.  tests/test_timeline_host.py pins these to the 34-frame restatements at N = 34.
"""
import os

import numpy as np

import beat_metrics_restatement as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TED_FPS, TED_SIGMA, HOP = 15.0, 0.1, 512
CASES = ("G22_ddim100_skip95_timeline", "G22_ddpm6_timeline", "G22_sag_ddim100_skip95_timeline")


def g22(dataset):
    z = np.load(os.path.join(GOLDEN, f"{dataset}_golden_long.npz"))
    return {k: z[k] for k in CASES}


def ted_beat_mask(angle_diff, thres):
    """test_RAG_ted.py:104-111 over a curve [B, N]: t in [2, N - 2]."""
    d = np.asarray(angle_diff)
    N = d.shape[1]
    mask = np.zeros(d.shape, bool)
    for t in range(2, N - 1):
        c, l, r = d[:, t], d[:, t - 1], d[:, t + 1]
        mask[:, t] = (c < l) & (c < r) & ((l - c >= thres) | (r - c >= thres))
    return mask


def ted_beat_margin(angle_diff, thres):
    """Per frame t in [2, N - 2], the distance of the beat decision from its nearest boundary: of the two strict comparisons and, where
    both hold, of the larger drop from the threshold (inf elsewhere)."""
    d = np.asarray(angle_diff, np.float64)
    N = d.shape[1]
    m = np.full(d.shape, np.inf)
    for t in range(2, N - 1):
        c, l, r = d[:, t], d[:, t - 1], d[:, t + 1]
        m[:, t] = np.minimum(np.minimum(np.abs(l - c), np.abs(r - c)), np.abs(np.maximum(l - c, r - c) - thres))
    return m


def ted_post(timeline):
    """oracle ted_post on [B, 9, 3, N] with the beat loop at N frames."""
    from livelyspeaker_amd import postprocess as pp
    from oracle import rag_oracle as orc
    o = orc.ted_post(timeline, pp.TED_MEAN_DIR_VEC, pp.TED_ANGLE_PAIRS, pp.TED_CHANGE_ANGLE, pp.TED_BEAT_THRES, pp.TED_DIR_VEC_PAIRS)
    o["beat_mask"] = ted_beat_mask(o["angle_diff"], pp.TED_BEAT_THRES)
    return o


def srgr_clip_sums(success, semantic, scale=R.SRGR_SCALE):
    """success [B, N, J], semantic [B, N] -> [B]."""
    return (success * np.asarray(semantic, np.float64)[:, :, None] * scale).sum((1, 2))


def score_batch(pred, target, semantic, onsets, joints=47, series=R.SERIES_JOINTS, order=R.ORDER, sigma=R.SIGMA, fps=R.FPS, align_series=2,
                threshold=R.SRGR_THRESHOLD, scale=R.SRGR_SCALE):
    """R.score_batch on Euler planes [B, N, joints*3]: what ls_beat_metrics_timeline returns, in float64."""
    B, N = pred.shape[0], pred.shape[1]
    out = {"vel": np.zeros((B, 6, N - 1)), "beat_mask": np.zeros((B, 6, N - 1), bool), "align": np.zeros(B)}
    if target is not None:
        out["success"], out["diff"] = (a.reshape(B, N, joints) for a in R.srgr_success(pred, target, threshold, joints))
        sem = np.ones((B, N)) if semantic is None else semantic
        out["srgr_sum"] = srgr_clip_sums(out["success"], sem, scale)
        out["rate"] = R.srgr_rate(out["success"].reshape(-1, joints), sem, scale)
    for b in range(B):
        out["vel"][b] = R.velocities(pred[b], series)
        out["beat_mask"][b] = R.beat_masks(out["vel"][b], order)
        if onsets is not None:
            out["align"][b] = R.gahr(np.nonzero(out["beat_mask"][b, align_series])[0] / fps, onsets[b], sigma)
    return out


def onset_slab(rng, batch, cols, counts, max_frame):
    """A slab as ls_onsets writes it: sorted frames in the first counts[b] entries of row b, -1 after them."""
    slab = np.full((batch, cols), -1, np.int32)
    for b, n in enumerate(counts):
        slab[b, :n] = np.sort(rng.integers(0, max_frame, size=n))
    return slab, np.asarray(counts, np.int32)


def slab_times(slab, counts, sr=16000):
    """The onset times BeatConsistency.push takes: frame * 512 / sr per clip, as audio_onsets.onset_times forms them."""
    return [slab[b, :int(n)].astype(np.int64) * HOP / float(sr) for b, n in enumerate(counts)]
