#!/usr/bin/env python3
"""Golden vectors for the BEAT evaluation metrics (fixture G21), produced by EXECUTING the reference's own classes at generation time:
scripts_beat/utils/metric.py (L1div.run, SRGR.run, alignment.load_pose, alignment.GAHR, alignment.motion_frames2time) and
scripts_beat/dataloaders/data_tools.py (FIDCalculator.frechet_distance, FIDCalculator.get_diversity), on Euler planes made by
scripts_beat/dataloaders/rot_utils.py as in make_golden_post_beat.py.  Build container only.

Third-party packages those modules import at module level and this path never reaches (librosa, lmdb, fasttext, loguru, IPython) get
empty stand-ins in sys.modules, as make_golden_eval.py does for umap.  alignment.calculate_align would call librosa.frames_to_time on
its audio argument, so GAHR is called directly with onset TIMES; that one librosa line, with the defaults the reference calls it with,
is `frames * 512 / 22050` and is restated here only to record its values.

Inputs: the committed sampler output beat_golden.npz["G3_ddpm50_final"] (4 clips) as the generated batch; the same array plus
0.04 * N(0, 1) as the target (the committed outputs are noise-like, so any other committed array would succeed nowhere); seeded
semantic weights from {0, 0.1, ..., 1} and 3 to 8 seeded onset times in [0, 2.2] s per clip (tests/beat_metrics_restatement.py).

A comparison fp32 rounding can flip is marked in two exclusion masks, and the conditions under which the fixture is usable are
asserted here, on the reference alone.
"""
import os
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.dont_write_bytecode = True
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, "/root/reference/scripts_beat")
for name in ("librosa", "librosa.display", "lmdb", "fasttext", "loguru", "IPython"):
    try:
        __import__(name)
    except ImportError:
        sys.modules[name] = types.ModuleType(name)
if not hasattr(sys.modules["loguru"], "logger"):
    sys.modules["loguru"].logger = None
import numpy as np                                  # noqa: E402
import torch                                        # noqa: E402
from dataloaders import data_tools, rot_utils       # noqa: E402
from utils import metric                            # noqa: E402
import beat_metrics_restatement as R                # noqa: E402


def euler_deg(sample):
    B = sample.shape[0]
    decoded = torch.from_numpy(sample).permute(0, 3, 1, 2).reshape(B, 34, 47 * 6)                          # test_RAG_beat.py:86
    return (rot_utils.matrix_to_euler_angles(rot_utils.rotation_6d_to_matrix(decoded.reshape(-1, 34, 47, 6)), "XYZ").flatten(2)
            / (np.pi) * 180).numpy().astype(np.float32), decoded.numpy()                                   # :101


sample = np.load(os.path.join(HERE, "beat_golden.npz"))["G3_ddpm50_final"]         # [4, 47, 6, 34]
B = sample.shape[0]
target, semantic, onsets = R.fixture_inputs(sample)
pred_euler, _ = euler_deg(sample)
target_euler, tar_pose = euler_deg(target)
out = {"pred_euler": pred_euler, "target_euler": target_euler, "tar_pose": tar_pose, "semantic": semantic,
       "onset_times": np.concatenate(onsets), "onset_offsets": np.cumsum([0] + [len(o) for o in onsets]).astype(np.int64)}

# ---- SRGR (test_LivelySpeaker_beat.py:148-154): the batch, then the first two clips again as a second batch for avg() ----
srgr = metric.SRGR(4, 47)
rate = srgr.run(pred_euler.reshape(-1, 141), target_euler.reshape(-1, 141), semantic.flatten())
rate2 = srgr.run(pred_euler[:2].reshape(-1, 141), target_euler[:2].reshape(-1, 141), semantic[:2].flatten())
out["srgr_rate"], out["srgr_rate2"], out["srgr_avg"] = np.float64(rate), np.float64(rate2), np.float64(srgr.avg())
diff = np.sum(abs(pred_euler.reshape(-1, 47, 3) - target_euler.reshape(-1, 47, 3)), 2)                    # metric.py:39
out["success"] = (np.where(diff < srgr.threshold, 1.0, 0.0) > 0).reshape(B, 34, 47)                        # :40
out["srgr_excluded"] = (np.abs(diff.astype(np.float64) - 4.0) < R.SRGR_MARGIN).reshape(B, 34, 47)
assert abs(rate - (out["success"].reshape(-1, 47).astype(np.float64) * semantic.reshape(-1)[:, None] * (1 / 0.165)).mean()) < 1e-12 * rate

# ---- L1div on the batch's Euler rows (run() overwrites its argument: a copy goes in) ----
l1 = metric.L1div()
l1.run(pred_euler.reshape(-1, 141).copy())
out["l1div_sum"], out["l1div_avg"] = np.float64(l1.sum), np.float64(l1.avg())
# the scripts hand run() the fp32 planes, so the sum above is an fp32 (pairwise) one; the same rows as float64 through the same
# method give the number a float64 restatement can be held to
l1 = metric.L1div()
l1.run(pred_euler.reshape(-1, 141).astype(np.float64))
out["l1div_sum_f64"], out["l1div_avg_f64"] = np.float64(l1.sum), np.float64(l1.avg())

# ---- motion beats and the per-clip GAHR value (test_RAG_beat.py:110-113) ----
al = metric.alignment(0.3, 2)
vel = np.zeros((B, 6, 33), np.float64)
beat_mask = np.zeros((B, 6, 33), bool)
beat_excluded = np.zeros((B, 6, 33), bool)
align = np.zeros(B, np.float64)
cols = [slice(3 * j, 3 * j + 3) for j in R.SERIES_JOINTS]
for i in range(B):
    beats = al.load_pose(pred_euler[i], 0, 500, 15, True)
    for s in range(6):
        beat_mask[i, s, beats[s][0]] = True
        d = pred_euler[i][1:, cols[s]] - pred_euler[i][:-1, cols[s]]                                      # metric.py:83, one joint
        vel[i, s] = np.linalg.norm(np.array([d[:, 0], d[:, 1], d[:, 2]]), axis=0)                         # :86-88
        assert np.array_equal(metric.argrelextrema(vel[i, s], np.less, order=2)[0], beats[s][0]), (i, s)
        beat_excluded[i, s] = R.minima_margin(vel[i, s], 2) < R.BEAT_MARGIN
    pose_bt = al.motion_frames2time(np.array([list(beats[2][0])]), 0, 15)                                  # :189-191
    align[i] = al.GAHR(pose_bt, onsets[i], 0.3)
beat_excluded[:, :, [0, 32]] = False                # an end frame is compared with itself: never a beat, nothing to flip
out.update(vel=vel, beat_mask=beat_mask, beat_excluded=beat_excluded, align=align)
frames = np.array([0, 1, 7, 43, 86])
out["frames"], out["frames_time"] = frames, frames * 512 / 22050          # librosa.frames_to_time(frames), defaults sr=22050, hop_length=512

# ---- FID and diversity on the committed BEAT features (eval_beat_golden.npz), as test_RAG_beat.py:118-121 calls them ----
feat = np.load(os.path.join(HERE, "eval_beat_golden.npz"))["beat_feat"]           # [96, 48]
out["fid"] = np.float64(data_tools.FIDCalculator.frechet_distance(feat[:48], feat[48:]))
batches = [feat[i:i + 16] for i in range(0, 96, 16)]
torch.manual_seed(4)
out["diversity"] = np.float64(data_tools.FIDCalculator.get_diversity(batches))

# ---- the conditions under which the fixture is usable ----
share = out["success"].mean()
ex = out["srgr_excluded"]
print(f"success share {share:.3f}; SRGR excluded {ex.mean():.4f} overall, {ex.reshape(B, -1).mean(1).max():.4f} worst clip; "
      f"beat frames excluded {beat_excluded.mean():.4f}; wrist series clean in {int((~beat_excluded[:, 2].any(1)).sum())} of {B} clips")
print("rate", rate, "avg", srgr.avg(), "l1div", l1.avg(), "align", align, "beats/series", beat_mask.sum(2).tolist(), "fid", out["fid"],
      "diversity", out["diversity"])
assert 0.2 <= share <= 0.8
assert ex.mean() <= 0.02 and ex.reshape(B, -1).mean(1).max() <= 0.02
assert beat_excluded.mean() <= 0.02
assert (~beat_excluded[:, 2].any(1)).sum() >= 3
np.savez_compressed(os.path.join(HERE, "beat_metrics_golden.npz"), **out)
print("wrote beat_metrics_golden.npz")
