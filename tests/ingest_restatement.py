"""The dataset ingest restated in numpy alone (no scipy, no sklearn, so it travels wherever the tests run): what
DataPreprocessor._sample_from_clip, MotionPreprocessor, resample_pose_seq, convert_pose_seq_to_dir_vec, make_audio_fixed_length and the
[:n_poses] clipping of SpeechMotionDataset.__getitem__ compute for TED, and beat.py:365-404 with process_cache.py:38-45 for BEAT.

Intermediate dtypes follow the reference where its own code fixes them (the interpolation is float64 on float32 frames and is cast
back to float32; bone differences are float32, their normalisation float64); ``dtype=np.float64`` on the BEAT chain gives the number
a float32 result is measured against.

Tolerances against fixture G23 (tests/test_ingest_host.py), recorded here:
  POSE_TOL   resampled poses: 2^-23 * 4, one float32 unit in the last place of a coordinate below 4 (scipy forms slope * dx + y_lo
             in float64 exactly as done here; the bound only allows for a differently rounded cast)
  VEC_TOL    directions: 2 * POSE_TOL (a difference of two coordinates) over the shortest non-zero bone of the fixture, which the
             generator asserts to be >= 0.01; the normalisation itself is float64 on both sides
  ROT_TOL    BEAT rot6d in float64 against the reference's float32: 4 float32 roundings of values below 1 in a row (degrees ->
             radians, sin / cos, product, sum), 4 * 2^-24 * amplification by |angle| <= pi: 1e-6
"""
import math

import numpy as np

DIR_VEC_PAIRS = [(0, 1, 0.26), (1, 2, 0.18), (2, 3, 0.14), (1, 4, 0.22), (4, 5, 0.36), (5, 6, 0.33), (1, 7, 0.22), (7, 8, 0.36), (8, 9, 0.33)]
VERDICTS = ("PASS", "pose", "spine angle", "motion", "words")
POSE_TOL = 4.0 * 2.0 ** -23
VEC_TOL = 2 * POSE_TOL / 0.01
ROT_TOL = 1e-6


def fixture_audio(b, L):
    """Recording b's waveform in fixture G23: every sample is its own index (plus 100000 b), exact in float32.  An audio window is a
    gather, so this input shows every index of it, and the fixture stores the reference's windows as first differences."""
    assert 100000 * b + L < 2 ** 24
    return (np.arange(L, dtype=np.int64) + 100000 * b).astype(np.float32)


def decode_audio(first, delta):
    """the windows of the fixture: first sample and int8 first differences -> float32 [W, n]"""
    return np.concatenate([first[:, None].astype(np.int64), delta.astype(np.int64)], 1).cumsum(1).astype(np.float32)


def resample_table(n, duration, fps):
    """np.arange(0, n, n / (duration * fps)) and interp1d's bracketing: (x_new, lo, frac)."""
    x_new = np.arange(0, n, n / (duration * fps))
    idx = np.clip(np.searchsorted(np.arange(0, n), x_new), 1, n - 1)
    lo = idx - 1
    return x_new, lo.astype(np.int64), x_new - lo


def resample_pose_seq(poses, duration, fps):
    x_new, lo, frac = resample_table(len(poses), duration, fps)
    y_lo, y_hi = poses[lo], poses[lo + 1]
    slope = (y_hi - y_lo).astype(np.float64)             # interp1d: the frames' own dtype, then / (x_hi - x_lo) = 1 as int64 -> float64
    out = slope * frac.reshape((-1,) + (1,) * (poses.ndim - 1)) + y_lo
    return out.astype(poses.dtype)


def convert_pose_seq_to_dir_vec(pose):
    """[T, 10, 3] -> [T, 9, 3] float64; a zero norm divides by 1"""
    pose = pose.reshape(pose.shape[0], -1, 3)
    out = np.zeros((pose.shape[0], len(DIR_VEC_PAIRS), 3))
    for i, (a, b, _) in enumerate(DIR_VEC_PAIRS):
        out[:, i] = pose[:, b] - pose[:, a]
        norm = np.sqrt((out[:, i] * out[:, i]).sum(1))
        norm[norm == 0] = 1.0
        out[:, i] /= norm[:, None]
    return out


def motion_stats(skeletons, mean_pose):
    """MotionPreprocessor's numbers in float64: pose difference, spine max and mean (degrees), left and right wrist variance"""
    sk = np.asarray(skeletons, np.float64).reshape(len(skeletons), -1, 3)
    diff = np.abs(sk - np.asarray(mean_pose, np.float64).reshape(-1, 3)).mean()
    spine = sk[:, 1] - sk[:, 0]
    cos = np.clip(-spine[:, 1] / np.linalg.norm(spine, axis=1), -1.0, 1.0)
    ang = np.rad2deg(np.arccos(cos))
    return np.array([diff, ang.max(), ang.mean(), np.var(sk[:, 6], axis=0).sum(), np.var(sk[:, 9], axis=0).sum()])


THRESHOLDS = np.array([0.02, 30.0, 20.0, 0.0014, 0.0014])


def motion_verdict(stats):
    if stats[0] < 0.02:
        return 1
    if stats[1] > 30 or stats[2] > 20:
        return 2
    if stats[3] < 0.0014 and stats[4] < 0.0014:
        return 3
    return 0


def words_in_range(words, start_time, end_time):
    n = 0
    for w in words:
        if w[-2] >= end_time:
            break
        if w[-1] <= start_time:
            continue
        n += 1
    return n


def symmetric_window(audio, start, length):
    """np.pad(audio, (0, n), mode='symmetric')[start:start + length] for one reflection, as index arithmetic"""
    L = len(audio)
    k = start + np.arange(length)
    assert start >= 0 and start + length <= 2 * L
    return audio[np.where(k >= L, 2 * L - 1 - k, k)]


def ted_windows(K, L, start_time, words, n_ext, stride, fps):
    """the window table of one recording: (start_idx, audio_start, n_pad, has_words)"""
    rows = []
    audio_len = int(n_ext / fps * 16000)
    for i in range(math.floor((K - n_ext) / stride) + 1):
        s = i * stride
        a0 = math.floor(s / K * L)
        has = True if words is None else words_in_range(words, start_time + s / fps, start_time + (s + n_ext) / fps) >= 2
        rows.append((s, a0, max(0, a0 + audio_len - L), has))
    return rows


def ted_ingest(skeletons, audio, start_time, end_time, mean_pose, mean_dir_vec, words=None, n_poses=34, stride=10, fps=15):
    """One recording -> a list with one dict per window, ALL windows: pose_seq [n_poses,30], vec_seq [n_poses,27], audio, stats, verdict"""
    n_ext = int(round(n_poses * 1.25))
    res = resample_pose_seq(skeletons, end_time - start_time, fps)
    out = []
    for s, a0, _, has in ted_windows(len(res), len(audio), start_time, words, n_ext, stride, fps):
        win = res[s:s + n_ext]
        stats = motion_stats(win, mean_pose)
        vec = convert_pose_seq_to_dir_vec(win) - np.asarray(mean_dir_vec, np.float64).reshape(-1, 3)
        out.append({"start_frame": s, "pose_seq": win[:n_poses].reshape(n_poses, -1), "vec_seq": vec[:n_poses].reshape(n_poses, -1),
                    "audio": symmetric_window(audio, a0, int(round(n_poses / fps * 16000))), "stats": stats,
                    "verdict": motion_verdict(stats) if has else 4})
    return out


def beat_windows(n, L, n_poses=34, stride=10, fps=15, sr=16000, clean_first=0, clean_final=0):
    """beat.py:348-395 for one recording: (start_idx, audio_start) per window"""
    seconds = min(n // fps, L // sr)
    s_t, e_t = clean_first, seconds - clean_final
    s_f, e_f = s_t * fps, e_t * fps
    return [(s_f + i * stride, sr * s_t + math.floor(i * stride * sr / fps)) for i in range(math.floor((e_f - s_f - n_poses) / stride) + 1)]


def beat_rot6d(tar_pose, mean_pose, std_pose, dtype=np.float64):
    """[T, J*3] normalised Euler degrees -> [T, J*6]: Rx Ry Rz, its first two rows"""
    e = (np.asarray(tar_pose, dtype) * np.asarray(std_pose, dtype) + np.asarray(mean_pose, dtype)).reshape(-1, 3)
    e = e / dtype(180) * dtype(np.pi)
    s, c = np.sin(e), np.cos(e)
    sx, sy, sz, cx, cy, cz = s[:, 0], s[:, 1], s[:, 2], c[:, 0], c[:, 1], c[:, 2]
    rows = np.stack([cy * cz, -cy * sz, sy, sx * sy * cz + cx * sz, -sx * sy * sz + cx * cz, -sx * cy], 1)
    return rows.reshape(len(tar_pose), -1)
