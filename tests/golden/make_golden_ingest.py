#!/usr/bin/env python3
"""Golden vectors for the dataset ingest (fixture G23), produced by EXECUTING the reference's own code at generation time:
scripts/data_loader/data_preprocessor.py (DataPreprocessor._sample_from_clip on an instance made without __init__, its txn.put calls
captured), data_loader/motion_preprocessor.py, utils/data_utils.py (resample_pose_seq, convert_pose_seq_to_dir_vec,
make_audio_fixed_length) with the [:n_poses] clipping of SpeechMotionDataset.__getitem__ (lmdb_data_loader.py:166-174) applied to
what was put; for BEAT the three lines of scripts_beat/data_libs/process_cache.py:38-45 through scripts_beat/dataloaders/rot_utils.py.
Build container only.

Stand-ins: lmdb and librosa (imported at module level, never reached) are empty modules; pyarrow's serialize(v).to_buffer() returns v.
numpy >= 1.25 refuses MotionPreprocessor's `ndarray != []`; the subclass below hands it an array whose comparison with an empty
list is True, which is what the numpy the reference was written for answered.  Nothing else of the reference is touched.

The batch (<= 100 raw frames per recording; float32 poses drawn from numpy.random.Generator(PCG64(seed)) as synth.py does):
  0 down    25 -> 15 fps, 2 windows; the bone (2, 3) has length zero in the first raw frames
  1 up      10 -> 15 fps (the tail is extrapolated, frac > 1); its second window holds a single word
  2 exact   resampled length exactly n_ext: one window
  3 short   shorter than n_ext: no window
  4 pad     audio shorter than the motion: the last window reads symmetric padding inside its first 36267 samples
  5 pose, 6 spine, 7 static: one window each with verdict "pose", "spine angle", "motion"
The audio of recording b is its own index ramp (tests/ingest_restatement.py: fixture_audio), so only lengths are stored, and the
reference's audio windows are stored as first differences (int8).

Asserted here, on the reference alone: every statistic of every window lies at least 1 % (relative) from its threshold; the shortest
non-zero bone is >= 0.01; the restatement's verdicts equal the reference's messages.
"""
import importlib.util
import math
import os
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
sys.dont_write_bytecode = True
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(REF, "scripts"))
for name in ("lmdb", "librosa"):
    sys.modules[name] = types.ModuleType(name)


class _Buffer:
    def __init__(self, v):
        self.v = v

    def to_buffer(self):
        return self.v


try:                                     # a current pyarrow has no serialize any more; pandas (under sklearn) wants the real module
    import pyarrow
except ImportError:
    pyarrow = sys.modules["pyarrow"] = types.ModuleType("pyarrow")
pyarrow.serialize = _Buffer

import numpy as np                                                   # noqa: E402
import torch                                                         # noqa: E402
import utils.data_utils as data_utils                                # noqa: E402
from data_loader import data_preprocessor as dp                      # noqa: E402
from data_loader.motion_preprocessor import MotionPreprocessor       # noqa: E402
import ingest_restatement as R                                       # noqa: E402
from livelyspeaker_amd.postprocess import TED_MEAN_DIR_VEC           # noqa: E402

spec = importlib.util.spec_from_file_location("ref_rot_utils", os.path.join(REF, "scripts_beat", "dataloaders", "rot_utils.py"))
rot_utils = importlib.util.module_from_spec(spec)
spec.loader.exec_module(rot_utils)

N_POSES, STRIDE, FPS = 34, 10, 15
N_EXT = int(round(N_POSES * 1.25))
AUDIO_LEN = int(round(N_POSES / FPS * 16000))
SEED = 23000


def rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


class _EmptyListNe(np.ndarray):
    def __ne__(self, other):
        if isinstance(other, list) and not other:
            return True
        return np.ndarray.__ne__(self, other)


MESSAGES = []


class RecordingPreprocessor(MotionPreprocessor):
    def __init__(self, skeletons, mean_pose):
        super().__init__(skeletons, mean_pose)
        self.skeletons = self.skeletons.view(_EmptyListNe)

    def get(self):
        r = super().get()
        MESSAGES.append(r[1])
        return r


class PassAll(MotionPreprocessor):
    """For the second run: with disable_filtering the reference appends the [] a filtered window has become and then fails in
    convert_pose_seq_to_dir_vec, so the data of the filtered windows is taken from a run whose three checks answer False."""

    def __init__(self, skeletons, mean_pose):
        super().__init__(skeletons, mean_pose)
        self.skeletons = self.skeletons.view(_EmptyListNe)

    def check_pose_diff(self, verbose=False):
        return False

    def check_spine_angle(self, verbose=False):
        return False

    def check_static_motion(self, verbose=False):
        return False


class _Txn:
    def __init__(self, puts):
        self.puts = puts

    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False

    def put(self, k, v):
        self.puts.append((k, v.v if isinstance(v, _Buffer) else v))


class _Env:
    def __init__(self):
        self.puts = []

    def begin(self, write=False):
        return _Txn(self.puts)


def preprocessor(mean_pose, mean_dir_vec, disable_filtering):
    p = object.__new__(dp.DataPreprocessor)
    p.n_poses, p.subdivision_stride, p.skeleton_resampling_fps = N_EXT, STRIDE, FPS
    p.mean_pose, p.mean_dir_vec, p.disable_filtering = mean_pose, mean_dir_vec, disable_filtering
    p.spectrogram_sample_length = data_utils.calc_spectrogram_length_from_motion_length(N_EXT, FPS)
    p.audio_sample_length = int(N_EXT / FPS * 16000)
    p.dst_lmdb_env = _Env()
    p.n_out_samples = 0
    return p


# ---- the recordings -------------------------------------------------------------------------------------------------------
mean_pose = data_utils.convert_dir_vec_to_pose(TED_MEAN_DIR_VEC.astype(np.float64)).astype(np.float32)       # [10, 3]
mean_dir_vec = TED_MEAN_DIR_VEC.reshape(-1, 3)


def moving(n, duration, seed, amp=0.1, noise=0.003):
    g = rng(seed)
    t = np.linspace(0.0, duration, n)[:, None, None]
    pose = np.repeat(mean_pose[None].astype(np.float64), n, 0)
    freq, phase = g.uniform(0.4, 1.0, (1, 6, 3)), g.uniform(0, 2 * np.pi, (1, 6, 3))
    pose[:, 4:] += amp * np.sin(2 * np.pi * freq * t + phase)
    return (pose + noise * g.standard_normal(pose.shape)).astype(np.float32)


def words_every(start, stop, step=0.3):
    return [["w%d" % k, start + step * k, start + step * k + 0.25] for k in range(int((stop - start) / step))]


clips = []


def add(name, raw, s_t, e_t, L=None, words=None):
    clips.append({"name": name, "raw": raw, "s_t": s_t, "e_t": e_t, "L": int((e_t - s_t) * 16000) if L is None else L,
                  "words": words_every(s_t, e_t) if words is None else words})


down = moving(100, 4.0, SEED)
down[:13, 3] = down[:13, 2]                                                      # the bone (2, 3) collapses
add("down", down, 2.0, 6.0)
add("up", moving(40, 4.0, SEED + 1), 0.0, 4.0, words=[["a", 0.1, 0.4], ["b", 0.5, 0.6], ["c", 3.0, 3.2]])
add("exact", moving(84, 2.8, SEED + 2), 1.0, 3.8)
add("short", moving(50, 2.0, SEED + 3), 0.0, 2.0)
add("pad", moving(100, 62 / 15, SEED + 4), 0.5, 0.5 + 62 / 15, L=50000)
g = rng(SEED + 5)
add("pose", (mean_pose[None] + 0.004 * g.standard_normal((75, 10, 3))).astype(np.float32), 0.0, 3.0)
tilt = math.radians(35.0)
rot = np.array([[math.cos(tilt), -math.sin(tilt), 0], [math.sin(tilt), math.cos(tilt), 0], [0, 0, 1]])
add("spine", (moving(75, 3.0, SEED + 6).astype(np.float64) @ rot.T).astype(np.float32), 0.0, 3.0)
static = np.repeat(mean_pose[None].astype(np.float64), 75, 0)
static[:, 4:] += 0.06
add("static", (static + 0.002 * rng(SEED + 7).standard_normal(static.shape)).astype(np.float32), 0.0, 3.0)
assert all(len(c["raw"]) <= 100 and c["raw"].dtype == np.float32 for c in clips)

# ---- the reference, twice: as configured (which windows are kept, in which order, and each window's message) and with the three
# checks answering False (the data of every window that has its words) ---------------------------------------------------------
out = {"mean_pose": mean_pose.reshape(-1), "mean_dir_vec": TED_MEAN_DIR_VEC, "n_raw": np.array([len(c["raw"]) for c in clips], np.int32),
       "raw": np.concatenate([c["raw"] for c in clips]), "start_time": np.array([c["s_t"] for c in clips]),
       "end_time": np.array([c["e_t"] for c in clips]), "audio_len": np.array([c["L"] for c in clips], np.int64),
       "word_offsets": np.cumsum([0] + [len(c["words"]) for c in clips]).astype(np.int64),
       "word_times": np.array([[w[1], w[2]] for c in clips for w in c["words"]], np.float64)}
kept_p, all_p = preprocessor(mean_pose, mean_dir_vec, False), preprocessor(mean_pose, mean_dir_vec, True)
win_clip, win_start, verdict, stats_all, kept_rows, data_rows, resampled_len = [], [], [], [], [], [], []
for b, c in enumerate(clips):
    res = data_utils.resample_pose_seq(c["raw"], c["e_t"] - c["s_t"], FPS)
    K = len(res)
    resampled_len.append(K)
    feat = np.zeros((2, data_utils.calc_spectrogram_length_from_motion_length(K, FPS)), np.float16)
    clip = {"skeletons_3d": c["raw"], "audio_feat": feat, "audio_raw": R.fixture_audio(b, c["L"]), "words": c["words"],
            "start_frame_no": 0, "end_frame_no": len(c["raw"]), "start_time": c["s_t"], "end_time": c["e_t"]}
    del MESSAGES[:]
    n_before = len(kept_p.dst_lmdb_env.puts)
    dp.MotionPreprocessor = RecordingPreprocessor
    filtered = kept_p._sample_from_clip("vid%d" % b, clip)
    messages = list(MESSAGES)
    dp.MotionPreprocessor = PassAll
    all_p._sample_from_clip("vid%d" % b, clip)
    m, first_row = 0, len(verdict)
    for i in range(math.floor((K - N_EXT) / STRIDE) + 1):
        s = i * STRIDE
        n_words = len(dp.DataPreprocessor.get_words_in_time_range(c["words"], c["s_t"] + s / FPS, c["s_t"] + (s + N_EXT) / FPS))
        win_clip.append(b)
        win_start.append(s)
        st = R.motion_stats(res[s:s + N_EXT], mean_pose)
        stats_all.append(st)
        if n_words < 2:
            verdict.append(4)
            continue
        verdict.append(R.VERDICTS.index(messages[m]))
        m += 1
        assert R.motion_verdict(st) == verdict[-1], (c["name"], i, st, verdict[-1])
        assert (np.abs(st - R.THRESHOLDS) / R.THRESHOLDS >= 0.01).all(), (c["name"], i, st)
        data_rows.append(len(verdict) - 1)
    assert m == len(messages)
    assert sum(filtered.values()) == sum(1 for v in verdict[first_row:] if v in (1, 2, 3))
    kept_rows += [r for r in range(first_row, len(verdict)) if verdict[r] == 0]
    assert len(kept_p.dst_lmdb_env.puts) - n_before == sum(1 for r in kept_rows if win_clip[r] == b)


def clipped(puts):
    """SpeechMotionDataset.__getitem__'s do_clipping branch on what was put"""
    pose_seq, vec_seq, audio, aux = [], [], [], []
    for _, (word_seq, poses, vec, au, spectrogram, info) in puts:
        audio.append(data_utils.make_audio_fixed_length(au, AUDIO_LEN))
        vec_seq.append(vec[0:N_POSES].reshape(N_POSES, -1))
        pose_seq.append(np.asarray(poses)[0:N_POSES].reshape(N_POSES, -1))
        aux.append(info["start_frame_no"])
    return np.array(pose_seq), np.array(vec_seq), np.array(audio), np.array(aux)


pose_k, vec_k, audio_k, start_k = clipped(kept_p.dst_lmdb_env.puts)
pose_a, vec_a, audio_a, start_a = clipped(all_p.dst_lmdb_env.puts)
assert list(start_k) == [win_start[r] for r in kept_rows] and list(start_a) == [win_start[r] for r in data_rows]
assert np.array_equal(pose_a[[data_rows.index(r) for r in kept_rows]], pose_k)      # the kept windows are those windows, in that order
assert np.array_equal(audio_a[[data_rows.index(r) for r in kept_rows]], audio_k)
delta = np.diff(audio_a.astype(np.int64), axis=1)
assert np.abs(delta).max() == 1 and (audio_a == np.round(audio_a)).all()
out.update(win_clip=np.array(win_clip, np.int32), win_start=np.array(win_start, np.int32), verdict=np.array(verdict, np.int32),
           stats=np.array(stats_all), kept_rows=np.array(kept_rows, np.int32), data_rows=np.array(data_rows, np.int32),
           resampled_len=np.array(resampled_len, np.int32), pose_seq=pose_a.astype(np.float32), vec_seq=vec_a.astype(np.float64),
           audio_first=audio_a[:, 0].astype(np.int64), audio_delta=delta.astype(np.int8))
assert pose_a.dtype == np.float32 or np.array_equal(pose_a.astype(np.float32), pose_a)

# ---- what the batch has to contain ---------------------------------------------------------------------------------------
names = [c["name"] for c in clips]
per_clip = [sum(1 for b in win_clip if b == i) for i in range(len(clips))]
assert resampled_len[names.index("exact")] == N_EXT and per_clip[names.index("exact")] == 1 and per_clip[names.index("short")] == 0
_, _, frac_up = R.resample_table(40, 4.0, FPS)
assert frac_up.max() > 1
assert {1, 2, 3, 4} <= set(verdict) and verdict.count(0) >= 4
pad_rows = [r for r in data_rows if win_clip[r] == names.index("pad")]
assert any((delta[data_rows.index(r)] == -1).any() for r in pad_rows)                # a reflected stretch inside the 36267 samples
bones = np.stack([np.linalg.norm(out["raw"][:, b] - out["raw"][:, a], axis=1) for a, b, _ in R.DIR_VEC_PAIRS], 1)
assert (bones == 0).any() and bones[bones > 0].min() >= 0.01
zero_rows = np.argwhere(np.abs(vec_a.reshape(-1, N_POSES, 9, 3) + mean_dir_vec).max(-1) == 0)
assert len(zero_rows), "no zero-length bone reached a window"
print("windows", len(verdict), "verdicts", verdict, "kept", kept_rows, "resampled", resampled_len, "zero-bone frames", len(zero_rows))

# ---- BEAT: process_cache.py:38-45 on two recordings (every frame once; a window is a slice of rows) -------------------------------
g = rng(SEED + 50)
beat_mean = g.uniform(-30, 30, 141).astype(np.float32)
beat_std = g.uniform(5, 40, 141).astype(np.float32)
for i, n in enumerate((75, 60)):
    tar_pose = g.standard_normal((n, 141)).astype(np.float32)
    pose_euler = (tar_pose * beat_std) + beat_mean
    pose_euler = (torch.Tensor(pose_euler.reshape(-1, 3)) / 180) * np.pi
    rot_matrix = rot_utils.euler_angles_to_matrix(pose_euler, "XYZ")
    rot6d = rot_utils.matrix_to_rotation_6d(rot_matrix)
    out["beat_tar_pose_%d" % i] = tar_pose
    out["beat_rot6d_%d" % i] = rot6d.reshape(tar_pose.shape[0], -1).numpy()
    assert out["beat_rot6d_%d" % i].dtype == np.float32
out.update(beat_mean=beat_mean, beat_std=beat_std, beat_audio_len=np.array([5 * 16000 + 123, 4 * 16000], np.int64))
path = os.path.join(HERE, "ingest_golden.npz")
np.savez_compressed(path, **out)
print("wrote ingest_golden.npz", os.path.getsize(path), "bytes")
