"""Dataset ingest: recorded poses and audio -> the tensors the sampler, the evaluators and the trainer take, cut on the device.

The reference prepares them offline, frame by frame in numpy behind lmdb, pyarrow, sklearn and librosa:
``DataPreprocessor._sample_from_clip`` (scripts/data_loader/data_preprocessor.py:69-167), ``MotionPreprocessor``
(data_loader/motion_preprocessor.py), ``resample_pose_seq`` / ``convert_pose_seq_to_dir_vec`` / ``make_audio_fixed_length``
(utils/data_utils.py:46-120) and the clipping of ``SpeechMotionDataset.__getitem__`` (lmdb_data_loader.py:166-174); for BEAT
``CustomDataset._sample_from_clip`` (scripts_beat/dataloaders/beat.py:365-485) and scripts_beat/data_libs/process_cache.py:38-45.
Here a batch of recordings of different lengths goes in and every window comes out in the layouts the other entry points take:
``ted_ingest`` and ``beat_ingest``.  The drop-ins below carry the reference's names and signatures and run the same kernels.

What is not here: words and vocabulary tensors, mel spectrograms, reading lmdb / BVH / audio files, speaker models.

Departures from the reference.  ``words=None``: every window then counts as having words (the reference drops a window with fewer
than two, and never has no word list).  ``disable_filtering=True`` keeps a filtered window with its data; the reference stores the
empty list its filter left behind and then fails in ``convert_pose_seq_to_dir_vec``.  The interpolation is float32; scipy's is float64
rounded to the poses' dtype (at most one float32 unit in the last place apart on fixture G23, profiles/r18_ingest.md)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from .postprocess import TED_DIR_VEC_PAIRS, ted_post_config

dir_vec_pairs = TED_DIR_VEC_PAIRS
VERDICTS = ("PASS", "pose", "spine angle", "motion", "words")      # LS_INGEST_*: MotionPreprocessor.filtering_message, then "words"
MAX_POSES, MAX_EXT = 64, 128                                          # LS_INGEST_MAX_POSES, LS_INGEST_MAX_EXT
STATS = ("pose_diff", "spine_max_deg", "spine_mean_deg", "left_wrist_var", "right_wrist_var")


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _word_rows(words, batch):
    """words: per recording a sequence of (word, start, end) or (start, end), sorted by start -> (offsets [B+1], times [n,2])."""
    if words is None:
        return None, None
    if len(words) != batch:
        raise ValueError(f"one word list per recording: got {len(words)} for {batch}")
    rows = [[(float(w[-2]), float(w[-1])) for w in clip] for clip in words]
    off = np.cumsum([0] + [len(r) for r in rows]).astype(np.int64)
    flat = np.array([t for r in rows for t in r], np.float64).reshape(-1, 2)
    return off, np.ascontiguousarray(flat)


def ingest_plan(n_raw, start_times, end_times, audio_len, words=None, n_poses=34, n_ext=None, stride=10, fps=15, sr=16000, beat=False):
    """``ls_ingest_plan`` (host only, no GPU): the frame table (clip, lo, hi, frac) of the resampling and the window table (clip,
    first frame, audio_start, n_audio_pad, has_words), as numpy arrays, with ``frame_offsets`` / ``window_offsets`` [B+1].
    ``n_ext`` defaults to ``int(round(n_poses * 1.25))`` (TED) or ``n_poses`` (``beat=True``).  A recording shorter than ``n_ext``
    frames has no window.  Raises ``EngineError`` for what the reference cannot compute either: an empty audio, a symmetric padding
    longer than the audio itself, fewer than 2 raw frames, ``n_poses > n_ext``."""
    B = len(n_raw)
    if n_ext is None:
        n_ext = n_poses if beat else int(round(n_poses * 1.25))
    a = _lib.LsIngestPlanArgs()
    a.batch, a.n_poses, a.n_ext, a.stride, a.beat, a.fps, a.sr = B, int(n_poses), int(n_ext), int(stride), int(bool(beat)), float(fps), float(sr)
    keep = [np.ascontiguousarray(n_raw, np.int32), np.ascontiguousarray(start_times, np.float64),
            np.ascontiguousarray(end_times, np.float64), np.ascontiguousarray(audio_len, np.int64)]
    if any(k.shape != (B,) for k in keep):
        raise ValueError("n_raw, start_times, end_times and audio_len hold one value per recording")
    a.n_raw, a.start_time, a.end_time, a.audio_len = (_ptr(k) for k in keep)
    w_off, w_times = _word_rows(words, B)
    a.word_offsets, a.word_times = _ptr(w_off), _ptr(w_times)
    _lib.call("ls_ingest_plan", C.byref(a))                      # the counts
    F, W = int(a.n_frames), int(a.n_windows)
    out = {"frame_offsets": np.zeros(B + 1, np.int32), "frame_clip": np.zeros(F, np.int32), "frame_lo": np.zeros(F, np.int32),
           "frame_hi": np.zeros(F, np.int32), "frame_frac": np.zeros(F, np.float32), "window_offsets": np.zeros(B + 1, np.int32),
           "win_clip": np.zeros(W, np.int32), "win_first": np.zeros(W, np.int32), "win_audio_start": np.zeros(W, np.int64),
           "win_n_pad": np.zeros(W, np.int32), "win_has_words": np.zeros(W, np.uint8)}
    a.frame_cap, a.window_cap = F, W
    for k, v in out.items():
        setattr(a, k, _ptr(v))
    _lib.call("ls_ingest_plan", C.byref(a))
    out.update(n_frames=F, n_windows=W, n_poses=int(n_poses), n_ext=int(n_ext), n_raw=keep[0], audio_len=keep[3])
    return out


def _cat(m, parts, width):
    """The recordings of one call, concatenated along the first axis: a CUDA tensor if the call is on the device, else numpy."""
    if m.on_device:
        t = m.torch
        return t.cat([t.as_tensor(p).to(device=m.dev, dtype=t.float32).reshape(-1, width) for p in parts])
    return np.concatenate([_lib._np32(p).reshape(-1, width) for p in parts])


def _post_cfg(mean_dir_vec=None):
    cfg = ted_post_config()
    if mean_dir_vec is not None:
        v = np.asarray(_lib._np32(mean_dir_vec)).reshape(-1)
        if v.size != 27:
            raise ValueError(f"mean_dir_vec holds 27 values, got {v.size}")
        for j in range(27):
            cfg.mean_dir_vec[j] = float(v[j])
    return cfg


def _ted_call(m, device, plan, raw, audio, mean_pose, cfg, audio_out_len, want):
    """One ``ls_ted_ingest``; ``want``: the outputs to allocate.  Returns them by name."""
    F, W, P = plan["n_frames"], plan["n_windows"], plan["n_poses"]
    shapes = {"resampled": (F, 10, 3), "dir_vec": (F, 9, 3), "pose_seq": (W, P, 30), "vec_seq": (W, P, 27), "x": (W, 9, 3, P),
              "audio_out": (W, audio_out_len), "stats": (W, len(STATS)), "verdict": (W,)}
    a = _lib.LsTedIngestArgs()
    a.batch, a.on_device, a.n_poses, a.n_ext = len(plan["n_raw"]), int(m.on_device), P, plan["n_ext"]
    a.n_frames, a.n_windows, a.audio_out_len = F, W, int(audio_out_len)
    a.cfg = C.pointer(cfg)
    mp = np.ascontiguousarray(np.asarray(_lib._np32(mean_pose)).reshape(-1))
    if mp.size != 30:
        raise ValueError(f"mean_pose holds 30 values, got {mp.size}")
    a.mean_pose = _ptr(mp)
    for k in ("n_raw", "audio_len", "frame_offsets", "frame_clip", "frame_lo", "frame_hi", "frame_frac", "win_clip", "win_first",
              "win_audio_start", "win_has_words"):
        setattr(a, k, _ptr(plan[k]))
    a.raw_poses, a.audio = m.f32(raw), m.f32(audio)
    out = {}
    for k in want:
        out[k], p = m.out(shapes[k], np.int32 if k == "verdict" else np.float32)
        setattr(a, k, p)
    m.ready()
    _lib.call("ls_ted_ingest", device, C.byref(a))
    return out


def _identity_plan(n, n_ext=None, n_poses=1):
    """Every raw frame as its own resampled frame (lo = hi = i, frac = 0), and one window over the first n_ext of them."""
    i = np.arange(n, dtype=np.int32)
    W = 0 if n_ext is None else 1
    return {"n_frames": n, "n_windows": W, "n_poses": n_poses, "n_ext": n_ext or n_poses, "n_raw": np.array([n], np.int32),
            "audio_len": np.array([1], np.int64), "frame_offsets": np.array([0, n], np.int32), "frame_clip": np.zeros(n, np.int32),
            "frame_lo": i, "frame_hi": i.copy(), "frame_frac": np.zeros(n, np.float32), "win_clip": np.zeros(W, np.int32),
            "win_first": np.zeros(W, np.int32), "win_audio_start": np.zeros(W, np.int64), "win_has_words": np.ones(W, np.uint8)}


_SILENCE = np.zeros(1, np.float32)


def resample_pose_seq(poses, duration_in_sec, fps, device: int = 0):
    """``utils.data_utils.resample_pose_seq``: poses [n, 10, 3] (or [n, 30]) recorded over ``duration_in_sec`` -> ceil(n / step)
    frames at ``fps``, linearly interpolated, the tail extrapolated.  numpy in, numpy out; CUDA tensor in, CUDA tensor out.  The
    arithmetic is float32, the reference's is float64 rounded to the input's dtype."""
    shape = tuple(poses.shape)
    n = int(shape[0])
    plan = ingest_plan([n], [0.0], [float(duration_in_sec)], [1 << 40], fps=fps, n_poses=1, n_ext=1)    # the frame table is what is wanted
    plan.update(n_windows=0, audio_len=np.array([1], np.int64))
    m = _lib._Marshal(device, poses)
    out = _ted_call(m, device, plan, _cat(m, [poses], 30), _SILENCE, np.zeros(30, np.float32), _post_cfg(), 1, ("resampled",))
    res = out["resampled"].reshape((plan["n_frames"],) + shape[1:])
    return res if m.on_device else res.astype(poses.dtype if hasattr(poses, "dtype") else np.float32)


def convert_pose_seq_to_dir_vec(pose, device: int = 0):
    """``utils.data_utils.convert_pose_seq_to_dir_vec``: joint positions [T, 10, 3] or [B, T, 10, 3] (the last two axes may be
    flattened to 30) -> unit bone directions [T, 9, 3] or [B, T, 9, 3]; a zero-length bone gives zeros, as
    sklearn.preprocessing.normalize does.  numpy in: float64 out like the reference's array (the values are float32)."""
    shape = tuple(pose.shape)
    if shape[-1] != 3:
        shape = shape[:-1] + (shape[-1] // 3, 3)
    if len(shape) not in (3, 4) or shape[-2:] != (10, 3):
        raise ValueError(f"expected [T, 10, 3] or [B, T, 10, 3], got {list(pose.shape)}")
    n = int(np.prod(shape[:-2]))
    m = _lib._Marshal(device, pose)
    if n == 0:
        return m.out(shape[:-2] + (9, 3))[0]
    out = _ted_call(m, device, _identity_plan(n), _cat(m, [pose], 30), _SILENCE, np.zeros(30, np.float32), _post_cfg(), 1, ("dir_vec",))
    d = out["dir_vec"].reshape(shape[:-2] + (9, 3))
    return d if m.on_device else d.astype(np.float64)


class MotionPreprocessor:
    """``data_loader.motion_preprocessor.MotionPreprocessor``: ``get()`` returns (skeletons as nested lists, "PASS") or ([], message)
    with message "pose", "spine angle" or "motion", from the statistics ``k_ted_ingest_window`` computes over the frames given
    (2 to 128 of them).  ``stats`` holds them after ``get()`` (``ingest.STATS`` names the five)."""

    def __init__(self, skeletons, mean_pose, device: int = 0):
        self.skeletons = skeletons
        self.mean_pose = mean_pose
        self.device = device
        self.filtering_message = "PASS"
        self.stats = None

    def get(self):
        assert self.skeletons is not None
        sk = self.skeletons
        if hasattr(sk, "shape") or len(sk):
            n = int(sk.shape[0]) if hasattr(sk, "shape") else len(sk)
            if not 2 <= n <= MAX_EXT:
                raise ValueError(f"MotionPreprocessor takes 2 to {MAX_EXT} frames, got {n}")
            m = _lib._Marshal(self.device, sk if hasattr(sk, "shape") else None)
            raw = _cat(m, [sk if hasattr(sk, "shape") else np.asarray(sk, np.float32)], 30)
            out = _ted_call(m, self.device, _identity_plan(n, n_ext=n), raw, _SILENCE, self.mean_pose, _post_cfg(), 1, ("stats", "verdict"))
            verdict, stats = (v.cpu().numpy() if m.on_device else v for v in (out["verdict"], out["stats"]))
            self.stats = stats[0]
            self.filtering_message = VERDICTS[int(verdict[0])]
            if self.filtering_message != "PASS":
                self.skeletons = []
            else:
                host = sk.detach().cpu().numpy() if hasattr(sk, "detach") else np.asarray(sk)
                assert not np.isnan(host).any()      # missing joints
                self.skeletons = host.tolist()
        return self.skeletons, self.filtering_message


def _beat_call(m, device, plan, poses, audio, mean_pose, std_pose, njoints, audio_out_len, keep_windows, want):
    W, P = plan["n_windows"], plan["n_poses"]
    shapes = {"rot6d": (W, P, njoints * 6), "x": (W, njoints, 6, P), "audio_out": (W, audio_out_len), "verdict": (W,)}
    a = _lib.LsBeatIngestArgs()
    a.batch, a.on_device, a.n_poses, a.njoints, a.n_windows = len(plan["n_raw"]), int(m.on_device), P, njoints, W
    a.audio_out_len = int(audio_out_len)
    keep = [np.ascontiguousarray(np.asarray(_lib._np32(v)).reshape(-1)) for v in (mean_pose, std_pose)]
    if any(k.size != njoints * 3 for k in keep):
        raise ValueError(f"mean_pose and std_pose hold {njoints * 3} values")
    a.mean_pose, a.std_pose = _ptr(keep[0]), _ptr(keep[1])
    for k in ("n_raw", "audio_len", "win_clip", "win_first", "win_audio_start"):
        setattr(a, k, _ptr(plan[k]))
    a.win_has_words = _ptr(keep_windows)
    a.poses, a.audio = m.f32(poses), m.f32(audio)
    out = {}
    for k in want:
        out[k], p = m.out(shapes[k], np.int32 if k == "verdict" else np.float32)
        setattr(a, k, p)
    m.ready()
    _lib.call("ls_beat_ingest", device, C.byref(a))
    return out


def make_audio_fixed_length(audio, expected_audio_length, device: int = 0):
    """``utils.data_utils.make_audio_fixed_length``: cut to ``expected_audio_length`` samples, or extend by
    np.pad(mode='symmetric'), read on the device as index arithmetic (no padded copy).  A padding longer than the audio itself (numpy
    would reflect back and forth) raises ValueError."""
    L, E = int(audio.shape[0]), int(expected_audio_length)
    if E < 1 or L < 1 or E > 2 * L:
        raise ValueError(f"cannot bring {L} samples to {E}: the symmetric padding may be as long as the audio, not longer")
    plan = {"n_windows": 1, "n_poses": 1, "n_raw": np.array([1], np.int32), "audio_len": np.array([L], np.int64),
            "win_clip": np.zeros(1, np.int32), "win_first": np.zeros(1, np.int32), "win_audio_start": np.zeros(1, np.int64)}
    m = _lib._Marshal(device, audio)
    one = np.ones(3, np.float32)
    out = _beat_call(m, device, plan, np.zeros((1, 3), np.float32), audio.reshape(-1), one, one, 1, E, None, ("audio_out",))
    res = out["audio_out"][0]
    return res if m.on_device else res.astype(audio.dtype)


def _lengths(parts):
    return [int(p.shape[0]) for p in parts]


def ted_ingest(skeletons, audio, start_times, end_times, mean_pose, mean_dir_vec, words=None, n_poses=34, stride=10, fps=15,
               disable_filtering=False, device: int = 0):
    """Every training / evaluation / editing window of a batch of TED recordings, as ``DataPreprocessor._sample_from_clip`` and the
    clipping of ``SpeechMotionDataset.__getitem__`` produce them.

    skeletons: list of [n_b, 10, 3] raw joint positions; audio: list of [L_b] 16 kHz waveforms; start_times / end_times: seconds per
    recording (their difference is the duration the n_b frames span); numpy arrays or tensors -- if any is a CUDA tensor, everything
    stays on the device and the results are CUDA tensors.  words: per recording a list of (word, start, end) sorted by start, or
    None (then every window has words; the reference always has a list).  A window spans ``int(round(n_poses * 1.25))`` resampled
    frames, of which the first ``n_poses`` are the sample.

    Returns a dict.  Over ALL windows, in the reference's order (recording by recording, window by window): ``clip`` and
    ``start_frame`` (host int32), ``verdict`` (int32, index into ``ingest.VERDICTS``), ``stats`` [W, 5] (``ingest.STATS``: how close
    a window was to a threshold) and ``keep`` (bool: verdict PASS, or anything but "words" with ``disable_filtering``).  Over the
    KEPT windows, in the same order: ``x`` [K, 9, 3, n_poses] (the model's layout), ``vec_seq`` [K, n_poses, 27], ``pose_seq``
    [K, n_poses, 30] and ``audio`` [K, int(round(n_poses / fps * 16000))].  ``keep`` is applied by one boolean index per output,
    which on the device costs one host wait (the number of kept windows decides the shapes)."""
    B = len(skeletons)
    if not (B and len(audio) == B and len(start_times) == B and len(end_times) == B):
        raise ValueError("one skeleton sequence, waveform, start and end time per recording")
    plan = ingest_plan(_lengths(skeletons), start_times, end_times, _lengths(audio), words=words, n_poses=n_poses, stride=stride, fps=fps)
    m = _lib._Marshal(device, *skeletons, *audio)
    raw, wav = _cat(m, skeletons, 30), _cat(m, audio, 1)
    out = _ted_call(m, device, plan, raw, wav.reshape(-1), mean_pose, _post_cfg(mean_dir_vec), int(round(n_poses / fps * 16000)),
                    ("pose_seq", "vec_seq", "x", "audio_out", "stats", "verdict"))
    verdict = out["verdict"]
    keep = verdict == 0
    if disable_filtering:
        keep = keep | (verdict != 4)
    return {"x": out["x"][keep], "vec_seq": out["vec_seq"][keep], "pose_seq": out["pose_seq"][keep],
            "audio": out["audio_out"][keep], "clip": plan["win_clip"], "start_frame": plan["win_first"], "verdict": verdict,
            "stats": out["stats"], "keep": keep}


def beat_ingest(poses, audio, mean_pose, std_pose, keep_windows=None, n_poses=34, stride=10, fps=15, sr=16000, clean_first_seconds=0,
                clean_final_seconds=0, device: int = 0):
    """BEAT twin (beat.py:365-485, then process_cache.py:38-45).  poses: list of [n_b, 141] normalised Euler rows at ``fps``; audio:
    list of [L_b]; mean_pose / std_pose [141] (bvh_mean.npy / bvh_std.npy, degrees).  Per recording the whole seconds both streams
    cover, less the clean seconds, are cut into ``n_poses``-frame windows; each becomes ``* std + mean`` -> radians ->
    ``euler_angles_to_matrix(., "XYZ")`` -> ``matrix_to_rotation_6d``.

    BEAT's ``MotionPreprocessor.get`` filters nothing, so the verdict is PASS or "words".  The reference's two word rules --
    ``len(set(sample_word)) < 4`` and, with ``use_sem``, ``(sample_sem < 0.4).all()`` -- read arrays this entry does not take: the
    caller evaluates them and passes ``keep_windows``, one byte per window in the order of ``ingest_plan(..., beat=True)`` (0: the
    window is dropped with verdict "words"); None keeps every window.

    Returns ``x`` [K, 47, 6, n_poses], ``rot6d`` [K, n_poses, 282] and ``audio`` [K, floor(n_poses / fps * sr)] over the kept
    windows, and ``clip``, ``start_frame``, ``verdict``, ``keep`` over all of them; the boolean index costs one host wait."""
    B = len(poses)
    if not (B and len(audio) == B):
        raise ValueError("one pose sequence and one waveform per recording")
    J3 = int(poses[0].shape[-1])
    if J3 % 3 or not 1 <= J3 // 3 <= 47:
        raise ValueError(f"expected rows of 3 Euler angles for up to 47 joints, got {J3} columns")
    n_raw, L = _lengths(poses), _lengths(audio)
    seconds = [min(n // int(fps), l // int(sr)) for n, l in zip(n_raw, L)]
    plan = ingest_plan(n_raw, [clean_first_seconds] * B, [s - clean_final_seconds for s in seconds], L, n_poses=n_poses, stride=stride,
                       fps=fps, sr=sr, beat=True)
    if keep_windows is not None:
        keep_windows = np.ascontiguousarray(np.asarray(keep_windows).reshape(-1) != 0, np.uint8)
        if keep_windows.size != plan["n_windows"]:
            raise ValueError(f"keep_windows holds one byte per window: got {keep_windows.size} for {plan['n_windows']}")
    m = _lib._Marshal(device, *poses, *audio)
    out = _beat_call(m, device, plan, _cat(m, poses, J3), _cat(m, audio, 1).reshape(-1), mean_pose, std_pose, J3 // 3,
                     int(np.floor(n_poses / fps * sr)), keep_windows, ("rot6d", "x", "audio_out", "verdict"))
    keep = out["verdict"] == 0
    return {"x": out["x"][keep], "rot6d": out["rot6d"][keep], "audio": out["audio_out"][keep],
            "clip": plan["win_clip"], "start_frame": plan["win_first"], "verdict": out["verdict"], "keep": keep}
