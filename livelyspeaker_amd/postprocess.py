"""Caller-side plumbing around the sampler: what ``scripts/test_RAG_ted.py:84-111`` and
``scripts/utils/data_utils.py:77-97`` do with a sampled batch, as one small GPU kernel (``ls_ted_post``).

The numbers below are DATASET CONSTANTS of the TED gesture data as published in the reference's scripts
(mean direction vector ``test_RAG_ted.py:22``, angle pairs ``:24-29``, per-pair normalisers ``:30``, beat
threshold ``:32``, bone tree and lengths ``utils/data_utils.py:13-14``); they are data, passed to the kernel."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib

TED_MEAN_DIR_VEC = np.array([0.0154009, -0.9690125, -0.0884354, -0.0022264, -0.8655276, 0.4342174, -0.0035145, -0.8755367,
                             -0.4121039, -0.9236511, 0.3061306, -0.0012415, -0.5155854, 0.8129665, 0.0871897, 0.2348464,
                             0.1846561, 0.8091402, 0.9271948, 0.2960011, -0.013189, 0.5233978, 0.8092403, 0.0725451,
                             -0.2037076, 0.1924306, 0.8196916], dtype=np.float32)
TED_ANGLE_PAIRS = [(3, 4), (4, 5), (6, 7), (7, 8)]
TED_CHANGE_ANGLE = [0.0034540758933871984, 0.007043459918349981, 0.003493624273687601, 0.007205077446997166]
TED_BEAT_THRES = 0.03
TED_DIR_VEC_PAIRS = [(0, 1, 0.26), (1, 2, 0.18), (2, 3, 0.14), (1, 4, 0.22), (4, 5, 0.36), (5, 6, 0.33), (1, 7, 0.22),
                     (7, 8, 0.36), (8, 9, 0.33)]
TED_FPS = 15.0
TED_BEAT_SIGMA = 0.1          # test_RAG_ted.py:33


def ted_post_config() -> "_lib.LsPostConfig":
    c = _lib.LsPostConfig()
    c.njoints, c.n_pairs, c.n_pose_joints, c.thres = 9, len(TED_ANGLE_PAIRS), 10, TED_BEAT_THRES
    for k, (a, b) in enumerate(TED_ANGLE_PAIRS):
        c.pair_a[k], c.pair_b[k], c.change_angle[k] = a, b, TED_CHANGE_ANGLE[k]
    for j, (pa, ch, ln) in enumerate(TED_DIR_VEC_PAIRS):
        c.bone_parent[j], c.bone_child[j], c.bone_len[j] = pa, ch, ln
    for j, v in enumerate(TED_MEAN_DIR_VEC):
        c.mean_dir_vec[j] = float(v)
    return c


def _ted_result(m, B, aligned, pose, diff, mask) -> dict:
    """What both TED wrappers return: the mask as bool, the beats as seconds (t / 15)."""
    mask_np = mask.cpu().numpy() if m.on_device else mask
    beats = [[float(t) / TED_FPS for t in np.nonzero(mask_np[b])[0]] for b in range(B)]
    return {"aligned_motions": aligned, "pose": pose, "angle_diff": diff,
            "beat_mask": mask.bool() if m.on_device else mask.astype(bool), "motion_beat_times": beats}


def ted_postprocess(sample, device: int = 0, want_pose: bool = True) -> dict:
    """sample: [B, 9, 3, 34] (numpy, CPU tensor or CUDA tensor as returned by the sampler).
    Returns aligned_motions [B,34,27], pose [B,34,10,3], angle_diff [B,34], beat_mask [B,34] (bool) and
    motion_beat_times (list of lists of seconds, t/15 as in test_RAG_ted.py:111)."""
    m = _lib._Marshal(device, sample)
    B = int(sample.shape[0])
    cfg = ted_post_config()
    aligned, p_al = m.out((B, 34, 27))
    pose, p_pose = m.out((B, 34, 10, 3)) if want_pose else (None, None)
    diff, p_diff = m.out((B, 34))
    mask, p_mask = m.out((B, 34), np.uint8)
    p_in = m.f32(sample, (B, 9, 3, 34))
    m.ready()
    _lib.call("ls_ted_post", device, int(m.on_device), B, C.byref(cfg), p_in, p_al, p_pose, p_diff, p_mask)
    return _ted_result(m, B, aligned, pose, diff, mask)


def beat_postprocess(sample, device: int = 0, want_euler: bool = True) -> dict:
    """BEAT caller plumbing (scripts_beat/test_RAG_beat.py:86, 101).  sample: [B, 47, 6, 34] (numpy, CPU tensor or CUDA tensor as
    returned by the sampler).  Returns decoded_motions [B, 34, 282] (the rot6d pose sequence the evaluator and the metrics
    consume) and pred_euler [B, 34, 141]: Euler XYZ angles in degrees of every joint (rot_utils.matrix_to_euler_angles(
    rot_utils.rotation_6d_to_matrix(.), "XYZ") / pi * 180).  ``beat_metrics`` scores these planes (SRGR, motion beats, BeatAlign, L1
    diversity); audio onsets stay with the caller."""
    m = _lib._Marshal(device, sample)
    B, J = int(sample.shape[0]), int(sample.shape[1])
    if tuple(sample.shape[2:]) != (6, 34):
        raise ValueError(f"expected [B, J, 6, 34], got {tuple(sample.shape)}")
    dec, p_dec = m.out((B, 34, J * 6))
    eul, p_eul = m.out((B, 34, J * 3)) if want_euler else (None, None)
    p_in = m.f32(sample, (B, J, 6, 34))
    m.ready()
    _lib.call("ls_beat_post", device, int(m.on_device), B, J, p_in, p_dec, p_eul)
    return {"decoded_motions": dec, "pred_euler": eul}


TIMELINE_TILE = 64            # frames per workgroup of the timeline kernels (LS_TIMELINE_TILE); no result depends on it
TIMELINE_MAX_FRAMES = 4096    # LS_TIMELINE_MAX_FRAMES


def _timeline_frames(timeline, feats, least):
    if len(timeline.shape) != 4 or int(timeline.shape[2]) != feats:
        raise ValueError(f"expected a timeline [B, J, {feats}, N], got {list(timeline.shape)}")
    N = int(timeline.shape[3])
    if not least <= N <= TIMELINE_MAX_FRAMES:
        raise ValueError(f"a timeline holds {least} to {TIMELINE_MAX_FRAMES} frames, got {N} (longer timelines are not built)")
    return N


def _clip_frames(frames, B, least, N):
    return None if frames is None else _lib.host_lengths(frames, B, least, N, "frames")


def ted_postprocess_timeline(timeline, device: int = 0, want_pose: bool = True, frames=None) -> dict:
    """``ted_postprocess`` on a stitched timeline [B, 9, 3, N] of any length N in [4, 4096] (``long_form.sample_long``), as ONE series
    per clip: nothing resets at a window seam (``ls_ted_post_timeline``).  Returns aligned_motions [B,N,27], pose [B,N,10,3],
    angle_diff [B,N], beat_mask [B,N] (bool; beats at t in [2, N-2]) and motion_beat_times (one list of seconds, t/15, per clip).
    ``frames`` (a host sequence [B], each in [4, N]): clips of different lengths in one call (``ls_ted_post_timeline_ragged``); N is
    then the row stride.  On clip b's first ``frames[b]`` frames every output is bit for bit that of the clip alone at its own length
    (beats at t in [2, frames[b] - 2]); beyond them the outputs are 0 and the input is never read."""
    N = _timeline_frames(timeline, 3, 4)
    m = _lib._Marshal(device, timeline)
    B = int(timeline.shape[0])
    fr = _clip_frames(frames, B, 4, N)
    cfg = ted_post_config()
    aligned, p_al = m.out((B, N, 27))
    pose, p_pose = m.out((B, N, 10, 3)) if want_pose else (None, None)
    diff, p_diff = m.out((B, N))
    mask, p_mask = m.out((B, N), np.uint8)
    p_in = m.f32(timeline, (B, 9, 3, N))
    m.ready()
    if fr is None:
        _lib.call("ls_ted_post_timeline", device, int(m.on_device), B, N, C.byref(cfg), p_in, p_al, p_pose, p_diff, p_mask)
    else:
        _lib.call("ls_ted_post_timeline_ragged", device, int(m.on_device), B, N, fr.ctypes.data_as(C.c_void_p), C.byref(cfg), p_in, p_al,
                  p_pose, p_diff, p_mask)
    return _ted_result(m, B, aligned, pose, diff, mask)


def beat_postprocess_timeline(timeline, device: int = 0, want_euler: bool = True, frames=None) -> dict:
    """``beat_postprocess`` on a stitched timeline [B, J, 6, N], N in [2, 4096] (``ls_beat_post_timeline``): decoded_motions
    [B, N, J*6] and pred_euler [B, N, J*3] in degrees, which ``beat_metrics.beat_metrics_timeline`` scores.  ``frames`` (a host
    sequence [B], each in [2, N]): the clips' valid frames (``ls_beat_post_timeline_ragged``); the outputs are 0 beyond them."""
    N = _timeline_frames(timeline, 6, 2)
    m = _lib._Marshal(device, timeline)
    B, J = int(timeline.shape[0]), int(timeline.shape[1])
    fr = _clip_frames(frames, B, 2, N)
    dec, p_dec = m.out((B, N, J * 6))
    eul, p_eul = m.out((B, N, J * 3)) if want_euler else (None, None)
    p_in = m.f32(timeline, (B, J, 6, N))
    m.ready()
    if fr is None:
        _lib.call("ls_beat_post_timeline", device, int(m.on_device), B, J, N, p_in, p_dec, p_eul)
    else:
        _lib.call("ls_beat_post_timeline_ragged", device, int(m.on_device), B, J, N, fr.ctypes.data_as(C.c_void_p), p_in, p_dec, p_eul)
    return {"decoded_motions": dec, "pred_euler": eul}


POST_STREAM_MAX_CHUNK = _lib.POST_STREAM_MAX_CHUNK      # frames per slot and push (LS_POST_STREAM_MAX_CHUNK)
BEAT_SERIES_JOINTS = (4, 3, 5, 26, 25, 27)              # beat_metrics.BEAT_SERIES_JOINTS: right arm, shoulder, wrist; left arm, shoulder, wrist


def post_stream_plan(dataset, n_before, n_new, finishing=False, order=2):
    """The beat entries a ``PostStream.push`` of ``n_new`` frames decides on a series that holds ``n_before`` (no GPU):
    ``(beat_first, beat_count)``.  TED entries are frames of ``beat_mask``: ``[max(0, n - 1), N - 1)`` with ``N = n_before + n_new``
    (the beat at f needs ``angle_diff[f + 1]``), up to ``N`` when finishing.  BEAT entries are velocity indices:
    ``[max(0, n - order - 1), max(0, N - order - 1))``, up to ``N - 1`` when finishing.  One definition for the engine and for this
    module (``ls_post_stream_plan``)."""
    return _lib.post_stream_plan(dataset, n_before, n_new, finishing, order)


class PostStream:
    """A running ``open_post_stream``; see there.  ``frames_in``: the frames of each slot's running series (host int64 [S])."""

    def __init__(self, dataset, capacity, device, order, series_joints, joints):
        if dataset not in ("ted", "beat"):
            raise ValueError(f"dataset must be 'ted' or 'beat', got {dataset!r}")
        S = int(capacity)
        if S < 1:
            raise ValueError(f"capacity must be >= 1, got {capacity}")
        self.dataset, self.capacity, self.device = dataset, S, int(device)
        self._beat = dataset == "beat"
        self.order = int(order) if self._beat else 1
        self.joints = int(joints) if self._beat else 9
        self._series = tuple(int(j) for j in series_joints)
        if self._beat:
            if not 1 <= self.order <= _lib.POST_STREAM_MAX_ORDER:
                raise ValueError(f"order must lie in [1, {_lib.POST_STREAM_MAX_ORDER}], got {order}")
            if self.joints < 1 or len(self._series) != 6 or any(not 0 <= j < self.joints for j in self._series):
                raise ValueError(f"series_joints must name six of the {self.joints} joints, got {list(series_joints)}")
        self._n = np.zeros(S, np.int64)
        self._eng = None
        self._closed = False

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    @property
    def frames_in(self):
        return self._n.copy()

    def _engine(self):
        if self._eng is None:         # bound at the first push: every refusal above and in push comes before a device is touched
            self._eng = _lib.PostStreamEngine(self.dataset, self.capacity, self.device, None if self._beat else ted_post_config(), self.joints,
                                              self.order, self._series if self._beat else (0,) * 6)
        return self._eng

    def device_bytes(self) -> int:
        """What the handle holds on the device (``ls_post_stream_info``); constant from the first push on."""
        return self._engine().info()["device_bytes"]

    def push(self, frames, counts=None, finish=None) -> dict:
        """``frames`` [S, J, F, K], K <= 256 (numpy, CPU or CUDA tensor): slot s's new frames in ``frames[s, ..., :counts[s]]``
        (``counts=None``: K for every slot).  ``finish`` (bool [S]): the slots whose series end with this push."""
        if self._closed:
            raise RuntimeError("the post-processing stream is closed")
        S, J, F = self.capacity, self.joints, 6 if self._beat else 3
        if len(frames.shape) != 4 or tuple(int(v) for v in frames.shape[:3]) != (S, J, F):
            raise ValueError(f"frames must be [{S}, {J}, {F}, K], got {list(frames.shape)}")
        K = int(frames.shape[3])
        if K > POST_STREAM_MAX_CHUNK:
            raise ValueError(f"a push takes at most {POST_STREAM_MAX_CHUNK} frames per slot, got {K} (larger chunks are not built)")
        if counts is None:
            counts = np.full(S, K, np.int64)
        if hasattr(counts, "detach"):
            counts = counts.detach().cpu().numpy()
        if finish is not None and hasattr(finish, "detach"):
            finish = finish.detach().cpu().numpy()
        first, count = _lib.post_stream_check(self.dataset, self.order, self._n, K, counts, finish)
        k = np.ascontiguousarray(np.asarray(counts).reshape(-1), dtype=np.int32)
        fin = np.zeros(S, np.int32) if finish is None else np.asarray(finish).reshape(-1).astype(bool).astype(np.int32)
        Kb = int(count.max())
        m = _lib._Marshal(self.device, frames)
        a = _lib.LsPostStreamPushArgs()
        a.on_device, a.K, a.beat_capacity = int(m.on_device), K, Kb
        a.counts, a.finish = k.ctypes.data, fin.ctypes.data
        if self._beat:
            dec, a.decoded = m.out((S, K, J * 6))
            eul, a.euler_deg = m.out((S, K, J * 3))
            mask, a.beat_mask = m.out((S, 6, Kb), np.uint8)
            res = {"decoded_motions": dec, "pred_euler": eul}
        else:
            aligned, a.aligned = m.out((S, K, 27))
            pose, a.pose = m.out((S, K, 10, 3))
            diff, a.angle_diff = m.out((S, K))
            mask, a.beat_mask = m.out((S, Kb), np.uint8)
            res = {"aligned_motions": aligned, "pose": pose, "angle_diff": diff}
        a.frames = m.f32(frames, (S, J, F, K)) if K else None
        eng = self._engine()
        m.ready()
        eng.push(a)
        self._n = np.where(fin != 0, 0, self._n + k)
        res.update(beat_mask=mask.bool() if m.on_device else mask.astype(bool), beat_first=first, beat_count=count)
        if not self._beat:
            host = mask.cpu().numpy() if m.on_device else mask
            res["motion_beat_times"] = [[float(first[s] + q) / TED_FPS for q in np.nonzero(host[s, :count[s]])[0]] for s in range(S)]
        return res

    def finish(self, slot) -> dict:
        """End slot ``slot``'s series: a push without frames that emits its pending beat entries.  The slot is free afterwards."""
        slot = int(slot)
        if not 0 <= slot < self.capacity or self._n[slot] < 1:
            raise ValueError(f"slot {slot} holds no running series")
        fin = np.zeros(self.capacity, bool)
        fin[slot] = True
        return self._finish(fin)

    def _finish(self, fin):
        empty = np.zeros((self.capacity, self.joints, 6 if self._beat else 3, 0), np.float32)       # no frames: the entries come back on the host
        return self.push(empty, np.zeros(self.capacity, np.int64), fin)

    def close(self):
        """Finish every slot that holds a series (returns that push's dict, or None when there was none) and release the handle."""
        if self._closed:
            return None
        res = self._finish(self._n > 0) if (self._n > 0).any() else None
        self._closed = True
        if self._eng is not None:
            self._eng.close()
        return res


def open_post_stream(dataset, capacity, device=0, order=2, series_joints=BEAT_SERIES_JOINTS, joints=47) -> PostStream:
    """The online form of ``ted_postprocess_timeline`` / ``beat_postprocess_timeline`` + ``beat_metrics_timeline``'s motion beats: a
    device-resident stream of ``capacity`` slots that is fed model-space frames as they arrive (``open_stream`` / ``open_pool``'s
    output, or any source in that layout) and returns their post-processed rows at once, plus the beats that have just become decidable.

        ps = open_post_stream('ted', capacity)
        out = ps.push(frames, counts=None, finish=None)     # [S, J, F, K], K <= 256
        tail = ps.finish(slot)                              # the slot's pending beat entries; its next frames start a new series
        ps.close()

    ``push`` returns, all ``[S, K, ...]`` with rows behind ``counts[s]`` zero and on the device for device input: TED
    ``aligned_motions`` [S,K,27], ``pose`` [S,K,10,3], ``angle_diff`` [S,K]; BEAT ``decoded_motions`` [S,K,J*6], ``pred_euler``
    [S,K,J*3].  And the beats: ``beat_mask`` (TED bool [S,Kb]; BEAT [S,6,Kb], one row per series of ``series_joints``) whose entry q of
    slot s is series entry ``beat_first[s] + q`` for ``q < beat_count[s]`` (``post_stream_plan``; Kb = the largest count), and for TED
    ``motion_beat_times``: per slot the seconds ``frame / 15`` of the beats decided in this push.  TED beats lag the frames by one, BEAT
    minima by ``order + 1``; ``finish`` emits what is pending.

    Per slot, everything concatenated over the pushes and the finish is bit for bit what the timeline entries give for the whole
    series, whatever the chunking and for series of any length (tests/test_gpu_post_stream.py): the kernels run the timeline kernels'
    per-frame functions, and what a frame needs from its left is carried on the device (TED: 3 raw frames per slot; BEAT: 2 order + 1
    Euler triples of the six joints).  Device memory is allocated at the first push and does not grow (``device_bytes``).

    Audio onsets and the BC / BeatAlign scores come at the finish: ``open_score_stream`` (librosa normalises the onset envelope by the
    whole signal's extrema and clamps at the global maximum - 80 dB, so they are not causal).  Not built: SRGR (it needs targets),
    device-resident ``counts``, chunks over 256 frames per push."""
    return PostStream(dataset, capacity, device, order, series_joints, joints)


SCORE_OUTPUTS = ("count", "onset_raw", "onset_bt", "onset_bt_rms", "oenv", "mel_db", "rms")


def score_stream_plan(samples_before, n_new, finishing=False, pad_mode="constant"):
    """The audio frames a ``ScoreStream.push`` of ``n_new`` samples decides on a series that holds ``samples_before`` (no GPU):
    ``(frame_first, frame_count)``.  Frame f covers samples [512 f - 1024, 512 f + 1024): it is decided once the series holds
    512 f + 1024 samples (and, under reflect padding, 1025); a finish decides every frame below 1 + L // 512.  One definition for the
    engine and for this module (``ls_score_stream_plan``)."""
    from .audio_onsets import PAD_MODES
    if pad_mode not in PAD_MODES:
        raise ValueError(f"pad_mode must be 'constant' or 'reflect', got {pad_mode!r}")
    return _lib.score_stream_plan(PAD_MODES[pad_mode], samples_before, n_new, finishing)


class ScoreStream:
    """A running ``open_score_stream``; see there.  ``frames_in``: the decided audio frames of each slot's series, ``samples_in`` its
    samples, ``beats_in`` its motion-beat entries (host int64 [S])."""

    def __init__(self, dataset, capacity, max_seconds, sr=16000, device=0, *, sr_pick=None, pad_mode="constant", fmax=11025.0, delta=0.07,
                 sigma=None, fps=TED_FPS, max_chunk=65536, align_series=2, onset_source="onset_bt_rms", time_rate=22050.0,
                 want=("count", "onset_raw")):
        from . import audio_onsets as ao
        if dataset not in ("ted", "beat"):
            raise ValueError(f"dataset must be 'ted' or 'beat', got {dataset!r}")
        S = int(capacity)
        if S < 1:
            raise ValueError(f"capacity must be >= 1, got {capacity}")
        if pad_mode not in ao.PAD_MODES:
            raise ValueError(f"pad_mode must be 'constant' or 'reflect', got {pad_mode!r}")
        if not float(max_seconds) > 0 or not float(sr) > 0 or not float(fps) > 0:
            raise ValueError(f"max_seconds, sr and fps must be > 0, got {max_seconds}, {sr}, {fps}")
        unknown = set(want) - set(SCORE_OUTPUTS)
        if unknown:
            raise ValueError(f"unknown outputs {sorted(unknown)}")
        sources = ("onset_raw", "onset_bt", "onset_bt_rms")
        if onset_source not in sources:
            raise ValueError(f"onset_source must be one of {sources}, got {onset_source!r}")
        if not 0 <= int(align_series) < 6:
            raise ValueError(f"align_series must name one of the six series, got {align_series}")
        if int(max_chunk) < 1:
            raise ValueError(f"max_chunk must be >= 1, got {max_chunk}")
        self.dataset, self.capacity, self.device, self.sr = dataset, S, int(device), float(sr)
        self._beat = dataset == "beat"
        self.align_series = int(align_series)
        self.want = tuple(want)
        self.max_samples = int(round(float(max_seconds) * float(sr)))
        self.max_audio_frames = 1 + self.max_samples // ao.HOP
        self.max_beat_entries = int(np.ceil(float(max_seconds) * float(fps))) + 1
        if self.max_samples < 1 or self.max_samples > ao.MAX_LENGTH_LONG:
            raise ValueError(f"max_seconds * sr must lie in [1, {ao.MAX_LENGTH_LONG}] samples, got {self.max_samples}")
        c = _lib.LsScoreConfig()
        c.sr, c.pad_mode, c.fmax, c.delta = float(sr), ao.PAD_MODES[pad_mode], float(fmax), float(delta)
        c.sr_pick = float(sr_pick) if sr_pick is not None else (22050.0 if self._beat else float(sr))
        c.hop, c.onset_source, c.max_chunk = ao.HOP, sources.index(onset_source), int(max_chunk)
        c.fps, c.time_rate = float(fps), float(time_rate)
        c.sigma = float(sigma) if sigma is not None else (0.3 if self._beat else TED_BEAT_SIGMA)
        if not (c.fmax > 0 and c.sr_pick > 0 and c.sigma > 0 and c.time_rate > 0):
            raise ValueError("fmax, sr_pick, sigma and time_rate must be > 0")
        self._cfg, self.max_chunk, self.pad_mode, self.sigma = c, int(max_chunk), pad_mode, float(c.sigma)
        self._samples = np.zeros(S, np.int64)
        self._frames = np.zeros(S, np.int64)
        self._beats = np.zeros(S, np.int64)
        self._eng = None
        self._closed = False

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    @property
    def frames_in(self):
        return self._frames.copy()

    @property
    def samples_in(self):
        return self._samples.copy()

    @property
    def beats_in(self):
        return self._beats.copy()

    def _engine(self):
        if self._eng is None:         # bound at the first push: every refusal above and in push comes before a device is touched
            self._eng = _lib.ScoreStreamEngine(self.dataset, self.capacity, self.max_audio_frames, self.max_beat_entries, self._cfg, self.device)
        return self._eng

    @property
    def device_bytes(self) -> int:
        """What the handle holds on the device (``ls_score_stream_info``); constant from the first push on."""
        return self._engine().info()["device_bytes"]

    def push(self, audio=None, lengths=None, beats=None):
        """``audio`` [S, n] (numpy, CPU or CUDA tensor; n <= max_chunk): slot s's new samples in ``audio[s, :lengths[s]]`` (``lengths=None``:
        n for every slot).  ``beats``: the dict a ``PostStream.push`` (or ``finish`` / ``close``) of the same slots returned -- its
        ``beat_mask``, ``beat_first`` and ``beat_count``; for BEAT the row ``align_series`` of the mask is taken.  Either may be left out.
        What would not fit a slot is refused (``ValueError``) before anything runs, and the stream stays as it was."""
        if self._closed:
            raise RuntimeError("the score stream is closed")
        if audio is None and beats is None:
            raise ValueError("pass audio, beats or both")
        S = self.capacity
        a = _lib.LsScoreStreamPushArgs()
        members, fresh, new_frames, k = [], np.zeros(S, np.int64), np.zeros(S, np.int64), np.zeros(S, np.int64)
        if audio is not None:
            if len(audio.shape) != 2 or int(audio.shape[0]) != S:
                raise ValueError(f"audio must be [{S}, n], got {list(audio.shape)}")
            n_max = int(audio.shape[1])
            if n_max > self.max_chunk:
                raise ValueError(f"a push takes at most max_chunk = {self.max_chunk} samples per slot, got {n_max}")
            fresh = np.full(S, n_max, np.int64) if lengths is None else _lib.host_lengths(lengths, S, 0, n_max, "lengths").astype(np.int64)
            for s in range(S):
                if 1 + (self._samples[s] + fresh[s]) // 512 > self.max_audio_frames:
                    raise ValueError(f"slot {s} would hold {self._samples[s] + fresh[s]} samples, above the {self.max_samples} of max_seconds")
                new_frames[s] = score_stream_plan(self._samples[s], fresh[s], False, self.pad_mode)[1]
            members.append(audio)
        elif lengths is not None:
            raise ValueError("lengths are the valid samples of audio: pass audio")
        if beats is not None:
            mask, first, k = beats["beat_mask"], np.asarray(beats["beat_first"]).reshape(-1), np.asarray(beats["beat_count"]).reshape(-1).astype(np.int64)
            if self._beat:
                if len(mask.shape) != 3 or int(mask.shape[1]) != 6:
                    raise ValueError(f"a BEAT beat_mask is [S, 6, Kb], got {list(mask.shape)}")
                mask = mask[:, self.align_series]
            if len(mask.shape) != 2 or int(mask.shape[0]) != S or first.shape != (S,) or k.shape != (S,):
                raise ValueError(f"beat_mask [{S}, Kb] with beat_first and beat_count [{S}], got {list(mask.shape)}, {first.shape}, {k.shape}")
            Kb = int(mask.shape[1])
            if Kb > _lib.SCORE_STREAM_MAX_BEATS or (k < 0).any() or (k > Kb).any():
                raise ValueError(f"beat_count must lie in [0, Kb] and Kb <= {_lib.SCORE_STREAM_MAX_BEATS}, got {k.tolist()} for Kb = {Kb}")
            for s in range(S):
                if k[s] and int(first[s]) != int(self._beats[s]):
                    raise ValueError(f"slot {s} holds {self._beats[s]} beat entries, the chunk starts at {int(first[s])}")
                if self._beats[s] + k[s] > self.max_beat_entries:
                    raise ValueError(f"slot {s} would hold {self._beats[s] + k[s]} beat entries, above the {self.max_beat_entries} of max_seconds")
            members.append(mask)
        m = _lib._Marshal(self.device, *members)
        a.on_device = int(m.on_device)
        keep = []
        if audio is not None:
            lens32 = np.ascontiguousarray(fresh, np.int32)
            keep.append(lens32)
            a.n_max, a.audio, a.lengths = n_max, m.f32(members[0], (S, n_max)), lens32.ctypes.data
        if beats is not None:
            first64, k32 = np.ascontiguousarray(first, np.int64), np.ascontiguousarray(k, np.int32)
            keep += [first64, k32]
            a.beat_capacity, a.beats = Kb, m.u8(members[-1], (S, Kb))
            a.beat_first, a.beat_count = first64.ctypes.data, k32.ctypes.data
        if (audio is None or n_max == 0 or not fresh.any()) and (beats is None or Kb == 0 or not k.any()):
            return
        eng = self._engine()
        m.ready()
        eng.push(a)
        self._samples += fresh
        self._frames += new_frames
        if beats is not None:
            self._beats += k

    def finish(self, slot) -> dict:
        """End slot ``slot``'s series and score it.  Returns ``n_frames`` (audio frames), ``count`` (onsets), the outputs named in the
        stream's ``want`` cut to the slot's own frames ([F], mel_db [F, 128]; host arrays, also for a stream that was fed device
        tensors), and TED ``align_sum`` (float), ``n_beats``; BEAT ``align``.  The slot is free afterwards."""
        slot = int(slot)
        if not 0 <= slot < self.capacity or self._samples[slot] < 1:
            raise ValueError(f"slot {slot} holds no audio")
        return self._finish([slot])[slot]

    def _finish(self, slots) -> dict:
        if self._closed:
            raise RuntimeError("the score stream is closed")
        S = self.capacity
        flags = np.zeros(S, np.int32)
        flags[list(slots)] = 1
        F = [1 + int(self._samples[s]) // 512 for s in range(S)]
        for s in slots:
            score_stream_plan(self._samples[s], 0, True, self.pad_mode)          # raises for what the engine refuses
        cols = max(F[s] for s in slots)
        o = _lib.LsScoreStreamOutputs()
        o.on_device, o.cols = 0, cols
        bufs = {"n_frames": np.zeros(S, np.int32), "count": np.zeros(S, np.int32)}
        for name in self.want:
            if name != "count":
                bufs[name] = np.zeros((S, cols, 128) if name == "mel_db" else (S, cols), np.float32 if name in ("oenv", "mel_db", "rms") else np.int32)
        if self._beat:
            bufs["align"] = np.zeros(S, np.float32)
        else:
            bufs["align_sum"], bufs["n_beats"] = np.zeros(S, np.float64), np.zeros(S, np.int32)
        for name, arr in bufs.items():
            setattr(o, name, arr.ctypes.data)
        self._engine().finish(flags, o)
        res = {}
        for s in slots:
            r = {"n_frames": int(bufs["n_frames"][s]), "count": int(bufs["count"][s])}
            for name in self.want:
                if name != "count":
                    r[name] = bufs[name][s, :F[s]].copy()
            if self._beat:
                r["align"] = float(bufs["align"][s])
            else:
                r["align_sum"], r["n_beats"] = float(bufs["align_sum"][s]), int(bufs["n_beats"][s])
            res[s] = r
            self._samples[s] = self._frames[s] = self._beats[s] = 0
        return res

    def close(self) -> dict:
        """Finish every slot that holds audio (returns {slot: its ``finish`` dict}) and release the handle."""
        if self._closed:
            return {}
        slots = [s for s in range(self.capacity) if self._samples[s] > 0]
        res = self._finish(slots) if slots else {}
        self._closed = True
        if self._eng is not None:
            self._eng.close()
        return res


def open_score_stream(dataset, capacity, max_seconds, sr=16000, device=0, **options) -> ScoreStream:
    """Audio onsets and the beat-alignment scores for talks of any length: the scoring half of ``open_post_stream``.

        ss = open_score_stream('ted', capacity, max_seconds=900)
        ss.push(audio=chunk, lengths=None, beats=ps.push(frames))     # audio [S, n]; beats: a PostStream.push dict
        res = ss.finish(slot)                                          # count, onset_raw, align_sum, n_beats (TED) / align (BEAT)
        ss.close()

    Only two steps of librosa's onset chain need the whole signal -- the clamp at max - 80 dB and the envelope's min / max
    normalisation -- and both are order-independent reductions; the spectrum is causal.  A push computes the mel spectra of the audio
    frames its samples decide (``score_stream_plan``) and appends the motion beats; ``finish`` pads the end at the slot's own last
    sample, runs the tiled pick of ``audio_onsets_long`` on the slot's frames and the alignment sum against its beats.  Up to
    4096 audio frames every output equals ``audio_onsets`` on the slot's samples alone bit for bit, under any chunking; up to 4096
    pose frames ``align_sum`` / ``n_beats`` equal ``ted_beat_align`` and ``align`` ``beat_metrics_timeline``'s bit for bit
    (tests/test_gpu_score_stream.py).  A slot does not depend on the other slots.

    Everything is allocated at the first push for ``max_seconds`` per slot -- 516 B per audio frame (about 16 KB per second at 16 kHz),
    one byte per pose frame, one slot's workspace for the finish -- and nothing grows (``device_bytes``).  ``options``: ``sr_pick``
    (default ``sr`` on TED, 22050 on BEAT), ``pad_mode``, ``fmax``, ``delta``, ``sigma`` (0.1 / 0.3), ``fps`` (15), ``max_chunk``
    (samples per slot and push, 65536), ``want`` (the per-frame outputs a finish returns), and for BEAT ``align_series`` (2),
    ``onset_source`` ('onset_bt_rms') and ``time_rate`` (22050): ``score_timeline``'s choices.

    Not built: a causal approximation of the normalisation (scores appear at the finish), SRGR online, device-resident lengths,
    growing a slot beyond ``max_seconds``, results left on the device."""
    return ScoreStream(dataset, capacity, max_seconds, sr, device, **options)


def ted_beat_align(beat_mask, onset_frames, onset_count, sigma=TED_BEAT_SIGMA, fps=TED_FPS, sr=16000, hop=512, device=0):
    """``ls_ted_beat_align``: per clip, the beat-consistency sum and the number of motion beats.  beat_mask [B, N] (bool or bytes),
    onset_frames [B, F] int32 and onset_count [B] int32 as ``audio_onsets`` returns them (numpy, or CUDA tensors: then nothing but
    the results' host copies leaves the device).  Returns (align_sum [B] float64, n_beats [B] int32) as host arrays."""
    if len(beat_mask.shape) != 2 or len(onset_frames.shape) != 2:
        raise ValueError(f"expected beat_mask [B, N] and onset_frames [B, F], got {list(beat_mask.shape)} and {list(onset_frames.shape)}")
    B, N, F = int(beat_mask.shape[0]), int(beat_mask.shape[1]), int(onset_frames.shape[1])
    if int(onset_frames.shape[0]) != B or tuple(int(v) for v in onset_count.shape) != (B,):
        raise ValueError(f"one row of onsets and one count per clip: {list(onset_frames.shape)} and {list(onset_count.shape)} for {B} clips")
    m = _lib._Marshal(device, beat_mask, onset_frames, onset_count)
    a = _lib.LsTedAlignArgs()
    a.batch, a.n_frames, a.on_device, a.onset_cols, a.hop = B, N, int(m.on_device), F, int(hop)
    a.fps, a.sigma, a.sr = float(fps), float(sigma), float(sr)
    a.beat_mask, a.onset_frames, a.onset_count = m.u8(beat_mask, (B, N)), m.i32(onset_frames), m.i32(onset_count)
    total, a.align_sum = m.out((B,), np.float64)
    beats, a.n_beats = m.out((B,), np.int32)
    m.ready()
    _lib.call("ls_ted_beat_align", device, C.byref(a))
    if m.on_device:
        return total.cpu().numpy(), beats.cpu().numpy()
    return total, beats


class BeatConsistency:
    """Running beat-alignment (BC) score over clips, as the evaluation loop accumulates it (test_RAG_ted.py:113-127): for every
    audio onset, exp(-min_m (onset - m)^2 / (2 sigma^2)) over the clip's motion beats; clips without a motion beat contribute
    nothing (not even their onsets).  Audio onset times are an input, or are detected on the device from ``audio``
    (``audio_onsets``: the reference's librosa.onset.onset_detect(y, sr=16000, units='time'))."""

    def __init__(self, sigma: float = TED_BEAT_SIGMA):
        self.sigma = float(sigma)
        self.align_sum = 0.0
        self.num_beats = 0
        self.motion_beats_sum = 0

    def push(self, motion_beat_times, audio_beat_times=None, audio=None, sr=16000, device=0, **onset_options):
        """motion_beat_times and audio_beat_times: one sequence of times (seconds) per clip.  ``audio`` [B, L] instead of
        audio_beat_times: the onsets are detected on the device (``onset_options``: pad_mode, fmax, delta of ``audio_onsets``); a
        clip without an onset contributes nothing, as in the reference."""
        if (audio_beat_times is None) == (audio is None):
            raise ValueError("pass either audio_beat_times or audio")
        if audio is not None:
            from .audio_onsets import onset_times
            audio_beat_times = onset_times(audio, sr, device=device, **onset_options)
        if len(motion_beat_times) != len(audio_beat_times):
            raise ValueError("one list of motion beats and one list of audio onsets per clip")
        for mb, ab in zip(motion_beat_times, audio_beat_times):
            self.motion_beats_sum += len(mb)
            if len(mb) == 0:
                continue
            mb = np.asarray(mb, np.float64)
            for a in np.asarray(ab, np.float64).reshape(-1):
                self.align_sum += float(np.exp(-np.min((a - mb) ** 2) / (2.0 * self.sigma * self.sigma)))
            self.num_beats += len(ab)

    def push_timeline(self, beat_mask, onset_frames=None, onset_count=None, audio=None, sr=16000, device=0, frames=None,
                      audio_lengths=None, **onset_options):
        """``push`` for device-resident clips of any length: beat_mask [B, N] as ``ted_postprocess_timeline`` returns it, and either
        the onset slab ``onset_frames`` [B, F] with ``onset_count`` [B] (``audio_onsets``'s onset_raw and count) or ``audio``
        [B, L], whose onsets are then detected on the device.  The clip sums are formed on the device in float64
        (``ls_ted_beat_align``); only the per-clip scalars come to the host, into the accumulators ``push`` feeds.  Returns them:
        (align_sum [B], n_beats [B], onset_count [B]).

        Clips of different lengths: ``frames`` [B] are the clips' valid frames -- beat_mask must be 0 beyond them, which is what
        ``ted_postprocess_timeline(frames=)`` returns -- and ``audio_lengths`` [B] the valid samples of the rows of ``audio``, whose
        onsets then come from ``ls_onsets_ragged``.  ``ls_ted_beat_align`` itself needs no lengths: a frame without a beat
        contributes nothing, so the sums and the running counts hold the valid beats and onsets alone."""
        if (onset_frames is None) == (audio is None):
            raise ValueError("pass either onset_frames (with onset_count) or audio")
        if audio_lengths is not None and audio is None:
            raise ValueError("audio_lengths are the valid samples of audio: pass audio")
        if frames is not None:
            _clip_frames(frames, int(beat_mask.shape[0]), 4, int(beat_mask.shape[1]))
        if audio is not None:
            from . import audio_onsets as ao
            longest = int(audio.shape[1])
            if audio_lengths is not None:
                audio_lengths = _lib.host_lengths(audio_lengths, int(audio.shape[0]), 1, longest, "audio_lengths")
                longest = int(audio_lengths.max())
                audio = audio[:, :longest]                # the row stride: nothing past the longest clip is uploaded
            n_audio_frames = 1 + longest // ao.HOP
            if n_audio_frames > ao.MAX_FRAMES:
                raise NotImplementedError(f"the onset detector takes at most {ao.MAX_FRAMES} audio frames "
                                          f"({ao.MAX_FRAMES * ao.HOP / float(sr):.0f} s at {sr} Hz); this audio has {n_audio_frames}")
            got = ao.audio_onsets(audio, sr, device=device, want=("count", "onset_raw"), lengths=audio_lengths, **onset_options)
            onset_frames, onset_count, counts = got["onset_raw"], got["count"], got["counts"]
        else:
            if onset_count is None:
                raise ValueError("onset_frames needs onset_count [B]")
            counts = onset_count.cpu().numpy() if hasattr(onset_count, "detach") else np.asarray(onset_count)
        total, beats = ted_beat_align(beat_mask, onset_frames, onset_count, sigma=self.sigma, sr=sr, device=device)
        counts = np.asarray(counts).astype(np.int64)
        self.motion_beats_sum += int(beats.sum())
        self.align_sum += float(total.sum())
        self.num_beats += int(counts[beats > 0].sum())
        return total, beats, counts

    def push_score(self, result):
        """A finished TED slot of a ``ScoreStream`` (the dict ``finish`` returns, or every dict of ``close``'s) into the running score,
        with ``push_timeline``'s rule: a slot without a motion beat contributes neither its sum nor its onsets."""
        if not result:
            return
        results = [result[k] for k in sorted(result)] if all(isinstance(v, dict) for v in result.values()) else [result]
        if any("align_sum" not in r or "n_beats" not in r or "count" not in r for r in results):
            raise ValueError("push_score takes the finish dict of a TED score stream (align_sum, n_beats, count)")
        total = np.array([r["align_sum"] for r in results], np.float64)
        beats = np.array([r["n_beats"] for r in results], np.int64)
        counts = np.array([r["count"] for r in results], np.int64)
        self.motion_beats_sum += int(beats.sum())             # push_timeline's accumulation, call for call
        self.align_sum += float(total.sum())
        self.num_beats += int(counts[beats > 0].sum())

    def score(self) -> float:
        return self.align_sum / self.num_beats
