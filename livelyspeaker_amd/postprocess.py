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

    def score(self) -> float:
        return self.align_sum / self.num_beats
