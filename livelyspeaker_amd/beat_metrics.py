"""The BEAT evaluation metrics (``scripts_beat/utils/metric.py``; ``FIDCalculator`` of ``scripts_beat/dataloaders/data_tools.py``) on the
gfx950 engine: SRGR, L1 diversity, motion beats and BeatAlign run as HIP kernels (``ls_beat_metrics``, ``ls_beat_ldiv``) on the Euler
planes ``ls_beat_post`` writes.  ``from utils import metric`` becomes ``from livelyspeaker_amd import beat_metrics as metric`` for what
``scripts_beat/test_RAG_beat.py`` and ``test_LivelySpeaker_beat.py`` call; ``BeatEvaluator`` is the batched form of their loop bodies,
from which only per-clip scalars come back to the host.

Two documented differences: ``L1div.run`` does not overwrite its argument (the reference replaces the caller's rows by
``|row - mean|``), and audio onsets are an INPUT here, as onset times in seconds -- ``alignment.load_audio`` of this module
raises; ``audio_onsets.alignment`` is the subclass that detects them on the device (``ls_onsets``), and ``BeatEvaluator.push`` takes
``audio=`` through it (``postprocess.BeatConsistency`` does the same on TED).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from .ted_evaluator import EmbeddingSpaceEvaluator, _Moments

T, V = 34, 33
#: joints of the six velocity series in ``load_pose``'s return order (right arm, right shoulder, right wrist, left arm, left shoulder,
#: left wrist): Euler columns [9:18] and [75:84] are joints 3, 4, 5 and 25, 26, 27, which the reference labels shoulder, arm, wrist
BEAT_SERIES_JOINTS = (4, 3, 5, 26, 25, 27)
SRGR_SCALE = 1 / 0.165        # metric.py:41
BEAT_FPS = 15


def frames_to_time(frames, sr=22050, hop_length=512):
    """``librosa.frames_to_time`` with librosa's defaults, which the reference calls it with (on 16 kHz audio; the defaults are part of
    the score)."""
    return np.asarray(frames) * hop_length / float(sr)


def _ragged(onset_times, batch):
    """One sequence of onset times per clip -> (flat float32, offsets int64 [B + 1]); a clip without an onset has no score."""
    if len(onset_times) != batch:
        raise ValueError(f"one sequence of onset times per clip: got {len(onset_times)} for {batch} clips")
    rows = [np.asarray(o.detach().cpu().numpy() if hasattr(o, "detach") else o, dtype=np.float32).reshape(-1) for o in onset_times]
    for b, r in enumerate(rows):
        if r.size == 0:
            raise ValueError(f"clip {b} has no audio onset: its alignment score is 0 / 0")
    off = np.zeros(batch + 1, np.int64)
    np.cumsum([r.size for r in rows], out=off[1:])
    return np.concatenate(rows), off


def beat_metrics(pred_euler, target_euler=None, semantic=None, onset_times=None, *, joints=47, threshold=4.0, scale=SRGR_SCALE,
                 series_joints=BEAT_SERIES_JOINTS, order=2, sigma=0.3, fps=BEAT_FPS, align_series=2, device=0,
                 want=("success", "srgr_sum", "vel", "beat_mask", "align"), _ragged_onsets=None):
    """``ls_beat_metrics`` on Euler planes [B, 34, joints*3] in degrees (numpy, or CUDA tensors: then the outputs stay on the device).
    ``onset_times``: one sequence of seconds per clip.  Returns a dict of the outputs named in ``want`` whose inputs were given:
    success [B,34,J] and beat_mask [B,6,33] as bytes, srgr_sum [B], vel [B,6,33], align [B]."""
    return _beat_metrics(None, pred_euler, target_euler, semantic, onset_times, joints, threshold, scale, series_joints, order, sigma, fps,
                         align_series, device, want, _ragged_onsets)


def beat_metrics_timeline(pred_euler, target_euler=None, semantic=None, onset_times=None, *, joints=47, threshold=4.0, scale=SRGR_SCALE,
                          series_joints=BEAT_SERIES_JOINTS, order=2, sigma=0.3, fps=BEAT_FPS, align_series=2, device=0,
                          want=("success", "srgr_sum", "vel", "beat_mask", "align"), _ragged_onsets=None, frames=None):
    """``beat_metrics`` on the Euler planes of a stitched timeline, [B, N, joints*3] with 2 * order + 2 <= N <= 4096
    (``ls_beat_metrics_timeline``): every clip is one series of N frames.  success [B,N,J] and beat_mask [B,6,N-1] as bytes,
    srgr_sum [B], vel [B,6,N-1], align [B]; semantic, if given, is [B, N]; a motion beat at velocity index m lies at m / fps seconds.
    ``frames`` (a host sequence [B], each in [2 * order + 2, N]): the clips' valid frames (``ls_beat_metrics_timeline_ragged``).  N
    is then the row stride; clip b's numbers are bit for bit those of the clip alone at its own length (mode='clip' clamps at its own
    last velocity, srgr_sum[b] and align[b] are its own), and success, vel and beat_mask are 0 beyond its valid range."""
    if len(pred_euler.shape) != 3:
        raise ValueError(f"expected Euler planes [B, N, joints*3], got {list(pred_euler.shape)}")
    if frames is not None:
        frames = _lib.host_lengths(frames, int(pred_euler.shape[0]), 2 * int(order) + 2, int(pred_euler.shape[1]), "frames")
    return _beat_metrics(int(pred_euler.shape[1]), pred_euler, target_euler, semantic, onset_times, joints, threshold, scale, series_joints,
                         order, sigma, fps, align_series, device, want, _ragged_onsets, frames)


def _beat_metrics(n_frames, pred_euler, target_euler, semantic, onset_times, joints, threshold, scale, series_joints, order, sigma, fps,
                  align_series, device, want, _ragged_onsets, frames=None):
    """All entry points: ``n_frames`` None is the 34-frame ``ls_beat_metrics``, ``frames`` (host int32 [B]) the ragged timeline call."""
    B = int(pred_euler.shape[0])
    T = 34 if n_frames is None else n_frames
    V = T - 1
    m = _lib._Marshal(device, pred_euler, target_euler, semantic)
    a = _lib.LsBeatMetricsArgs()
    a.batch, a.njoints, a.on_device, a.order, a.align_series = B, int(joints), int(m.on_device), int(order), int(align_series)
    for s, j in enumerate(series_joints):
        a.series_joint[s] = int(j)
    a.threshold, a.scale, a.sigma, a.fps = float(threshold), float(scale), float(sigma), float(fps)
    shape = (B, T, joints * 3)
    a.pred, a.target, a.semantic = m.f32(pred_euler, shape), m.f32(target_euler, shape), m.f32(semantic, (B, T))
    if onset_times is not None:
        flat, off = _ragged_onsets or _ragged(onset_times, B)       # BeatEvaluator.push has checked them already
        a.onset_times = m.f32(flat, (flat.size,))
        a.onset_offsets = off.ctypes.data_as(C.c_void_p)

    out = {}
    if target_euler is not None:
        if "success" in want:
            out["success"], a.success = m.out((B, T, joints), np.uint8)
        if "srgr_sum" in want:
            out["srgr_sum"], a.srgr_sum = m.out((B,))
    if "vel" in want:
        out["vel"], a.vel = m.out((B, 6, V))
    if "beat_mask" in want:
        out["beat_mask"], a.beat_mask = m.out((B, 6, V), np.uint8)
    if onset_times is not None and "align" in want:
        out["align"], a.align = m.out((B,))
    m.ready()
    if n_frames is None:
        _lib.call("ls_beat_metrics", device, C.byref(a))
    elif frames is None:
        _lib.call("ls_beat_metrics_timeline", device, n_frames, C.byref(a))
    else:
        _lib.call("ls_beat_metrics_timeline_ragged", device, n_frames, frames.ctypes.data_as(C.c_void_p), C.byref(a))
    return out


def l1div_sum(rows, device=0) -> float:
    """``ls_beat_ldiv``: sum of |x - column mean| over rows [N, D] (numpy or a CUDA tensor), which are only read."""
    m = _lib._Marshal(device, rows)
    n, d = int(rows.shape[0]), int(rows.shape[1])
    total = C.c_double()
    px = m.f32(rows, (n, d))
    m.ready()
    _lib.call("ls_beat_ldiv", device, int(m.on_device), n, d, px, C.byref(total))
    return float(total.value)


class L1div(object):
    """metric.py:12-24.  ``run`` leaves ``results`` as it is (the reference overwrites it with |row - mean|)."""

    def __init__(self, device=0):
        self.counter = 0
        self.sum = 0
        self.device = device

    def run(self, results):
        self.counter += results.shape[0]
        self.sum += l1div_sum(results, self.device)

    def avg(self):
        return self.sum / self.counter


class SRGR(object):
    """metric.py:27-51: the success mask and the weighted sum per clip on the GPU, the running average in Python floats.  ``run``
    takes whole clips (a multiple of 34 rows, which is what both scripts pass); the reference takes any number of rows."""

    def __init__(self, threshold=0.1, joints=47, device=0):
        self.threshold = threshold
        self.pose_dimes = 3
        self.joints = joints
        self.counter = 0
        self.sum = 0
        self.device = device

    def run(self, results, targets, semantic):
        width = self.joints * self.pose_dimes
        if results.shape[0] % T:
            raise ValueError(f"SRGR.run scores whole clips of {T} frames: got {results.shape[0]} rows")
        results, targets, semantic = results.reshape(-1, T, width), targets.reshape(-1, T, width), semantic.reshape(-1, T)
        got = beat_metrics(results, targets, semantic, joints=self.joints, threshold=self.threshold, device=self.device, want=("srgr_sum",))
        return self.add(got["srgr_sum"], results.shape[0] * T)

    def add(self, srgr_sum, rows):
        """Account for a batch from its per-clip sums (``srgr_sum`` of ``ls_beat_metrics``) over ``rows`` frames."""
        s = srgr_sum.detach().cpu().numpy() if hasattr(srgr_sum, "detach") else np.asarray(srgr_sum)
        rate = float(s.astype(np.float64).sum()) / (rows * self.joints)
        self.counter += rows
        self.sum += rate * rows
        return rate

    def avg(self):
        if self.counter == 0:
            return 0
        return self.sum / self.counter


class alignment(object):
    """metric.py:53-193 for what the two BEAT scripts call.  Audio beats are given as onset TIMES in seconds
    (``frames_to_time(onset_frames)`` for librosa frame indices)."""

    def __init__(self, sigma, order, device=0):
        self.sigma = sigma
        self.order = order
        self.device = device
        self.times = self.oenv = self.S = self.rms = None
        self.pose_data = []

    def load_audio(self, wave, t_start, t_end, without_file=False, sr_audio=16000):
        raise NotImplementedError("load_audio is librosa onset detection, which is not part of this package: detect the onsets with "
                                  "librosa and pass calculate_align their times (frames_to_time(onset_bt_rms))")

    def load_pose(self, pose, t_start, t_end, pose_fps, without_file=False):
        """pose [34, 141] Euler degrees -> the six ``(indices,)`` tuples, in the reference's return order."""
        if t_start != 0 or t_end * pose_fps < V:
            raise NotImplementedError("t_start != 0 or a t_end that cuts the clip: the reference slices only its right-hand series, "
                                      "relative to the cut, and neither script asks for it")
        pose = pose.detach().cpu().numpy() if hasattr(pose, "detach") else np.asarray(pose)
        if pose.ndim != 2 or pose.shape[0] != T or pose.shape[1] % 3:
            raise ValueError(f"pose must be [{T}, joints*3], got {list(pose.shape)}")
        mask = beat_metrics(pose[None], joints=pose.shape[1] // 3, order=self.order, device=self.device, want=("beat_mask",))["beat_mask"]
        return tuple((np.nonzero(mask[0, s])[0],) for s in range(6))

    @staticmethod
    def motion_frames2time(vel, offset, pose_fps):
        return vel[0] / pose_fps + offset

    @staticmethod
    def GAHR(a, b, sigma):
        """Mean over the audio times ``b`` of exp(-min_a |a - b|^2 / (2 sigma^2)); a handful of host numbers, in float64."""
        a = np.asarray(a, np.float64).reshape(-1)
        b = np.asarray(b, np.float64).reshape(-1)
        if a.size == 0:
            return 0.0
        d = np.abs(a[None, :] - b[:, None]).min(axis=1)
        return float(np.exp(-(d * d) / (2 * sigma ** 2)).sum() / len(b))

    def calculate_align(self, onset_raw, onset_bt, onset_bt_rms, beat_right_arm, beat_right_shoulder, beat_right_wrist, beat_left_arm,
                        beat_left_shoulder, beat_left_wrist, pose_fps=15):
        """The reference's signature; ``onset_bt_rms`` holds onset times in seconds and only the right wrist's beats are read (:189)."""
        pose_bt = self.motion_frames2time(np.array([list(beat_right_wrist[0])]), 0, pose_fps)
        return self.GAHR(pose_bt, onset_bt_rms, self.sigma)


class FIDCalculator(object):
    """``frechet_distance`` and ``get_diversity`` of data_tools.FIDCalculator on the evaluator's shared statistics (the BVH-file
    methods are not built)."""

    @staticmethod
    def frechet_distance(samples_A, samples_B):
        a, b = _Moments(), _Moments()
        a.add(samples_A)
        b.add(samples_B)
        try:
            return EmbeddingSpaceEvaluator.calculate_frechet_distance(a.mean, a.covariance(), b.mean, b.covariance())
        except ValueError:              # data_tools.py:236-237
            return 1e+10

    calculate_frechet_distance = staticmethod(EmbeddingSpaceEvaluator.calculate_frechet_distance)

    def get_diversity(generated_feat_list):
        """Called on the class, as the reference's scripts do; the pairing is drawn with ``torch.randperm`` where the reference draws it."""
        ev = object.__new__(EmbeddingSpaceEvaluator)
        ev.generated_feat_list = list(generated_feat_list)
        return ev.get_diversity_scores()


class BeatEvaluator:
    """The loop bodies of test_RAG_beat.py:86-121 and test_LivelySpeaker_beat.py:132-177 for one batch at a time, on the device:
    ``ls_beat_post`` on the sampled and the target clips, ``ls_beat_metrics`` and ``ls_beat_ldiv`` on the Euler planes and, with
    ``eval_model`` (a ``HalfEmbeddingNet``), the features of both for FID and diversity."""

    def __init__(self, eval_model=None, srgr_threshold=4, joints=47, sigma=0.3, order=2, pose_fps=BEAT_FPS, device=0):
        self.eval_model = eval_model
        self.joints, self.sigma, self.order, self.pose_fps, self.device = joints, sigma, order, pose_fps, device
        self.srgr_calculator = SRGR(srgr_threshold, joints, device)
        self.l1_calculator = L1div(device)
        self.align = 0.0
        self.total_length = 0
        self.latent_out_all, self.latent_ori_all = [], []
        self._out, self._ori = _Moments(), _Moments()

    def push(self, sample, tar_pose, semantic=None, onset_times=None, audio=None, sr_audio=16000, **onset_options):
        """sample [B, joints, 6, 34] as the sampler returns it, tar_pose [B, 34, joints*6] (both CUDA tensors), semantic [B, 34] or
        None (no SRGR), onset_times: one sequence of seconds per clip or None (no alignment).  ``audio`` [B, L] instead of
        onset_times: the onsets are detected on the device as ``alignment.load_audio`` finds them (``audio_onsets``; its pad_mode
        and fmax pass through ``onset_options``) and scored as frames_to_time(onset_bt_rms).  Returns this batch's per-clip scalars."""
        from .postprocess import beat_postprocess
        B, J = int(sample.shape[0]), self.joints
        if tuple(sample.shape[1:]) != (J, 6, T) or tuple(tar_pose.shape) != (B, T, J * 6):
            raise ValueError(f"expected sample [B, {J}, 6, {T}] and tar_pose [B, {T}, {J * 6}], got {list(sample.shape)} and "
                             f"{list(tar_pose.shape)}")
        if audio is not None:
            if onset_times is not None:
                raise ValueError("pass either onset_times or audio")
            from . import audio_onsets
            onset_times = audio_onsets.onset_times(audio, sr_audio, 22050, which="onset_bt_rms", time_sr=22050, device=self.device,
                                                   **onset_options)
        # a clip without an onset is refused before anything is launched
        ragged = _ragged(onset_times, B) if onset_times is not None else None
        pred = beat_postprocess(sample, self.device)
        target = None
        if semantic is not None:        # the target's Euler planes serve SRGR alone
            target = beat_postprocess(tar_pose.reshape(B, T, J, 6).permute(0, 2, 3, 1), self.device)["pred_euler"]
        got = beat_metrics(pred["pred_euler"], target, semantic, onset_times, joints=J, threshold=self.srgr_calculator.threshold,
                           order=self.order, sigma=self.sigma, fps=self.pose_fps, device=self.device, want=("srgr_sum", "align"),
                           _ragged_onsets=ragged)
        res = {}
        if "srgr_sum" in got:
            res["srgr_rate"] = self.srgr_calculator.add(got["srgr_sum"], B * T)
        if "align" in got:
            al = got["align"]
            res["align"] = al.detach().cpu().numpy() if hasattr(al, "detach") else al
            self.align += float(res["align"].astype(np.float64).sum())
        self.l1_calculator.run(pred["pred_euler"].reshape(B * T, J * 3))
        self.total_length += B
        if self.eval_model is not None:
            for poses, keep, mom in ((pred["decoded_motions"], self.latent_out_all, self._out), (tar_pose, self.latent_ori_all, self._ori)):
                f = self.eval_model(poses)
                f = f.detach().cpu().numpy() if hasattr(f, "detach") else np.asarray(f)
                keep.append(f)
                mom.add(f)
        return res

    def scores(self) -> dict:
        """fid, align (sum over clips / clips pushed), diversity, srgr (``SRGR.avg()``) and l1div (``L1div.avg()``); fid and diversity
        are None without ``eval_model``."""
        if self.total_length == 0:
            raise ValueError("no batch pushed")
        fid = diversity = None
        if self.latent_out_all:
            fid = EmbeddingSpaceEvaluator.calculate_frechet_distance(self._out.mean, self._out.covariance(), self._ori.mean,
                                                                     self._ori.covariance())
            diversity = FIDCalculator.get_diversity(self.latent_out_all)
        return {"fid": fid, "align": self.align / self.total_length, "diversity": diversity, "srgr": self.srgr_calculator.avg(),
                "l1div": self.l1_calculator.avg()}
