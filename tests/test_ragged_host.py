"""Clips of different lengths in one call, host side: the tile table (ls_ragged_tiles), the C-ABI surface of the ragged entry points
and every refusal they answer without a device, and the Python plumbing above them (plan_lengths, timeline_clips(frames=), the
ValueErrors of score_timeline and sample_long).  Nothing here needs a GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

from livelyspeaker_amd import _lib, audio_onsets as ao, beat_metrics as bm, long_form, postprocess as pp, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ls_onsets_ragged", "ls_ted_post_timeline_ragged", "ls_beat_post_timeline_ragged", "ls_beat_metrics_timeline_ragged",
         "ls_ragged_tiles")


def i32(v):
    return np.ascontiguousarray(v, np.int32)


def tiles(frames, tile, cap=None):
    lib = _lib.load_library()
    fr = i32(frames)
    n = ctypes.c_int32(-7)
    rc = lib.ls_ragged_tiles(len(fr), fr.ctypes.data, tile, None, None, 0, ctypes.byref(n))
    if rc != 0:
        return rc, None, None
    cap = n.value if cap is None else cap
    clip, start = np.full(max(cap, 1), -9, np.int32), np.full(max(cap, 1), -9, np.int32)
    m = ctypes.c_int32(-7)
    rc = lib.ls_ragged_tiles(len(fr), fr.ctypes.data, tile, clip.ctypes.data, start.ctypes.data, cap, ctypes.byref(m))
    return rc, (n.value, m.value), (clip[:cap], start[:cap])


def test_ragged_tiles_is_the_python_enumeration():
    frames = [1, 63, 64, 65, 129]
    want = [(b, t0) for b, n in enumerate(frames) for t0 in range(0, n, 64)]
    assert len(want) == 1 + 1 + 1 + 2 + 3
    rc, counts, (clip, start) = tiles(frames, 64)
    assert rc == 0 and counts == (len(want), len(want))
    assert list(zip(clip.tolist(), start.tolist())) == want
    for tile in (1, 7, 200):
        rc, counts, (clip, start) = tiles(frames, tile)
        assert rc == 0 and list(zip(clip.tolist(), start.tolist())) == [(b, t0) for b, n in enumerate(frames) for t0 in range(0, n, tile)]
    # one output alone
    lib = _lib.load_library()
    fr, only = i32(frames), np.zeros(len(want), np.int32)
    assert lib.ls_ragged_tiles(5, fr.ctypes.data, 64, None, only.ctypes.data, len(want), None) == 0
    assert only.tolist() == [t0 for _, t0 in want]


def test_ragged_tiles_refusals():
    lib = _lib.load_library()
    frames = [1, 63, 64, 65, 129]
    rc, _, (clip, _) = tiles(frames, 64, cap=7)                               # one short: refused, nothing written
    assert rc == -1 and (clip == -9).all()
    assert tiles([1, 0, 64], 64)[0] == -1 and tiles([5, -3], 64)[0] == -1     # an entry < 1
    assert tiles(frames, 0)[0] == -1 and tiles(frames, -64)[0] == -1
    n = ctypes.c_int32()
    fr = i32(frames)
    assert lib.ls_ragged_tiles(0, fr.ctypes.data, 64, None, None, 0, ctypes.byref(n)) == -1
    assert lib.ls_ragged_tiles(5, None, 64, None, None, 0, ctypes.byref(n)) == -1
    assert lib.ls_ragged_tiles(5, fr.ctypes.data, 64, None, None, 0, None) == 0            # nothing asked for: nothing to refuse


def test_header_exports_and_library_agree_on_the_ragged_names():
    hdr = open(os.path.join(ROOT, "include", "ls_hip.h")).read()
    lib = ctypes.CDLL(_lib.library_path())
    for name in NAMES:
        assert re.fullmatch(r"[a-z_]+", name)
        assert name in _lib.EXPORTS and re.search(rf"\bint {name}\s*\(", hdr) and hasattr(lib, name), name
    lib.ls_abi_version.restype = ctypes.c_int
    assert lib.ls_abi_version() == 5 and re.search(r"#define LS_ABI_VERSION 5\b", hdr)
    assert len(set(_lib.EXPORTS)) == len(_lib.EXPORTS)


def test_invalid_arguments_are_refused_without_a_launch():
    """Every LS_EINVAL exit sits in front of hipSetDevice: no GPU is needed to be refused."""
    lib = _lib.load_library()
    cfg = pp.ted_post_config()
    x = np.zeros(2 * 47 * 6 * 16, np.float32)
    out = np.zeros(4096 * 64, np.float32)
    px, po = x.ctypes.data, out.ctypes.data

    def ted(frames, B=2, N=16, c=cfg, src=px):
        fr = None if frames is None else i32(frames)
        return lib.ls_ted_post_timeline_ragged(0, 0, B, N, None if fr is None else fr.ctypes.data, ctypes.byref(c) if c else None, src, po,
                                               None, None, None)

    assert ted(None) == -1                                                    # a NULL frames
    assert ted([16, 3]) == -1 and ted([0, 16]) == -1 and ted([-1, 16]) == -1  # below the per-clip minimum of 4
    assert ted([16, 17]) == -1                                                # above the row stride
    assert ted([16, 8], src=None) == -1 and ted([16, 8], c=None) == -1        # what the equal-length entry refuses
    assert ted([16, 8], B=0) == -1 and ted([3, 3], N=3) == -1 and ted([8, 8], N=pp.TIMELINE_MAX_FRAMES + 1) == -1
    bad = pp.ted_post_config()
    bad.njoints = 17
    assert ted([16, 8], c=bad) == -1

    def beat(frames, B=2, J=47, N=16, src=px):
        fr = None if frames is None else i32(frames)
        return lib.ls_beat_post_timeline_ragged(0, 0, B, J, N, None if fr is None else fr.ctypes.data, src, po, None)

    assert beat(None) == -1 and beat([16, 1]) == -1 and beat([0, 16]) == -1 and beat([17, 16]) == -1
    assert beat([16, 2], src=None) == -1 and beat([16, 2], B=0) == -1 and beat([16, 2], J=0) == -1
    assert beat([1, 1], N=1) == -1 and beat([2, 2], N=pp.TIMELINE_MAX_FRAMES + 1) == -1

    al = np.zeros(2, np.float32)

    def margs(**kw):
        a = _lib.LsBeatMetricsArgs()
        a.batch, a.njoints, a.order, a.align_series = 2, 47, 2, 2
        for s, j in enumerate(bm.BEAT_SERIES_JOINTS):
            a.series_joint[s] = j
        a.threshold, a.scale, a.sigma, a.fps = 4.0, 1 / 0.165, 0.3, 15.0
        a.pred, a.vel = px, po
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    def met(frames, N=16, **kw):
        fr = None if frames is None else i32(frames)
        return lib.ls_beat_metrics_timeline_ragged(0, N, None if fr is None else fr.ctypes.data, ctypes.byref(margs(**kw)))

    assert lib.ls_beat_metrics_timeline_ragged(0, 16, i32([16, 16]).ctypes.data, None) == -1
    assert met(None) == -1
    assert met([16, 5]) == -1 and met([16, 7], order=3) == -1 and met([17, 16]) == -1      # 2 * order + 2 per clip; the stride
    assert met([16, 6], pred=None) == -1 and met([16, 6], batch=0) == -1 and met([16, 6], order=0) == -1
    assert met([16, 6], N=pp.TIMELINE_MAX_FRAMES + 1) == -1
    assert met([16, 6], njoints=27) == -1 and met([16, 6], align_series=6) == -1
    assert met([16, 6], srgr_sum=al.ctypes.data) == -1 and met([16, 6], align=al.ctypes.data) == -1

    audio = np.zeros((2, 4096), np.float32)
    slab = np.zeros((2, 4096), np.int32)

    def oargs(**kw):
        a = _lib.LsOnsetsArgs()
        a.batch, a.length, a.on_device, a.pad_mode = 2, 4096, 0, 0
        a.sr, a.sr_pick, a.fmax, a.delta = 16000.0, 16000.0, 11025.0, 0.07
        a.audio, a.onset_raw = audio.ctypes.data, slab.ctypes.data
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    def ons(lengths, **kw):
        ln = None if lengths is None else i32(lengths)
        return lib.ls_onsets_ragged(0, ctypes.byref(oargs(**kw)), None if ln is None else ln.ctypes.data)

    assert lib.ls_onsets_ragged(0, None, i32([1, 1]).ctypes.data) == -1
    assert ons(None) == -1                                                    # a NULL lengths
    assert ons([4096, 0]) == -1 and ons([-5, 4096]) == -1 and ons([4097, 4096]) == -1
    assert ons([4096, 1024], pad_mode=1) == -1 and ons([1, 4096], pad_mode=1) == -1        # reflect needs more than 1024 samples per clip
    assert ons([4096, 2000], batch=0) == -1 and ons([4096, 2000], length=0) == -1          # everything ls_onsets refuses
    assert ons([4096, 2000], pad_mode=2) == -1 and ons([4096, 2000], sr=0.0) == -1 and ons([4096, 2000], fmax=0.0) == -1
    assert ons([4096, 2000], sr_pick=0.0) == -1 and ons([4096, 2000], audio=None) == -1
    assert ons([4096, 2000], envelope=audio.ctypes.data) == -1                             # both inputs
    assert ons([4096, 2000], audio=None, envelope=audio.ctypes.data, rms=out.ctypes.data) == -1
    assert ons([4096, 2000], audio=None, envelope=audio.ctypes.data, length=4097) == -1    # more than 4096 frames in a row
    assert ons([4096, 4097], audio=None, envelope=audio.ctypes.data) == -1


def test_python_wrappers_refuse_bad_lengths_before_the_engine():
    tl = np.zeros((2, 9, 3, 40), np.float32)
    with pytest.raises(ValueError, match="frames"):
        pp.ted_postprocess_timeline(tl, frames=[40, 3])
    with pytest.raises(ValueError, match="frames"):
        pp.ted_postprocess_timeline(tl, frames=[40, 41])
    with pytest.raises(ValueError, match="one length per clip"):
        pp.ted_postprocess_timeline(tl, frames=[40])
    with pytest.raises(ValueError, match="frames"):
        pp.beat_postprocess_timeline(np.zeros((2, 47, 6, 40), np.float32), frames=[1, 40])
    with pytest.raises(ValueError, match="frames"):
        bm.beat_metrics_timeline(np.zeros((2, 40, 141), np.float32), frames=[40, 5])
    with pytest.raises(ValueError, match="lengths"):
        ao.audio_onsets(np.zeros((2, 4096), np.float32), lengths=[4096, 0])
    with pytest.raises(ValueError, match="reflect"):
        ao.audio_onsets(np.zeros((2, 4096), np.float32), lengths=[4096, 1024], pad_mode="reflect")
    bc = pp.BeatConsistency()
    with pytest.raises(ValueError, match="audio_lengths"):
        bc.push_timeline(np.zeros((1, 40), bool), np.zeros((1, 4), np.int32), np.zeros(1, np.int32), audio_lengths=[100])
    with pytest.raises(ValueError, match="frames"):
        bc.push_timeline(np.zeros((1, 40), bool), np.zeros((1, 4), np.int32), np.zeros(1, np.int32), frames=[41])
    assert (bc.align_sum, bc.num_beats, bc.motion_beats_sum) == (0.0, 0, 0)


def test_plan_lengths_is_plan_windows_per_clip():
    cfg = synth.CONFIGS["ted"]
    AL, S = int(cfg.audio_len), long_form.AUDIO_STRIDE
    lengths = [1, AL - 1, AL, AL + 1, AL + S, AL + S + 1, AL + 5 * S - 7]
    got = long_form.plan_lengths(lengths, cfg)
    assert got == [(long_form.plan_windows(n, cfg)[0], long_form.plan_windows(n, cfg)[2]) for n in lengths]
    assert [w for w, _ in got] == [1, 1, 1, 2, 2, 3, 6] and [f for _, f in got] == [34 + 30 * (w - 1) for w, _ in got]
    assert long_form.plan_lengths(np.array(lengths[:2], np.int32), cfg) == got[:2]
    with pytest.raises(ValueError):
        long_form.plan_lengths([AL, 0], cfg)


@pytest.mark.parametrize("stride", [34, 30, 7])
def test_timeline_clips_with_frames_is_the_concatenation_of_per_clip_calls(stride):
    import torch
    frames = [33, 34, 35, 94, 131, 64]                                         # a clip too short for one clip, one that fills exactly one
    x = np.arange(6 * 131 * 5, dtype=np.float32).reshape(6, 131, 5)
    for b, n in enumerate(frames):
        x[b, n:] = np.nan                                                      # nothing beyond a clip's frames is gathered
    clips, off = long_form.timeline_clips(x, stride=stride, frames=frames)
    K = [(n - 34) // stride + 1 if n >= 34 else 0 for n in frames]
    assert K[0] == 0 and K[1] == 1
    assert isinstance(clips, np.ndarray) and off.dtype == np.int64 and off.tolist() == [0] + np.cumsum(K).tolist()
    want = np.concatenate([long_form.timeline_clips(x[b:b + 1, :n], stride=stride) for b, n in enumerate(frames) if n >= 34])
    assert clips.shape == (sum(K), 34, 5) and np.array_equal(clips, want) and np.isfinite(clips).all()
    t, off_t = long_form.timeline_clips(torch.from_numpy(x), stride=stride, frames=np.array(frames, np.int32))
    assert torch.is_tensor(t) and t.is_contiguous() and np.array_equal(t.numpy(), want) and np.array_equal(off_t, off)
    none, off0 = long_form.timeline_clips(x[:1], stride=stride, frames=[20])  # every clip too short: an empty pack
    assert none.shape == (0, 34, 5) and off0.tolist() == [0, 0]
    with pytest.raises(ValueError):
        long_form.timeline_clips(x, stride=stride, frames=[34] * 5)
    with pytest.raises(ValueError):
        long_form.timeline_clips(x, stride=stride, frames=[34] * 5 + [132])
    with pytest.raises(ValueError):
        long_form.timeline_clips(x, stride=0, frames=frames)


def test_score_timeline_wants_frames_and_audio_lengths_together():
    tl, audio = np.zeros((2, 9, 3, 40), np.float32), np.zeros((2, 16000), np.float32)
    with pytest.raises(ValueError, match="go together"):
        long_form.score_timeline(tl, audio, frames=[40, 34])
    with pytest.raises(ValueError, match="go together"):
        long_form.score_timeline(tl, audio, audio_lengths=[16000, 8000])
    with pytest.raises(ValueError, match="audio_lengths"):
        long_form.score_timeline(tl, audio, frames=[40, 34], audio_lengths=[16000, 16001])
    with pytest.raises(ValueError, match="frames"):
        long_form.score_timeline(tl, audio, frames=[40, 41], audio_lengths=[16000, 8000])
    long_audio = np.zeros((2, 4096 * 512), np.float32)                         # the 4096-frame limit applies per clip
    with pytest.raises(NotImplementedError, match="4096 audio frames"):
        long_form.score_timeline(tl, long_audio, frames=[40, 34], audio_lengths=[4096 * 512, 16000])


def test_sample_long_refuses_n_windows_with_audio_lengths():
    with pytest.raises(ValueError, match="n_windows or audio_lengths"):
        long_form.sample_long(None, None, np.zeros((2, 70000), np.float32), None, None, None, n_windows=2, audio_lengths=[70000, 40000])
