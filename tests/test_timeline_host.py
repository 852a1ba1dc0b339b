"""Post-processing and scoring of stitched timelines, host side: the N-frame restatement (tests/timeline_restatement.py) against the
34-frame restatements and fixtures it generalises (G9, G21), the consistency of every 34-frame slice of the G22 timelines with the
timeline's own curve, and the C-ABI / Python surface of the four timeline entry points.  Nothing here needs a GPU."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import beat_metrics_restatement as R
import timeline_restatement as T
from livelyspeaker_amd import _lib, beat_metrics as bm, long_form, postprocess as pp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ls_ted_post_timeline", "ls_beat_post_timeline", "ls_beat_metrics_timeline", "ls_ted_beat_align")


def _oracle34(sample):
    from oracle import rag_oracle as orc
    return orc.ted_post(sample, pp.TED_MEAN_DIR_VEC, pp.TED_ANGLE_PAIRS, pp.TED_CHANGE_ANGLE, pp.TED_BEAT_THRES, pp.TED_DIR_VEC_PAIRS)


def test_restatement_at_34_frames_reproduces_g9_and_the_g21_restatement(golden):
    g9 = np.load(os.path.join(T.GOLDEN, "post_golden.npz"))
    sample = golden["ted"]["G5_ddpm1000_final"]
    o = T.ted_post(sample)
    assert np.array_equal(o["beat_mask"], g9["G9_beat_mask"]) and o["beat_mask"].sum() > 0
    assert np.array_equal(o["beat_mask"], _oracle34(sample)["beat_mask"])
    g21 = dict(np.load(R.GOLDEN))
    onsets = np.split(g21["onset_times"], g21["onset_offsets"][1:-1])
    want = R.score_batch(g21["pred_euler"], g21["target_euler"], g21["semantic"], onsets)
    got = T.score_batch(g21["pred_euler"], g21["target_euler"], g21["semantic"], onsets)
    assert set(got) == set(want)
    for k in want:
        assert np.array_equal(got[k], want[k]), k


@pytest.mark.parametrize("case", T.CASES)
def test_every_34_frame_slice_is_consistent_with_the_timeline(case):
    """The timeline is one series: what a 34-frame clip cut from it can know (its curve from frame 1 on, its beats at [2, 32]) is the
    timeline's own, exactly."""
    tl = T.g22("ted")[case]
    N = tl.shape[3]
    o = T.ted_post(tl)
    assert o["angle_diff"].shape == (2, N) and not o["angle_diff"][:, 0].any()
    assert not o["beat_mask"][:, [0, 1, N - 1]].any() and o["beat_mask"].sum(1).min() >= 20
    for s in range(N - 34 + 1):
        c = _oracle34(tl[..., s:s + 34])
        assert np.array_equal(c["angle_diff"][:, 1:], o["angle_diff"][:, s + 1:s + 34]), s
        assert np.array_equal(c["beat_mask"][:, 2:33], o["beat_mask"][:, s + 2:s + 33]), s
        assert np.array_equal(c["aligned"], o["aligned"][:, s:s + 34]) and np.array_equal(c["pose"], o["pose"][:, s:s + 34]), s


def test_header_exports_library_and_abi_mirror_agree(tmp_path):
    hdr = open(os.path.join(ROOT, "include", "ls_hip.h")).read()
    lib = ctypes.CDLL(_lib.library_path())
    for name in NAMES:
        assert re.fullmatch(r"[a-z_]+", name)
        assert name in _lib.EXPORTS and re.search(rf"\bint {name}\s*\(", hdr) and hasattr(lib, name), name
    lib.ls_abi_version.restype = ctypes.c_int
    assert lib.ls_abi_version() == 5
    fields = [n for n, _ in _lib.LsTedAlignArgs._fields_]
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ls_hip.h"\nint main(void) {\n'
                   '    printf("%zu", sizeof(ls_ted_align_args));\n' +
                   "".join(f'    printf(" %zu", offsetof(ls_ted_align_args, {n}));\n' for n in fields) +
                   '    printf(" %d %d %d\\n", LS_ABI_VERSION, LS_TIMELINE_MAX_FRAMES, LS_TIMELINE_TILE);\n    return 0;\n}\n')
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    A = _lib.LsTedAlignArgs
    assert got == [ctypes.sizeof(A)] + [getattr(A, n).offset for n in fields] + [5, pp.TIMELINE_MAX_FRAMES, pp.TIMELINE_TILE]


def test_invalid_arguments_are_refused_without_a_launch():
    """Every LS_EINVAL exit sits in front of hipSetDevice: no GPU is needed to be refused."""
    lib = _lib.load_library()
    cfg = pp.ted_post_config()
    x = np.zeros(2 * 47 * 6 * 8, np.float32)
    out = np.zeros(4096 * 64, np.float32)
    px, po = x.ctypes.data, out.ctypes.data
    ted = lambda B, N, c=cfg, src=px: lib.ls_ted_post_timeline(0, 0, B, N, ctypes.byref(c) if c else None, src, po, None, None, None)  # noqa: E731
    assert ted(1, 8, src=None) == -1 and ted(1, 8, c=None) == -1
    assert ted(0, 8) == -1 and ted(1, 3) == -1 and ted(1, pp.TIMELINE_MAX_FRAMES + 1) == -1
    bad = pp.ted_post_config()
    bad.njoints = 17
    assert ted(1, 8, c=bad) == -1                                     # what ls_ted_post refuses
    beat = lambda B, J, N, src=px: lib.ls_beat_post_timeline(0, 0, B, J, N, src, po, None)  # noqa: E731
    assert beat(1, 47, 8, src=None) == -1 and beat(0, 47, 8) == -1 and beat(1, 0, 8) == -1
    assert beat(1, 47, 1) == -1 and beat(1, 47, pp.TIMELINE_MAX_FRAMES + 1) == -1

    al = np.zeros(1, np.float32)
    on = np.array([0.5], np.float32)

    def margs(**kw):
        a = _lib.LsBeatMetricsArgs()
        a.batch, a.njoints, a.order, a.align_series = 1, 47, 2, 2
        for s, j in enumerate(bm.BEAT_SERIES_JOINTS):
            a.series_joint[s] = j
        a.threshold, a.scale, a.sigma, a.fps = 4.0, 1 / 0.165, 0.3, 15.0
        a.pred, a.vel = px, po
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    met = lambda N, **kw: lib.ls_beat_metrics_timeline(0, N, ctypes.byref(margs(**kw)))  # noqa: E731
    assert lib.ls_beat_metrics_timeline(0, 8, None) == -1
    assert met(8, pred=None) == -1 and met(8, batch=0) == -1 and met(8, order=0) == -1
    assert met(5) == -1 and met(7, order=3) == -1                     # n_frames < 2 * order + 2
    assert met(pp.TIMELINE_MAX_FRAMES + 1) == -1
    assert met(8, njoints=27) == -1 and met(8, align_series=6) == -1  # what ls_beat_metrics refuses
    assert met(8, srgr_sum=al.ctypes.data) == -1 and met(8, align=al.ctypes.data) == -1
    for offs in ((0, 0), (1, 2), (0, -1)):
        o = np.array(offs, np.int64)
        assert met(8, onset_offsets=o.ctypes.data, onset_times=on.ctypes.data, align=al.ctypes.data) == -1, offs

    mask = np.zeros((1, 8), np.uint8)
    slab = np.zeros((1, 4), np.int32)
    count = np.array([2], np.int32)
    total, beats = np.zeros(1, np.float64), np.zeros(1, np.int32)

    def aargs(**kw):
        a = _lib.LsTedAlignArgs()
        a.batch, a.n_frames, a.on_device, a.onset_cols, a.hop = 1, 8, 0, 4, 512
        a.fps, a.sigma, a.sr = 15.0, 0.1, 16000.0
        a.beat_mask, a.onset_frames, a.onset_count = mask.ctypes.data, slab.ctypes.data, count.ctypes.data
        a.align_sum, a.n_beats = total.ctypes.data, beats.ctypes.data
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    ali = lambda **kw: lib.ls_ted_beat_align(0, ctypes.byref(aargs(**kw)))  # noqa: E731
    assert lib.ls_ted_beat_align(0, None) == -1
    for name in ("beat_mask", "onset_frames", "onset_count"):
        assert ali(**{name: None}) == -1, name
    assert ali(batch=0) == -1 and ali(n_frames=3) == -1 and ali(n_frames=pp.TIMELINE_MAX_FRAMES + 1) == -1
    assert ali(fps=0.0) == -1 and ali(sigma=-0.1) == -1 and ali(sr=0.0) == -1 and ali(hop=0) == -1 and ali(sigma=float("nan")) == -1
    for c in (-1, 5):
        count[0] = c
        assert ali() == -1, c


def _config(**fields):
    c = pp.ted_post_config()
    for k, v in fields.items():
        if isinstance(v, tuple):
            getattr(c, k)[v[0]] = v[1]
        else:
            setattr(c, k, v)
    return c


BAD_CONFIGS = {"bone_child[0]=17": dict(bone_child=(0, 17)), "bone_parent[0]=-1": dict(bone_parent=(0, -1)), "pair_a[0]=9": dict(pair_a=(0, 9)),
               "pair_b[0]=-1": dict(pair_b=(0, -1)), "n_pose_joints=-1": dict(n_pose_joints=-1), "n_pose_joints=18": dict(n_pose_joints=18),
               "njoints=0": dict(njoints=0), "njoints=17": dict(njoints=17), "n_pairs=9": dict(n_pairs=9)}


def test_both_ted_post_entries_refuse_the_same_configurations():
    """One check (post_params) serves ls_ted_post and ls_ted_post_timeline: a bone or pair index outside a frame is LS_EINVAL (-1) in
    front of hipSetDevice, not an out-of-bounds access on the device.  Without a GPU, reaching hipSetDevice gives LS_EHIP (-3)."""
    lib = _lib.load_library()
    x = np.zeros(2 * 47 * 6 * 34, np.float32)
    out = np.zeros(2 * 34 * 47 * 6, np.float32)
    px, po = x.ctypes.data, out.ctypes.data
    ref = lambda c: ctypes.byref(c) if c is not None else None  # noqa: E731
    ted = lambda c, B=1, src=px: lib.ls_ted_post(0, 0, B, ref(c), src, po, None, None, None)  # noqa: E731
    tl = lambda c, B=1, src=px: lib.ls_ted_post_timeline(0, 0, B, 34, ref(c), src, po, None, None, None)  # noqa: E731
    for name, fields in BAD_CONFIGS.items():
        assert ted(_config(**fields)) == -1 and tl(_config(**fields)) == -1, name
    good = pp.ted_post_config()
    for entry in (ted, tl):
        assert entry(None) == -1 and entry(good, src=None) == -1 and entry(good, B=0) == -1
    beat = lambda B=1, J=47, src=px: lib.ls_beat_post(0, 0, B, J, src, po, None)  # noqa: E731
    assert beat(src=None) == -1 and beat(B=0) == -1 and beat(J=0) == -1


def test_marshal_out_makes_every_output_dtype_on_the_host():
    m = _lib._Marshal(0, np.zeros(3, np.float32))
    assert not m.on_device
    arr, ptr = m.out((2, 3))
    assert arr.dtype == np.float32 and arr.shape == (2, 3)
    for dtype in (np.float32, np.uint8, np.int32, np.float64):
        arr, ptr = m.out((2, 5, 3), dtype)
        assert isinstance(arr, np.ndarray) and arr.dtype == dtype and arr.shape == (2, 5, 3) and arr.flags.c_contiguous
        assert ptr.value == arr.ctypes.data


def test_python_wrappers_refuse_other_shapes():
    with pytest.raises(ValueError, match="timeline"):
        pp.ted_postprocess_timeline(np.zeros((1, 9, 6, 40), np.float32))
    with pytest.raises(ValueError, match="4096"):
        pp.ted_postprocess_timeline(np.zeros((1, 9, 3, 4097), np.float32))
    with pytest.raises(ValueError, match="frames"):
        pp.ted_postprocess_timeline(np.zeros((1, 9, 3, 3), np.float32))
    with pytest.raises(ValueError, match="timeline"):
        pp.beat_postprocess_timeline(np.zeros((1, 47, 3, 40), np.float32))
    with pytest.raises(ValueError, match="Euler planes"):
        bm.beat_metrics_timeline(np.zeros((40, 141), np.float32))


def test_timeline_clips_shapes_and_the_dropped_tail():
    import torch
    x = np.arange(2 * 94 * 5, dtype=np.float32).reshape(2, 94, 5)
    c = long_form.timeline_clips(x)
    assert isinstance(c, np.ndarray) and c.shape == (4, 34, 5)                # 94 = 2 * 34 + 26: the last 26 frames are dropped
    for b in range(2):
        for k in range(2):
            assert np.array_equal(c[2 * b + k], x[b, 34 * k:34 * k + 34])
    t = long_form.timeline_clips(torch.from_numpy(x), stride=30)             # one clip per window of the chain
    assert torch.is_tensor(t) and tuple(t.shape) == (6, 34, 5) and t.is_contiguous()
    assert np.array_equal(t[5].numpy(), x[1, 60:94]) and np.array_equal(t[1].numpy(), x[0, 30:64])
    assert long_form.timeline_clips(x[:, :34]).shape == (2, 34, 5)
    with pytest.raises(ValueError):
        long_form.timeline_clips(x[:, :33])
    with pytest.raises(ValueError):
        long_form.timeline_clips(x, stride=0)


def test_push_timeline_takes_either_audio_or_an_onset_slab():
    bc = pp.BeatConsistency()
    mask = np.zeros((1, 40), bool)
    slab, count, audio = np.zeros((1, 4), np.int32), np.zeros(1, np.int32), np.zeros((1, 16000), np.float32)
    with pytest.raises(ValueError, match="either"):
        bc.push_timeline(mask)
    with pytest.raises(ValueError, match="either"):
        bc.push_timeline(mask, slab, count, audio=audio)
    with pytest.raises(ValueError, match="onset_count"):
        bc.push_timeline(mask, slab)
    long_audio = np.zeros((1, 4096 * 512), np.float32)                        # 4097 audio frames
    with pytest.raises(NotImplementedError, match="4096 audio frames"):
        bc.push_timeline(mask, audio=long_audio)
    with pytest.raises(NotImplementedError, match="4096 audio frames"):
        long_form.score_timeline(np.zeros((1, 9, 3, 40), np.float32), long_audio)
    assert (bc.align_sum, bc.num_beats, bc.motion_beats_sum) == (0.0, 0, 0)
