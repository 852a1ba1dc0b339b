"""Host side of ``long_form.edit_long(mask=)``: the plan of an element mask (``edit_plan(mask=)`` / ``edit_plan_compact(mask=)`` ->
ls_long_edit_plan_mask) against the range plans on random rectangles and against a restatement on random masks; the seam frames; the
refusals, ahead of any engine; ``edit_window(mask=)`` against a three-line statement of the rule; ``edit_mask`` / ``keyframe_mask``;
tests/edit_mask_plan_main.cpp -- a stand-alone program around the plan's unit -- under the host sanitizers; the ABI, which only
grew.  No GPU."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

from livelyspeaker_amd import _lib, build, long_form, synth
from test_long_form_host import _no_engine, _parts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T, NPRE, S = 34, 4, 30
B, W = 4, 3
N = T + (W - 1) * S


def gpu_test_mask(cfg):
    """The test mask of tests/test_gpu_long_edit_mask.py, bool [B, J, F, N], True = editable: clip 0 has two stretches with other joints
    in each -- [26, 38) across the seam of windows 0 and 1 (frames 30..33 are window 0's and window 1's prefix) and [70, 94) to the last
    frame, with frame 80 pinned inside it; clip 1 one feature of one joint at one frame window 1 owns; clip 2 nothing; clip 3 frame 0."""
    J, F = cfg.njoints, cfg.nfeats
    m = np.zeros((B, J, F, N), bool)
    m[0, :J // 2, :, 26:38] = True
    m[0, J // 2:, :, 70:94] = True
    m[0, :, :, 80] = False
    m[1, J - 1, F - 1, 45] = True
    m[3, :, :, 0] = True
    return m


GPU_TEST_PLAN = [(0, [0, 3]), (1, [0, 1]), (2, [0])]


def _restated(m3, Wn, frames=None):
    """pair (b, w) iff some channel of b is set on a frame w S + f that w owns; window w runs iff it has a pair, clips ascending"""
    f = np.arange(T)
    plan = []
    for w in range(Wn):
        own = (f >= NPRE) | (w == 0)
        rows = [b for b in range(m3.shape[0]) if m3[b][:, w * S + f[own]].any() and (frames is None or w < (frames[b] - T) // S + 1)]
        if rows:
            plan.append((w, rows))
    return plan


def test_the_plan_of_the_gpu_test_mask():
    for cfg in (synth.TED, synth.BEAT):
        m = gpu_test_mask(cfg)
        assert long_form.edit_plan_compact(None, W, cfg, mask=m) == GPU_TEST_PLAN
        assert long_form.edit_plan(None, W, cfg, mask=m) == [0, 1, 2]
        assert long_form.edit_plan_compact(None, W, cfg, mask=torch.from_numpy(m)) == GPU_TEST_PLAN        # torch or numpy
        assert _restated(m.reshape(B, -1, N), W) == GPU_TEST_PLAN
    m = gpu_test_mask(synth.TED)
    m[0, :, :, 34:38] = False                                   # only the seam frames 26..33 are left of the first stretch: window 0's alone
    assert long_form.edit_plan_compact(None, W, synth.TED, mask=m) == [(0, [0, 3]), (1, [1]), (2, [0])]


@pytest.mark.parametrize("ds", ["ted", "beat"])
def test_a_rectangle_mask_plans_what_the_ranges_plan(ds):
    cfg = synth.CONFIGS[ds]
    rng = np.random.default_rng(20261021)
    seen_empty = seen_ragged = 0
    for _ in range(300):
        Bn, Wn = int(rng.integers(1, 6)), int(rng.integers(1, 6))
        Nn = T + (Wn - 1) * S
        frames = None
        if rng.random() < 0.5:
            frames = T + S * rng.integers(0, Wn, Bn)
            frames[int(rng.integers(0, Bn))] = Nn
        most = np.full(Bn, Nn) if frames is None else frames
        lo = rng.integers(0, most + 1)
        hi = np.minimum(most, lo + rng.integers(0, 50, Bn))
        sel = None
        if rng.random() < 0.5:
            sel = rng.random((Bn, cfg.njoints)) < 0.3
            sel[rng.random(Bn) < 0.3] = False
        ranges = np.stack([lo, hi], 1)
        m = long_form.edit_mask(ranges, sel, Nn, cfg)
        assert m.shape == (Bn, cfg.njoints, cfg.nfeats, Nn) and m.dtype == np.bool_
        want = long_form.edit_plan_compact(ranges, Wn, cfg, joints=sel, frames=frames)
        assert long_form.edit_plan_compact(None, Wn, cfg, frames=frames, mask=m) == want, (lo, hi, Wn, frames)
        if frames is None and want:
            folded = hi if sel is None else np.where(sel.any(axis=1), hi, lo)
            assert long_form.edit_plan(None, Wn, cfg, mask=m) == long_form.edit_plan(np.stack([lo, folded], 1), Wn, cfg)
        seen_empty += not want
        seen_ragged += frames is not None and bool(want)
    assert seen_empty and seen_ragged


def test_random_masks_agree_with_the_restatement():
    cfg = synth.TED
    rng = np.random.default_rng(7)
    for _ in range(200):
        Bn, Wn = int(rng.integers(1, 6)), int(rng.integers(1, 6))
        Nn = T + (Wn - 1) * S
        m = np.zeros((Bn, cfg.njoints, cfg.nfeats, Nn), bool)
        for _ in range(int(rng.integers(0, 5))):
            m[rng.integers(0, Bn), rng.integers(0, cfg.njoints), rng.integers(0, cfg.nfeats), rng.integers(0, Nn)] = True
        assert long_form.edit_plan_compact(None, Wn, cfg, mask=m) == _restated(m.reshape(Bn, -1, Nn), Wn)


def test_the_prefix_frames_of_a_window_plan_the_window_before():
    cfg = synth.TED
    for w in range(1, W):
        m = np.zeros((2, N), bool)
        m[1, w * S:w * S + NPRE] = True                         # window w covers them, window w - 1 owns them
        assert long_form.edit_plan_compact(None, W, cfg, mask=m) == [(w - 1, [1])]
        assert long_form.edit_plan(None, W, cfg, mask=m) == [w - 1]
        m[1, w * S + NPRE] = True
        assert long_form.edit_plan_compact(None, W, cfg, mask=m) == [(w - 1, [1]), (w, [1])]


def test_mask_shapes_and_helpers():
    cfg = synth.TED
    J, F = cfg.njoints, cfg.nfeats
    one = np.zeros(N, bool)
    one[40:45] = True
    want = np.zeros((B, J * F, N), bool)
    want[:, :, 40:45] = True
    for m in (one, np.broadcast_to(one, (B, N)), np.broadcast_to(one, (B, J, N)), np.broadcast_to(one, (B, J, F, N)), np.broadcast_to(one, (1, J, F, N)), one[None, :],
              torch.from_numpy(one)):
        got = long_form._edit_mask(m, B, cfg, N)
        assert got.dtype == torch.bool and got.shape == (B, J * F, N) and got.is_contiguous() and np.array_equal(got.numpy(), want)
    for bad in (one[:-1], np.zeros((B + 1, N), bool), np.zeros((B, J + 1, N), bool), np.zeros((B, J, F + 1, N), bool), np.zeros((B, J, F, N, 1), bool),
                np.zeros((), bool)):
        with pytest.raises(ValueError, match="mask must be"):
            long_form._edit_mask(bad, B, cfg, N)
    for bad in (one.astype(np.uint8), one.astype(np.float32), torch.from_numpy(one).int()):
        with pytest.raises(ValueError, match="bool"):
            long_form._edit_mask(bad, B, cfg, N)
    # edit_mask: the rectangle
    sel = np.zeros((2, J), bool)
    sel[0, 1] = sel[1, 2] = True
    m = long_form.edit_mask(np.array([(3, 9), (90, 94)]), sel, N, cfg)
    assert m.sum() == F * (6 + 4) and m[0, 1, :, 3:9].all() and m[1, 2, :, 90:].all()
    assert long_form.edit_mask((3, 9), None, N, cfg).shape == (1, J, F, N) and long_form.edit_mask((3, 9), sel, N, cfg).shape == (2, J, F, N)
    with pytest.raises(ValueError):
        long_form.edit_mask((3, N + 1), None, N, cfg)
    # keyframe_mask: everything but the pins, optionally inside ranges, optionally on some joints
    k = long_form.keyframe_mask(N, [0, 40, 93], cfg)
    assert k.shape == (1, J, F, N) and k.dtype == np.bool_ and k.sum() == J * F * (N - 3) and not k[..., [0, 40, 93]].any()
    pin = np.zeros(J, bool)
    pin[[0, 3]] = True
    k = long_form.keyframe_mask(N, [40], cfg, joints=pin, within=[(30, 50), (60, 70)])
    assert k.sum() == J * F * 30 - 2 * F and not k[0, [0, 3], :, 40].any() and k[0, 1, :, 40].all() and not k[..., :30].any() and not k[..., 50:60].any()
    assert long_form.keyframe_mask(N, [], cfg, within=(10, 12)).sum() == J * F * 2
    for bad in ([N], [-1]):
        with pytest.raises(ValueError, match="pinned_frames"):
            long_form.keyframe_mask(N, bad, cfg)
    with pytest.raises(ValueError, match="within"):
        long_form.keyframe_mask(N, [1], cfg, within=(5, N + 1))


@pytest.mark.parametrize("ds", ["ted", "beat"])
def test_edit_window_planes_are_the_rule(ds):
    cfg = synth.CONFIGS[ds]
    J, F = cfg.njoints, cfg.nfeats
    rng = np.random.default_rng(3)
    timeline = torch.from_numpy(rng.standard_normal((B, J, F, N)).astype(np.float32))
    seed = torch.from_numpy(rng.standard_normal((B, J, F, NPRE)).astype(np.float32))
    for m in (gpu_test_mask(cfg), rng.random((B, J, F, N)) < 0.2):
        for w in range(W):
            origin_x, keep, motion = long_form.edit_window(timeline, w, None, None, seed, cfg, mask=m)
            # the rule, in three lines: set in the mask, on a frame the window owns
            n = w * S + np.arange(T)
            own = (np.arange(T) >= NPRE) | (w == 0)
            editable = m[..., n] & own
            assert keep.dtype == torch.bool and np.array_equal(keep.numpy(), ~editable)
            assert torch.equal(motion, timeline[..., w * S:w * S + T]) and motion.is_contiguous()
            assert torch.equal(origin_x[..., :NPRE], seed if w == 0 else motion[..., :NPRE]) and not origin_x[..., NPRE:].any()
    # the rectangle as a mask gives the range form's planes
    ranges = np.array([(20, 50), (0, 0), (70, 80), (40, 72)])
    sel = rng.random((B, J)) < 0.5
    for w in range(W):
        a = long_form.edit_window(timeline, w, ranges, sel, seed, cfg)
        b = long_form.edit_window(timeline, w, None, None, seed, cfg, mask=long_form.edit_mask(ranges, sel, N, cfg))
        assert all(torch.equal(x, y) for x, y in zip(a, b))
    with pytest.raises(ValueError, match="excludes"):
        long_form.edit_window(timeline, 0, ranges, None, seed, cfg, mask=gpu_test_mask(cfg))


def test_plan_refusals():
    cfg = synth.TED
    m = np.zeros((2, N), bool)
    assert long_form.edit_plan_compact(None, W, cfg, mask=m) == []            # an empty plan is an empty list ...
    with pytest.raises(ValueError, match="empty"):
        long_form.edit_plan(None, W, cfg, mask=m)                             # ... and no window to run
    m[1, 34] = True
    assert long_form.edit_plan_compact(None, W, cfg, mask=m, frames=[94, 64]) == [(1, [1])]
    with pytest.raises(ValueError, match="frames"):
        long_form.edit_plan_compact(None, W, cfg, mask=m, frames=[94, 34])    # set at the clip's first frame beyond its own
    with pytest.raises(ValueError, match="frames"):
        long_form.edit_plan_compact(None, W, cfg, mask=m, frames=[94, 65])    # no stitched length
    with pytest.raises(ValueError, match="excludes"):
        long_form.edit_plan_compact((0, 4), W, cfg, mask=m)
    with pytest.raises(ValueError, match="excludes"):
        long_form.edit_plan_compact(None, W, cfg, joints=np.ones(cfg.njoints, bool), mask=m)
    with pytest.raises(ValueError, match="excludes"):
        long_form.edit_plan((0, 4), W, cfg, mask=m)
    with pytest.raises(ValueError):
        _lib.long_edit_plan_mask(np.zeros((2, 3, N + 1), bool), W)


@pytest.mark.parametrize("ds", ["ted", "beat"])
def test_edit_long_mask_refusals_come_before_any_engine(ds, monkeypatch):
    _no_engine(monkeypatch)
    cfg, model, diffusion = _parts(ds)
    Bn, Wn = 2, 2
    Nn = T + S
    y = synth.make_long_cond(cfg, Bn, Wn)
    emo = {"emo": y["emo"]} if ds == "beat" else {}
    timeline = np.zeros((Bn, cfg.njoints, cfg.nfeats, Nn), np.float32)
    L = y["audio"].shape[1]
    lens = [L, 20000]                                                       # W_b = (2, 1): frames (64, 34)
    some = np.zeros((Bn, Nn), bool)
    some[:, 10:20] = True

    def call(frames=None, mask=some, **kw):
        return long_form.edit_long(diffusion, model, timeline, frames, y["audio"], y["seed_poses"], y["vid_indices"], y["scale"], mask=mask, **emo, **kw)

    with pytest.raises(ValueError, match="empty"):
        call(mask=np.zeros((Bn, Nn), bool))
    with pytest.raises(ValueError, match="empty"):
        call(mask=np.zeros(Nn, bool), compact=True)
    beyond = some.copy()
    beyond[1, 34] = True
    with pytest.raises(ValueError, match="frames\\[b\\]"):
        call(mask=beyond, audio_lengths=lens)                               # clip 1 holds 34 frames
    with pytest.raises(ValueError, match="frames=None and joints=None"):
        call(frames=(10, 20))
    with pytest.raises(ValueError, match="frames=None and joints=None"):
        call(joints=np.ones(cfg.njoints, bool))
    with pytest.raises(ValueError, match="mask="):
        call(mask=None)                                                     # neither frames nor a mask
    for bad in (np.zeros((Bn, Nn + 1), bool), np.zeros((Bn + 1, Nn), bool), np.zeros((Bn, cfg.njoints + 1, Nn), bool), np.zeros((Bn, 1, 1, 1, Nn), bool)):
        with pytest.raises(ValueError, match="mask must be"):
            call(mask=bad)
    for bad in (some.astype(np.uint8), some.astype(np.float32)):
        with pytest.raises(ValueError, match="bool"):
            call(mask=bad)
    with pytest.raises(ValueError, match="compact=False"):
        call(audio_lengths=lens, compact=False)
    with pytest.raises(ValueError):
        call(sampler="plms")
    diffusion.noise_source = "torch_device"
    try:
        with pytest.raises(NotImplementedError):
            call()
    finally:
        diffusion.noise_source = "torch_cpu"


def test_edit_mask_plan_main_on_its_edges_under_asan_and_ubsan(tmp_path):
    """tests/edit_mask_plan_main.cpp with the plan's unit, as plain C++ with the host sanitizers linked statically: a child process of
    its own, nothing preloaded, nothing inside Python, no GPU."""
    exe = str(tmp_path / "edit_mask_plan")
    made = subprocess.run([build.hipcc_path(), "-x", "c++", "-std=c++17", "-O1", "-g", "-fno-gpu-sanitize", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "edit_mask_plan_main.cpp"),
                           os.path.join(ROOT, "livelyspeaker_amd", "csrc", "ls_chain_plan.cpp"), "-o", exe], capture_output=True, text=True)
    assert made.returncode == 0, made.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr
    assert run.stderr == "", run.stderr


NEW_EXPORTS = ("ls_long_edit_plan_mask", "ls_long_edit_mask", "ls_long_prepare_edit_mask", "ls_long_edit_compact_mask", "ls_long_edit_mask_pairs")


def test_the_abi_only_grew():
    lib = _lib.load_library()
    assert lib.ls_abi_version() == 5
    hdr = open(os.path.join(ROOT, "include", "ls_hip.h")).read()
    for name in NEW_EXPORTS:
        assert name in _lib.EXPORTS and f"int {name}(" in hdr and hasattr(lib, name), name
    # no struct changed: the sizes the parent commit's tests pin
    assert ctypes.sizeof(_lib.LsLongEditArgs) == 144 and ctypes.sizeof(_lib.LsLongEditCompactArgs) == 152 and ctypes.sizeof(_lib.LsLongCond) == 64
    for name in ("long_edit_mask_pairs", "long_edit_mask_plan"):
        assert hasattr(_lib.Engine, name)
