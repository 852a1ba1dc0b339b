"""Host side of ``long_form.edit_long``: the windows an edit runs (edit_plan -> ls_long_edit_plan) against a brute-force enumeration
of the definition, ``edit_window`` on a hand-written timeline, the ABI of ``ls_long_edit_args`` and the refusals raised before an
engine exists.  No GPU."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

from livelyspeaker_amd import _lib, long_form, synth
from test_long_form_host import _no_engine, _parts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T, NPRE, S, W = 34, 4, 30, 4
N = T + (W - 1) * S


def _owned(w, f):
    return w == 0 or f >= NPRE


def _brute_plan(ranges, n_windows):
    """The definition, element by element: window w runs iff some clip has a frame f of it with lo <= w S + f < hi that w owns."""
    return [w for w in range(n_windows)
            if any(lo <= w * S + f < hi and _owned(w, f) for lo, hi in ranges for f in range(T))]


PLAN_CASES = {
    "inside own(1)": ([(40, 45)], [1]),
    "across the seam 33/34": ([(30, 40)], [0, 1]),
    "frames 30..33 belong to window 0 alone": ([(30, 34)], [0]),
    "exactly frame 34": ([(34, 35)], [1]),
    "the whole timeline": ([(0, N)], [0, 1, 2, 3]),
    "per-clip ranges whose union skips a window": ([(10, 20), (0, 0), (70, 80)], [0, 2]),
    "the last frame": ([(N - 1, N)], [3]),
    "an empty range beside a full one": ([(50, 50), (64, 94)], [2]),
}


@pytest.mark.parametrize("ds", ["ted", "beat"])
@pytest.mark.parametrize("case", sorted(PLAN_CASES))
def test_edit_plan_is_the_brute_force_enumeration(ds, case):
    cfg = synth.CONFIGS[ds]
    assert (cfg.nframes, cfg.n_pre_seq) == (T, NPRE)
    ranges, want = PLAN_CASES[case]
    assert _brute_plan(ranges, W) == want                      # the table above restates the definition
    assert long_form.edit_plan(np.array(ranges), W, cfg) == want
    lo, hi = np.array(ranges).T
    assert _lib.long_edit_plan(lo, hi, W, T, NPRE) == want
    if len(ranges) == 1:
        assert long_form.edit_plan(ranges[0], W, cfg) == want  # one pair for every clip


def test_edit_plan_agrees_with_brute_force_on_random_ranges():
    cfg = synth.TED
    rng = np.random.Generator(np.random.PCG64(19))
    for _ in range(200):
        B = int(rng.integers(1, 4))
        lo = rng.integers(0, N + 1, size=B)
        hi = np.minimum(N, lo + rng.integers(0, 12, size=B))
        ranges = [(int(a), int(b)) for a, b in zip(lo, hi)]
        want = _brute_plan(ranges, W)
        if want:
            assert long_form.edit_plan(np.array(ranges), W, cfg) == want, ranges
        else:
            with pytest.raises(ValueError):
                long_form.edit_plan(np.array(ranges), W, cfg)


@pytest.mark.parametrize("ds", ["ted", "beat"])
def test_edit_plan_refuses_empty_and_bad_ranges(ds):
    cfg = synth.CONFIGS[ds]
    with pytest.raises(ValueError, match="empty"):
        long_form.edit_plan(np.array([(5, 5), (0, 0), (N, N)]), W, cfg)
    for bad in ([(5, 4)], [(-1, 3)], [(0, N + 1)], [(0.0, 3.0)], [(1, 2, 3)]):
        with pytest.raises(ValueError):
            long_form.edit_plan(np.array(bad), W, cfg)
    with pytest.raises(ValueError):
        _lib.long_edit_plan([3], [2], W, T, NPRE)
    assert _lib.long_edit_plan([5, 0], [5, 0], W, T, NPRE) == []          # the C plan reports an empty set; refusing it is the callers'


@pytest.mark.parametrize("ds", ["ted", "beat"])
def test_edit_window_on_an_arange_timeline(ds):
    cfg = synth.CONFIGS[ds]
    B, J, F = 3, cfg.njoints, cfg.nfeats
    timeline = torch.arange(B * J * F * N, dtype=torch.float32).reshape(B, J, F, N)
    seed = -1.0 - torch.arange(B * J * F * NPRE, dtype=torch.float32).reshape(B, J, F, NPRE)
    ranges = np.array([(20, 50), (0, 0), (70, 80)])
    joints = np.ones((B, J), bool)
    joints[2] = False
    joints[2, [1, 3]] = True
    for w in range(W):
        origin_x, mask, motion = long_form.edit_window(timeline, w, ranges, joints, seed, cfg)
        assert origin_x.shape == mask.shape == motion.shape == (B, J, F, T) and mask.dtype == torch.bool and motion.is_contiguous()
        assert torch.equal(motion, timeline[..., w * S:w * S + T])
        assert torch.equal(origin_x[..., :NPRE], seed if w == 0 else timeline[..., w * S:w * S + NPRE])
        assert not origin_x[..., NPRE:].any()
        want = torch.ones(B, J, F, T, dtype=torch.bool)
        for b, (lo, hi) in enumerate(ranges):
            for j in range(J):
                for f in range(T):
                    if joints[b, j] and lo <= w * S + f < hi and _owned(w, f):
                        want[b, j, :, f] = False
        assert torch.equal(mask, want), w
        assert bool(mask[1].all())                             # the clip with the empty range keeps everything
        if w > 0:
            assert bool(mask[..., :NPRE].all())                # the hand-off frames belong to the window before
    # the windows of this edit, and what each may change
    assert long_form.edit_plan(ranges, W, cfg) == [0, 1, 2]
    m0 = long_form.edit_window(timeline, 0, ranges, joints, seed, cfg)[1]
    m1 = long_form.edit_window(timeline, 1, ranges, joints, seed, cfg)[1]
    assert not m0[0, :, :, 20:34].any() and bool(m0[0, :, :, :20].all())
    assert not m1[0, :, :, 4:20].any() and bool(m1[0, :, :, 20:].all())                  # frames 34..49 are window 1's frames 4..19
    m2 = long_form.edit_window(timeline, 2, ranges, None, seed, cfg)[1]                    # joints=None selects every joint
    assert not m2[2, :, :, 10:20].any()
    # one (lo, hi) pair and one joint row hold for every clip
    one = long_form.edit_window(timeline, 1, (40, 45), joints[2], seed, cfg)[1]
    assert all(not one[b, 1, :, 10:15].any() and bool(one[b, 0].all()) for b in range(B))
    with pytest.raises(ValueError):
        long_form.edit_window(timeline, W, ranges, joints, seed, cfg)
    with pytest.raises(ValueError):
        long_form.edit_window(timeline, 0, ranges, joints[:, :2], seed, cfg)


FIELDS = ("sampler", "noise_mode", "skip_timesteps", "on_device", "use_graph", "clip_denoised", "two_pass_always", "eta", "inpaint_noised",
          "windows_capacity", "frame_lo", "frame_hi", "channels", "timeline", "windows", "windows_run", "n_windows_run", "x_init",
          "eps_tape", "noise_tape", "inpaint_noise", "seed", "sample_offset")


def test_long_edit_args_match_the_header_and_the_abi_is_unchanged(tmp_path):
    lib = _lib.load_library()
    assert lib.ls_abi_version() == 5
    hdr = open(os.path.join(ROOT, "include", "ls_hip.h")).read()
    for name in ("ls_long_edit", "ls_long_edit_plan"):
        assert name in _lib.EXPORTS and f"int {name}(" in hdr and hasattr(lib, name), name
    assert [n for n, _ in _lib.LsLongEditArgs._fields_] == list(FIELDS)
    prints = "".join(f'    printf("%zu\\n", offsetof(ls_long_edit_args, {f}));\n' for f in FIELDS)
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "ls_hip.h"\nint main(void) {\n'
                   '    printf("%zu %zu %zu %d\\n", sizeof(ls_long_edit_args), sizeof(ls_long_cond), sizeof(ls_long_sample_args), LS_ABI_VERSION);\n'
                   + prints + '    return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got[:4] == [ctypes.sizeof(_lib.LsLongEditArgs), 64, 104, 5]
    assert got[4:] == [getattr(_lib.LsLongEditArgs, f).offset for f in FIELDS]
    assert ctypes.sizeof(_lib.LsLongCond) == 64 and ctypes.sizeof(_lib.LsLongSampleArgs) == 104
    assert hasattr(_lib.Engine, "long_edit")


@pytest.mark.parametrize("ds", ["ted", "beat"])
def test_edit_long_refusals_come_before_any_engine(ds, monkeypatch):
    _no_engine(monkeypatch)
    cfg, model, diffusion = _parts(ds)
    B, Wn = 2, 2
    y = synth.make_long_cond(cfg, B, Wn)
    emo = {"emo": y["emo"]} if ds == "beat" else {}
    timeline = np.zeros((B, cfg.njoints, cfg.nfeats, T + S), np.float32)

    def call(tl=timeline, frames=(10, 20), model=model, **kw):
        return long_form.edit_long(diffusion, model, tl, frames, y["audio"], y["seed_poses"], y["vid_indices"], y["scale"], **emo, **kw)

    with pytest.raises(TypeError):
        call(model=model.model)                                             # the bare RAG, not the CFG wrapper
    for frames in ((10, 20, 30), np.zeros((B + 1, 2), np.int64), np.zeros((B, 3), np.int64), (1.0, 2.0)):
        with pytest.raises(ValueError, match="frames"):
            call(frames=frames)
    with pytest.raises(ValueError):
        call(frames=(20, 10))                                               # lo > hi
    with pytest.raises(ValueError):
        call(frames=(0, T + S + 1))                                         # hi beyond the timeline
    with pytest.raises(ValueError):
        call(frames=np.array([(0, 5), (-1, 5)]))
    with pytest.raises(ValueError, match="joints"):
        call(joints=np.ones(cfg.njoints + 1, bool))
    with pytest.raises(ValueError, match="joints"):
        call(joints=np.ones((B + 1, cfg.njoints), bool))
    for n in (T + S - 1, T + S + 1, T - 1):                                 # not 34 + 30 (W - 1) frames
        with pytest.raises(ValueError, match="frames"):
            call(tl=np.zeros((B, cfg.njoints, cfg.nfeats, n), np.float32))
    with pytest.raises(ValueError):
        call(tl=timeline[:, :-1])                                           # another joint count
    with pytest.raises(ValueError, match="empty"):
        call(frames=(7, 7))                                                 # nothing to edit
    with pytest.raises(ValueError, match="empty"):
        call(joints=np.zeros(cfg.njoints, bool))                            # no joint selected: no clip is edited
    with pytest.raises(ValueError):
        call(sampler="plms")
    with pytest.raises(ValueError):
        call(skip_timesteps=diffusion.num_timesteps)
    diffusion.noise_source = "torch_device"
    with pytest.raises(NotImplementedError):
        call()
    diffusion.noise_source = "torch_cpu"
    # sample_long keeps refusing the inpainting keys
    with pytest.raises(NotImplementedError):
        long_form.sample_long(diffusion, model, y["audio"], y["seed_poses"], y["vid_indices"], y["scale"], **emo, inpainting_mask=np.ones(1))
