"""Host side of the COMPACT ``long_form.edit_long``: the clip-windows it runs (``edit_plan_compact`` -> ls_long_edit_plan_compact)
against a restatement written here over random ranges, joints and frames; the property that ties it to ``edit_plan``; the counts-first
calling convention and every ``LS_EINVAL`` through ctypes; tests/edit_plan_main.cpp -- a stand-alone program around the plan's unit --
under the host sanitizers; the ABI, which only grew; the packed draws of ``RefDraws.edit_windows(batches=)``; and the refusals
``edit_long`` raises before an engine exists.  No GPU."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

from livelyspeaker_amd import _lib, build, long_form, ref_draws, synth
from test_long_form_host import _no_engine, _parts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T, NPRE, S = 34, 4, 30
I32 = ctypes.POINTER(ctypes.c_int32)


def _restated(lo, hi, W, sel=None, frames=None):
    """The definition in numpy: pair (b, w) iff some frame f of w has lo_b <= w S + f < hi_b on a frame w owns, a joint of b is selected,
    and w < W_b; window w runs iff it has a pair, with its clips ascending."""
    B = len(lo)
    f = np.arange(T)
    plan = []
    for w in range(W):
        t, own = w * S + f, (f >= NPRE) | (w == 0)
        rows = [b for b in range(B) if (own & (t >= lo[b]) & (t < hi[b])).any() and (sel is None or sel[b].any())
                and (frames is None or w < (frames[b] - T) // S + 1)]
        if rows:
            plan.append((w, rows))
    return plan


def _c_plan(lo, hi, W, chan=None, frames=None, caps=None):
    """ls_long_edit_plan_compact through ctypes, the two-call use: (rc, plan, n_run, n_pairs)."""
    lib = _lib.load_library()
    lo, hi = np.ascontiguousarray(lo, np.int32), np.ascontiguousarray(hi, np.int32)
    p = lambda a: None if a is None else a.ctypes.data_as(I32)      # noqa: E731
    fr = None if frames is None else np.ascontiguousarray(frames, np.int32)
    ch = None if chan is None else np.ascontiguousarray(chan, np.uint8)
    chp, nch = (None, 0) if ch is None else (ch.ctypes.data_as(ctypes.c_void_p), ch.shape[1])
    nw, npairs = ctypes.c_int32(-7), ctypes.c_int32(-7)
    head = (len(lo), W, T, NPRE, p(lo), p(hi), chp, nch, p(fr))
    rc = lib.ls_long_edit_plan_compact(*head, None, None, 0, None, 0, ctypes.byref(nw), ctypes.byref(npairs))
    if rc != 0:
        return rc, None, None, None
    n_run, n_pairs = nw.value, npairs.value
    wins, counts, rows = np.full(n_run + 1, -9, np.int32), np.full(n_run + 1, -9, np.int32), np.full(n_pairs + 1, -9, np.int32)
    cw, cr = caps if caps is not None else (n_run, n_pairs)
    rc = lib.ls_long_edit_plan_compact(*head, p(wins), p(counts), cw, p(rows), cr, ctypes.byref(nw), ctypes.byref(npairs))
    if rc != 0:
        return rc, None, n_run, n_pairs
    assert (nw.value, npairs.value) == (n_run, n_pairs) and wins[-1] == counts[-1] == rows[-1] == -9      # nothing behind the plan is written
    offs = np.concatenate([[0], np.cumsum(counts[:n_run])])
    return 0, [(int(wins[e]), rows[offs[e]:offs[e + 1]].tolist()) for e in range(n_run)], n_run, n_pairs


def test_the_plans_of_the_gpu_tests():
    cfg = synth.TED
    equal = np.array([(20, 50), (0, 0), (70, 80), (40, 72)])
    assert long_form.edit_plan_compact(equal, 3, cfg) == [(0, [0]), (1, [0, 3]), (2, [2, 3])]
    ragged = np.array([(20, 50), (5, 30), (70, 80), (40, 64)])
    lens = [cfg.audio_len + 64000, 20000, cfg.audio_len + 64000, 60000]
    plans = long_form.plan_lengths(lens, cfg)
    assert [W for W, _ in plans] == [3, 1, 3, 2] and [f for _, f in plans] == [94, 34, 94, 64]
    assert long_form.edit_plan_compact(ragged, 3, cfg, frames=[f for _, f in plans]) == [(0, [0, 1]), (1, [0, 3]), (2, [2])]
    # the same ranges on an equal-length batch: clip 1's range reaches no further, clip 3 is still out of window 2 (64 is own(2)'s first frame)
    assert long_form.edit_plan_compact(ragged, 3, cfg) == [(0, [0, 1]), (1, [0, 3]), (2, [2])]
    # where the lengths cut: a range that crosses into a window the clip does not have is refused, not clipped
    with pytest.raises(ValueError):
        long_form.edit_plan_compact(np.array([(20, 50), (5, 40), (70, 80), (40, 64)]), 3, cfg, frames=[94, 34, 94, 64])
    # one pair holds for every clip of `frames`; an empty plan is an empty list
    assert long_form.edit_plan_compact((10, 20), 3, cfg, frames=[94, 34]) == [(0, [0, 1])]
    assert long_form.edit_plan_compact(np.array([(5, 5), (94, 94)]), 3, cfg) == []
    # a joint selection: a clip without a selected joint is in no window
    sel = np.ones((4, cfg.njoints), bool)
    sel[0] = False
    assert long_form.edit_plan_compact(equal, 3, cfg, joints=sel) == [(1, [3]), (2, [2, 3])]


@pytest.mark.parametrize("ds", ["ted", "beat"])
def test_plan_agrees_with_the_restatement_on_random_cases(ds):
    cfg = synth.CONFIGS[ds]
    rng = np.random.default_rng(20261021)
    seen_empty = seen_skip = 0
    for _ in range(300):
        B, W = int(rng.integers(1, 7)), int(rng.integers(1, 6))
        N = T + (W - 1) * S
        frames = None
        if rng.random() < 0.5:
            frames = T + S * rng.integers(0, W, B)
            frames[int(rng.integers(0, B))] = N
        most = np.full(B, N) if frames is None else frames
        lo = rng.integers(0, most + 1)
        hi = np.minimum(most, lo + rng.integers(0, 50, B))
        sel = None
        if rng.random() < 0.5:
            sel = rng.random((B, cfg.njoints)) < 0.3
            sel[rng.random(B) < 0.3] = False
        want = _restated(lo, hi, W, sel, frames)
        got = long_form.edit_plan_compact(np.stack([lo, hi], 1), W, cfg, joints=sel, frames=frames)
        assert got == want, (lo, hi, W, frames)
        chan = None if sel is None else np.repeat(sel, cfg.nfeats, axis=1)
        rc, c_plan, n_run, n_pairs = _c_plan(lo, hi, W, chan, frames)
        assert rc == 0 and c_plan == want and n_run == len(want) and n_pairs == sum(len(r) for _, r in want)
        for w, rows in got:
            assert rows == sorted(set(rows)) and 0 <= rows[0] and rows[-1] < B            # ascending, distinct clips
        assert [w for w, _ in got] == sorted(w for w, _ in got)
        # the property: without frames, the windows that run are ls_long_edit_plan's for the same ranges
        if frames is None:
            folded = hi if sel is None else np.where(sel.any(axis=1), hi, lo)
            assert [w for w, _ in got] == _lib.long_edit_plan(lo, folded, W, T, NPRE)
        seen_empty += not got
        seen_skip += bool(got) and len(got) < got[-1][0] - got[0][0] + 1
    assert seen_empty and seen_skip                                                     # the draw reaches both kinds


def test_every_einval_and_the_counts_first_convention():
    ok = _c_plan([0, 40], [40, 60], 2)
    assert ok == (0, [(0, [0]), (1, [0, 1])], 2, 3)
    assert _c_plan([5], [4], 3)[0] == -1                                               # lo > hi
    assert _c_plan([-1], [4], 3)[0] == -1
    assert _c_plan([0], [95], 3)[0] == -1 and _c_plan([0], [94], 3)[0] == 0            # T + (W - 1) S = 94
    assert _c_plan([0], [65], 3, frames=[64])[0] == -1 and _c_plan([0], [64], 3, frames=[64])[0] == 0
    for bad in (65, 63, 33, 4, 0, -30, 124):                                           # not 34 + 30 k with k < W
        assert _c_plan([0], [0], 3, frames=[bad])[0] == -1, bad
    assert _c_plan([0, 40], [40, 60], 2, caps=(1, 3))[0] == -1                         # room for one window of two
    assert _c_plan([0, 40], [40, 60], 2, caps=(2, 2))[0] == -1                         # room for two rows of three
    assert _c_plan([0, 40], [40, 60], 2, caps=(-1, 3))[0] == -1
    assert _c_plan([5, 94], [5, 94], 3) == (0, [], 0, 0)                               # no pair: not an error of the plan
    with pytest.raises(ValueError):
        _lib.long_edit_plan_compact([3], [2], 3)
    with pytest.raises(ValueError):
        _lib.long_edit_plan_compact([0, 0], [4, 4], 3, frames=[94])                    # one entry per clip
    with pytest.raises(ValueError):
        long_form.edit_plan_compact((0, 10), 3, synth.TED, frames=[65])


def test_edit_plan_main_on_its_edges_under_asan_and_ubsan(tmp_path):
    """tests/edit_plan_main.cpp with the plan's unit, as plain C++ with the host sanitizers linked statically: a child process of its
    own, nothing preloaded, nothing inside Python, no GPU."""
    exe = str(tmp_path / "edit_plan")
    made = subprocess.run([build.hipcc_path(), "-x", "c++", "-std=c++17", "-O1", "-g", "-fno-gpu-sanitize", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "edit_plan_main.cpp"),
                           os.path.join(ROOT, "livelyspeaker_amd", "csrc", "ls_chain_plan.cpp"), "-o", exe], capture_output=True, text=True)
    assert made.returncode == 0, made.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr
    assert run.stderr == "", run.stderr


FIELDS = ("sampler", "noise_mode", "skip_timesteps", "on_device", "use_graph", "clip_denoised", "two_pass_always", "eta", "inpaint_noised",
          "windows_capacity", "frame_lo", "frame_hi", "channels", "timeline", "windows", "windows_run", "n_windows_run", "x_init",
          "eps_tape", "noise_tape", "inpaint_noise", "seed", "sample_offset", "rows_run")
NEW_EXPORTS = ("ls_long_edit_plan_compact", "ls_long_prepare_edit", "ls_long_edit_compact")


def test_the_new_struct_matches_the_header_and_the_abi_only_grew(tmp_path):
    lib = _lib.load_library()
    assert lib.ls_abi_version() == 5
    hdr = open(os.path.join(ROOT, "include", "ls_hip.h")).read()
    for name in NEW_EXPORTS:
        assert name in _lib.EXPORTS and f"int {name}(" in hdr and hasattr(lib, name), name
    for name in ("long_prepare_edit", "long_edit_compact"):
        assert hasattr(_lib.Engine, name)
    assert [n for n, _ in _lib.LsLongEditCompactArgs._fields_] == list(FIELDS)
    prints = "".join(f'    printf("%zu\\n", offsetof(ls_long_edit_compact_args, {f}));\n' for f in FIELDS)
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "ls_hip.h"\nint main(void) {\n'
                   '    printf("%zu %zu %zu %zu %d\\n", sizeof(ls_long_edit_compact_args), sizeof(ls_long_edit_args), sizeof(ls_long_cond),\n'
                   '           sizeof(ls_long_sample_args), LS_ABI_VERSION);\n' + prints + '    return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got[:5] == [ctypes.sizeof(_lib.LsLongEditCompactArgs), ctypes.sizeof(_lib.LsLongEditArgs), 64, 104, 5]
    assert got[5:] == [getattr(_lib.LsLongEditCompactArgs, f).offset for f in FIELDS]
    # the old structs' sizes, as the parent commit's tests pin them
    assert ctypes.sizeof(_lib.LsLongEditArgs) == 144 and ctypes.sizeof(_lib.LsLongCond) == 64 and ctypes.sizeof(_lib.LsLongSampleArgs) == 104
    assert ctypes.sizeof(_lib.LsLongEditCompactArgs) == 152


def test_packed_draws_are_one_call_per_window_at_its_batch():
    """RefDraws.edit_windows(batches=): what one public sampling call per window at batch A_w draws, one after the other."""
    cfg, model, diffusion = _parts("ted")
    J, F, D, n_exec, batches = cfg.njoints, cfg.nfeats, 8, 3, [1, 2, 2]
    for noised in (True, False):
        torch.manual_seed(3)
        x, eps, nz, inz = ref_draws.RefDraws("cpu").edit_windows(diffusion, 3, n_exec, (2, J, F, T), D, noised, batches=batches)
        assert x.shape == (5, J, F, T) and eps.shape == (5 * n_exec * 2 * D,) and nz.shape == (5 * n_exec * J * F * T,)
        assert (inz is None) == (not noised)
        torch.manual_seed(3)
        first = 0
        for A in batches:           # the dense form at batch A, window by window, continues the same generator
            x1, e1, n1, i1 = ref_draws.RefDraws("cpu").edit_windows(diffusion, 1, n_exec, (A, J, F, T), D, noised)
            per = n_exec * J * F * T
            assert torch.equal(x[first:first + A], x1[0])
            assert torch.equal(eps[first * n_exec * 2 * D:(first + A) * n_exec * 2 * D].view(n_exec, 2, A, D), e1[0])
            assert torch.equal(nz[first * per:(first + A) * per].view(n_exec, A, J, F, T), n1[0])
            if noised:
                assert torch.equal(inz[first * per:(first + A) * per].view(n_exec, A, J, F, T), i1[0])
            first += A
    with pytest.raises(ValueError):
        ref_draws.RefDraws("cpu").edit_windows(diffusion, 2, n_exec, (2, J, F, T), D, True, batches=[1, 2, 2])


@pytest.mark.parametrize("ds", ["ted", "beat"])
def test_compact_refusals_come_before_any_engine(ds, monkeypatch):
    _no_engine(monkeypatch)
    cfg, model, diffusion = _parts(ds)
    B, Wn = 2, 2
    y = synth.make_long_cond(cfg, B, Wn)
    emo = {"emo": y["emo"]} if ds == "beat" else {}
    timeline = np.zeros((B, cfg.njoints, cfg.nfeats, T + S), np.float32)
    L = y["audio"].shape[1]
    lens = [L, 20000]                                                       # W_b = (2, 1): frames (64, 34)

    def call(frames=(10, 20), **kw):
        return long_form.edit_long(diffusion, model, timeline, frames, y["audio"], y["seed_poses"], y["vid_indices"], y["scale"], **emo, **kw)

    with pytest.raises(ValueError, match="compact=False"):
        call(audio_lengths=lens, compact=False)
    with pytest.raises(ValueError, match="frames\\[b\\]"):
        call(frames=np.array([(10, 20), (10, 35)]), audio_lengths=lens)     # clip 1 holds 34 frames
    with pytest.raises(ValueError, match="frames\\[b\\]"):
        call(frames=(30, 40), audio_lengths=lens)                           # one pair for all clips: beyond clip 1 as well
    with pytest.raises(ValueError, match="audio_lengths"):
        call(audio_lengths=[L])                                             # one length per clip
    with pytest.raises(ValueError, match="audio_lengths"):
        call(audio_lengths=[L + 1, 5])                                      # beyond the waveform
    with pytest.raises(ValueError, match="windows"):
        call(audio_lengths=[20000, 20000])                                  # the timeline holds more windows than the lengths need
    with pytest.raises(ValueError, match="empty"):
        call(frames=(7, 7), compact=True)
    with pytest.raises(ValueError, match="empty"):
        call(joints=np.zeros(cfg.njoints, bool), audio_lengths=lens)
    with pytest.raises(ValueError):
        call(sampler="plms", compact=True)
    diffusion.noise_source = "torch_device"
    try:
        with pytest.raises(NotImplementedError):
            call(compact=True)
        with pytest.raises(NotImplementedError):
            call(audio_lengths=lens)
    finally:
        diffusion.noise_source = "torch_cpu"
