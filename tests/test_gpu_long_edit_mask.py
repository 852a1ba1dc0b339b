"""Timeline edits by ELEMENT MASK on the GPU (long_form.edit_long(mask=) -> ls_long_edit_mask / ls_long_prepare_edit_mask /
ls_long_edit_compact_mask; the mask forms of k_edit_gather / k_edit_start / k_edit_scatter, and k_edit_mask_pairs).

The contracts (every comparison is torch.equal, no tolerance anywhere):

1. A rectangle as a mask (``edit_mask``) gives the range call's timeline, plan and raw windows, dense and compact, both noise sources.
2. 'torch_cpu': an arbitrary mask is BIT FOR BIT the loop through the public API -- per planned window: ``edit_window(mask=)`` -> one
   ddim_sample_loop / p_sample_loop call -> the editable elements written back -- and everything not editable is the input's.
3. A scripted edit by mask is that loop with ``edit_start``.
4. k_edit_mask_pairs' flags are the host reduction's, byte for byte; a mask on the device gives what its host copy gives.
5. Ragged batches: nothing at or beyond a clip's length is read.
6. 'philox', compact: a clip's edited frames do not depend on the other clips' masks.
7. Constrained generation: pinned poses, everything else editable, skip_timesteps = 0.
8. Refusals come ahead of any window and leave the handle usable; an identical second call replays every window.

The test mask (tests/test_long_edit_mask_host.py: gpu_test_mask): clip 0 two stretches on other joints -- one across the seam of
windows 0 and 1, one to the last frame with a pinned frame inside --, clip 1 ONE element, clip 2 nothing, clip 3 frame 0 only.
B = 4, W = 3, 12 executed steps per window, the shapes, schedules and cached models of tests/test_gpu_long_edit_compact.py."""
import numpy as np
import pytest
import torch

from livelyspeaker_amd import _lib, long_form
from test_gpu_long_edit_compact import B, DEV, EQUAL, N, S, T, W, _edit, _joints, _lengths, _script, _silenced, _start
from test_long_edit_mask_host import GPU_TEST_PLAN, gpu_test_mask

pytestmark = pytest.mark.gpu
PINNED = 80                                                     # the frame gpu_test_mask pins inside clip 0's second stretch


def _edit_m(parts, mask, timeline=None, audio=None, **kw):
    cfg, model, diffusion, sampler, skip, y, tl, frames = parts
    return long_form.edit_long(diffusion, model, tl if timeline is None else timeline, None, y["audio"] if audio is None else audio,
                               y["seed_poses"], y["vid_indices"], y["scale"], emo=y.get("emo"), sampler=sampler, skip_timesteps=skip, mask=mask, **kw)


def _plan(parts, mask, compact):
    cfg, frames = parts[0], parts[7]
    if compact:
        return long_form.edit_plan_compact(None, W, cfg, frames=frames, mask=mask)
    return [(w, list(range(B))) for w in long_form.edit_plan(None, W, cfg, mask=mask)]      # the dense form: all clips in every window that runs


def _by_public_loop(parts, mask, compact, lens=None, sag=None, text=None, timeline=None):
    """The definition through the public API: one sampling call per planned window on its rows.  mask: numpy bool [B, J, F, N]."""
    cfg, model, diffusion, sampler, skip, y, tl0, frames = parts
    tl = (tl0 if timeline is None else timeline).clone()
    audio = y["audio"] if lens is None else _silenced(y["audio"], lens)
    loop = diffusion.ddim_sample_loop if sampler == "ddim" else diffusion.p_sample_loop
    plan = _plan(parts, mask, compact)
    wins = []
    for w, rows in plan:
        idx = torch.tensor(rows, device=tl.device)
        A = len(rows)
        origin_x, keep, motion = long_form.edit_window(tl[idx], w, None, None, y["seed_poses"][idx], cfg, mask=mask[rows])
        yy = {"audio_input": long_form.window_audio(audio[idx], w, cfg).contiguous(), "origin_x": origin_x,
              "vid_indices": y["vid_indices"][idx].contiguous(), "scale": y["scale"][idx].contiguous(), "inpainting_mask": keep,
              "inpainted_motion": motion}
        if "emo" in y:
            yy["emo"] = y["emo"][idx, w:w + 1].expand(A, T).contiguous()
        init = motion if skip > 0 else None
        if sag is not None:
            sag_out = sag({"x": origin_x.clone(), "z": text[idx, w].contiguous(), "mask": torch.ones(A, T, device=tl.device).bool()})["output"]
            init = long_form.edit_start(motion, keep, sag_out)
            assert torch.equal(init[keep], motion[keep])        # a kept element of the start plane is the slice's
        s = loop(model, (A, cfg.njoints, cfg.nfeats, T), clip_denoised=False, model_kwargs={"y": yy}, skip_timesteps=skip, init_image=init,
                 progress=False, dump_steps=None, noise=None, const_noise=False).contiguous()
        tl[idx, :, :, w * S:w * S + T] = torch.where(keep, motion, s)
        wins.append(s)
    return tl, plan, wins


def _check_against_the_loop(parts, mask, compact, seed=23, timeline=None, **kw):
    """Contract 2 on one case: the public loop, then edit_long twice (the second call replays every window)."""
    cfg, model, diffusion = parts[0], parts[1], parts[2]
    start = parts[6] if timeline is None else timeline
    torch.manual_seed(seed)
    want, plan, want_w = _by_public_loop(parts, mask, compact, kw.get("audio_lengths"), kw.get("sag"), kw.get("text_features"), timeline)
    before = start.clone()
    eng = model.model.engine()
    for rep in range(2):
        torch.manual_seed(seed)
        tl, ran, wins = _edit_m(parts, mask, timeline=timeline, return_windows=True, compact=compact, **kw)
        assert ran == (plan if compact else [w for w, _ in plan]) and tl.shape == start.shape and tl.device == start.device
        got_w = wins if compact else wins.reshape(-1, *wins.shape[2:])
        print(f"{cfg.name} compact={compact} rep {rep}: max |mask edit - public loop| = {float((tl - want).abs().max()):.3e}")
        assert torch.equal(got_w, torch.cat(want_w)), (rep, float((got_w - torch.cat(want_w)).abs().max()))
        assert torch.equal(tl, want), (rep, float((tl - want).abs().max()))
        t = eng.timing()
        assert t["n_segments"] == len(plan) and t["n_step_launches"] == len(plan) * 12
    if diffusion.use_graph:
        assert t["graph_replayed"] == len(plan)                 # no window of the second call captured anything
    assert torch.equal(start, before)                           # the caller's timeline is never written
    ed = torch.from_numpy(np.broadcast_to(mask, (B,) + mask.shape[1:]).copy()).to(tl.device)
    assert torch.equal(tl[~ed], start[~ed]) and not torch.equal(tl[ed], start[ed])      # every element that is not editable is the input's
    return tl, plan


@pytest.mark.parametrize("ds", ["ted", "beat"])
def test_a_rectangle_mask_is_bitwise_the_range_call(ds):
    parts = _start(ds, "ddim")
    cfg, diffusion = parts[0], parts[2]
    joints = _joints(cfg)
    mask = long_form.edit_mask(EQUAL, joints, N, cfg)
    for source in ("torch_cpu", "philox"):
        diffusion.noise_source, diffusion.philox_seed = source, (0x1234_5678_9ABC if source == "philox" else None)
        try:
            for compact in (False, True):
                torch.manual_seed(31)
                want, want_ran, want_w = _edit(parts, EQUAL, joints, return_windows=True, compact=compact)
                torch.manual_seed(31)
                tl, ran, wins = _edit_m(parts, mask, return_windows=True, compact=compact)
                assert ran == want_ran and torch.equal(wins, want_w) and torch.equal(tl, want), (source, compact)
                assert not torch.equal(tl, parts[6])
        finally:
            diffusion.noise_source, diffusion.philox_seed = "torch_cpu", None


@pytest.mark.parametrize("compact", [False, True])
@pytest.mark.parametrize("ds,schedule", [("ted", "ddim"), ("beat", "ddpm"), ("ted", "ddim_noskip")])
def test_an_arbitrary_mask_is_bitwise_the_public_loop(ds, schedule, compact):
    parts = _start(ds, schedule)
    cfg, timeline = parts[0], parts[6]
    mask = gpu_test_mask(cfg)
    tl, plan = _check_against_the_loop(parts, mask, compact)
    assert plan == (GPU_TEST_PLAN if compact else [(w, [0, 1, 2, 3]) for w in range(W)])
    J, F = cfg.njoints, cfg.nfeats
    assert torch.equal(tl[2], timeline[2])                                              # clip 2 entirely
    assert torch.equal(tl[0, :, :, PINNED], timeline[0, :, :, PINNED])                  # the pinned frame inside a stretch
    assert not torch.equal(tl[0, :J // 2, :, 30:34], timeline[0, :J // 2, :, 30:34])    # the seam frames: window 0's
    assert not torch.equal(tl[0, :J // 2, :, 34:38], timeline[0, :J // 2, :, 34:38])    # ... and window 1's
    assert torch.equal(tl[0, J // 2:, :, 26:38], timeline[0, J // 2:, :, 26:38])        # the other joints of that stretch
    assert not torch.equal(tl[0, J // 2:, :, 93], timeline[0, J // 2:, :, 93])          # the last frame
    assert tl[1, J - 1, F - 1, 45] != timeline[1, J - 1, F - 1, 45]                     # clip 1: one element, and nothing else of it
    assert int((tl[1] != timeline[1]).sum()) == 1
    assert not torch.equal(tl[3, :, :, 0], timeline[3, :, :, 0]) and torch.equal(tl[3, :, :, 1:], timeline[3, :, :, 1:])


@pytest.mark.parametrize("compact", [False, True])
def test_a_scripted_mask_edit_is_bitwise_the_loop_with_edit_start(compact):
    parts = _start("ted", "ddim")
    sag, text = _script("ted")
    _check_against_the_loop(parts, gpu_test_mask(parts[0]), compact, sag=sag, text_features=text)


def _host_flags(mask3, Wn, frames=None):
    flags = np.zeros((Wn, mask3.shape[0]), np.uint8)
    for w, rows in _lib.long_edit_plan_mask(mask3, Wn, frames):
        flags[w, rows] = 1
    return flags


def test_the_device_plan_is_the_host_plan_and_a_device_mask_edits_alike():
    parts = _start("ted", "ddim")
    cfg, model = parts[0], parts[1]
    eng = model.model.engine()
    JF = cfg.njoints * cfg.nfeats
    test = gpu_test_mask(cfg).reshape(B, JF, N)
    cases = [(test, W, None), (np.zeros_like(test), W, None), (np.ones_like(test), W, None)]
    rng = np.random.default_rng(11)
    for i in range(20):
        Bn, Wn = int(rng.integers(1, 7)), int(rng.integers(1, 6))
        Nn = T + (Wn - 1) * S
        frames = None
        if i % 2:
            frames = (T + S * rng.integers(0, Wn, Bn)).astype(np.int32)
            frames[int(rng.integers(0, Bn))] = Nn
        m = np.zeros((Bn, JF, Nn), bool)
        for _ in range(int(rng.integers(0, 6))):
            b = int(rng.integers(0, Bn))
            m[b, rng.integers(0, JF), rng.integers(0, Nn if frames is None else frames[b])] = True
        if i % 5 == 0:                                          # the seam: the prefix frames of a later window alone
            w = int(rng.integers(0, Wn))
            m[0, JF - 1, w * S:w * S + 4] = True
        cases.append((m, Wn, frames))
    for m, Wn, frames in cases:
        want = _host_flags(m, Wn, frames)
        for mask in (m, torch.from_numpy(m).to(DEV), torch.from_numpy(m.astype(np.uint8) * 255).to(DEV)):       # any non-zero byte is set
            got = eng.long_edit_mask_pairs(mask, Wn, frames)
            assert got.dtype == np.uint8 and got.shape == want.shape and np.array_equal(got, want), (Wn, frames)
    beyond = np.zeros((2, JF, N), bool)
    beyond[1, 3, 34] = True
    with pytest.raises(_lib.EngineError, match="frames"):
        eng.long_edit_mask_pairs(torch.from_numpy(beyond).to(DEV), W, np.array([94, 34], np.int32))
    assert np.array_equal(eng.long_edit_mask_pairs(torch.from_numpy(beyond).to(DEV), W, np.array([94, 64], np.int32)), [[0, 0], [0, 1], [0, 0]])
    # a device-resident mask: the result of its host copy, dense and compact
    mask = gpu_test_mask(cfg)
    for compact in (False, True):
        torch.manual_seed(5)
        host = _edit_m(parts, mask, return_windows=True, compact=compact)
        torch.manual_seed(5)
        dev = _edit_m(parts, torch.from_numpy(mask).to(DEV), return_windows=True, compact=compact)
        assert dev[1] == host[1] and torch.equal(dev[0], host[0]) and torch.equal(dev[2], host[2])
        assert not torch.equal(dev[0], parts[6])


@pytest.mark.parametrize("ds", ["ted", "beat"])
def test_a_ragged_batch_is_edited_by_mask_and_nothing_beyond_a_clips_length_is_read(ds):
    parts = _start(ds, "ddim", True, True)
    cfg, timeline, frames, y = parts[0], parts[6], parts[7], parts[5]
    assert frames.tolist() == [94, 34, 94, 64]
    lens = _lengths(cfg)
    J = cfg.njoints
    mask = np.zeros((B, J, cfg.nfeats, N), bool)
    mask[0, :, :, 40:50] = True
    mask[1, 1:J - 1, :, 5:34] = True                            # the clip of one window, to its last frame
    mask[3, :2, :, 60:64] = True                                # ... and clip 3 to its own last frame
    tl, plan = _check_against_the_loop(parts, mask, True, audio_lengths=lens)
    assert plan == [(0, [1]), (1, [0, 3])]
    for b, f in enumerate(frames):                              # frames beyond frames[b]: bit for bit as given
        assert torch.equal(tl[b, ..., int(f):], timeline[b, ..., int(f):])
    poisoned = y["audio"].clone()                               # NaN from each clip's own length on changes nothing
    for b, n in enumerate(lens):
        poisoned[b, n:] = float("nan")
    assert bool(torch.isnan(poisoned).any())
    torch.manual_seed(23)
    again = _edit_m(parts, mask, audio=poisoned, audio_lengths=lens)        # audio_lengths alone implies the compact form
    assert bool(torch.isfinite(again).all()) and torch.equal(again, tl)
    beyond = mask.copy()
    beyond[1, 0, 0, 34] = True
    for m in (beyond, torch.from_numpy(beyond).to(DEV)):
        with pytest.raises(ValueError, match="frames\\[b\\]"):
            _edit_m(parts, m, audio_lengths=lens)


def test_philox_a_clips_frames_do_not_depend_on_the_other_clips_masks():
    parts = _start("ted", "ddim")
    cfg, diffusion, timeline = parts[0], parts[2], parts[6]
    J = cfg.njoints
    mine = np.zeros((cfg.njoints, cfg.nfeats, N), bool)
    mine[1:J - 2, :, 40:45] = True
    mine[0, 0, 70] = True
    with_0, with_3 = np.zeros((B,) + mine.shape, bool), np.zeros((B,) + mine.shape, bool)
    with_0[2] = with_3[2] = mine
    with_0[0, :, :, 36:70] = True                               # clip 2 at row 1 of windows 1 and 2
    with_3[3, 2, 1, 5] = with_3[3, :, :, 60:94] = True          # clip 2 at row 0 of windows 1 and 2, and a window 0 that runs
    diffusion.noise_source, diffusion.philox_seed = "philox", 0x1234_5678_9ABC
    try:
        a, plan_a = _edit_m(parts, with_0, return_windows=True, compact=True)[:2]
        c, plan_c = _edit_m(parts, with_3, return_windows=True, compact=True)[:2]
        assert plan_a == [(1, [0, 2]), (2, [0, 2])] and plan_c == [(0, [3]), (1, [2, 3]), (2, [2, 3])]
        assert torch.equal(a[2], c[2]) and not torch.equal(a[2], timeline[2])
        assert torch.equal(a, _edit_m(parts, with_0, compact=True))
        assert torch.equal(a[3], timeline[3]) and torch.equal(c[0], timeline[0]) and torch.equal(a[1], timeline[1])
    finally:
        diffusion.noise_source, diffusion.philox_seed = "torch_cpu", None


@pytest.mark.parametrize("compact", [False, True])
def test_constrained_generation_passes_through_the_pinned_poses(compact):
    parts = _start("ted", "ddim_noskip")
    cfg, skip, timeline = parts[0], parts[4], parts[6]
    assert skip == 0
    pins = [10, 47, 93]
    poses = torch.zeros_like(timeline)
    poses[..., pins] = timeline[..., pins]                      # a timeline that holds only the pinned poses
    mask = long_form.keyframe_mask(N, pins, cfg)
    assert mask.shape == (1, cfg.njoints, cfg.nfeats, N)
    tl, plan = _check_against_the_loop(parts, np.broadcast_to(mask, (B,) + mask.shape[1:]).copy(), compact, timeline=poses)
    assert [w for w, _ in plan] == [0, 1, 2] and all(rows == [0, 1, 2, 3] for _, rows in plan)      # every window runs, for every clip
    assert torch.equal(tl[..., pins], timeline[..., pins])      # the pinned elements come back bit for bit
    free = [n for n in range(N) if n not in pins]
    assert bool((tl[..., free] != 0).all())                     # and everything else was generated
    torch.manual_seed(23)
    assert torch.equal(_edit_m(parts, mask, timeline=poses, compact=compact), tl)       # [1, J, F, N]: one mask for every clip


def test_engine_refusals_leave_the_handle_usable():
    parts = _start("ted", "ddim")
    cfg, model, diffusion, sampler, skip, y, timeline, _ = parts
    JF = cfg.njoints * cfg.nfeats
    mask = gpu_test_mask(cfg).reshape(B, JF, N)
    other = mask.copy()
    other[2, 0, 50] = True                                      # clip 2 joins window 1: other clip-windows than the prepared ones
    empty = np.zeros_like(mask)
    lo, hi = EQUAL[:, 0].astype(np.int32), EQUAL[:, 1].astype(np.int32)
    diffusion.noise_source, diffusion.philox_seed = "philox", 9
    try:
        eng = diffusion._bind_schedule(model.model.engine())
        model.model._cond_key = model.model._prefetched_key = None
        kw = dict(sampler=_lib.LS_SAMPLER_DDIM, skip_timesteps=skip, philox_seed=9, inpaint_noised=True, device_out=True)
        args = (y["audio"].float(), y["seed_poses"].float(), y["vid_indices"], y["scale"].float())

        def ordinary():                                         # an ordinary compact mask call, twice: the second replays every window
            for rep in range(2):
                tl, plan = eng.long_edit_compact(timeline, None, None, mask=mask, **kw)
                assert [(w, rows.tolist()) for w, rows in plan] == GPU_TEST_PLAN and bool(torch.isfinite(tl).all())
            t = eng.timing()
            assert t["n_segments"] == len(GPU_TEST_PLAN) and (not diffusion.use_graph or t["graph_replayed"] == len(GPU_TEST_PLAN))
            return tl

        for m in (empty, torch.from_numpy(empty).to(DEV)):      # an empty plan, from the host loop and from the kernel's flags
            with pytest.raises(_lib.EngineError, match="empty"):
                eng.long_prepare_edit(*args, None, None, n_windows=W, mask=m)
        eng.long_prepare_edit(*args, None, None, n_windows=W, mask=mask)
        assert [(w, rows.tolist()) for w, rows in eng.edit_plan] == GPU_TEST_PLAN
        first = ordinary()
        for m in (other, torch.from_numpy(other).to(DEV), empty):
            with pytest.raises(_lib.EngineError, match="differs"):
                eng.long_edit_compact(timeline, None, None, mask=m, **kw)
        assert torch.equal(ordinary(), first)
        with pytest.raises(_lib.EngineError, match="exclude each other"):
            eng.long_edit_compact(timeline, lo, hi, mask=mask, **kw)
        with pytest.raises(_lib.EngineError, match="exclude each other"):
            eng.long_edit_compact(timeline, None, None, channels=np.ones((B, JF), np.uint8), mask=mask, **kw)
        with pytest.raises(_lib.EngineError, match="ranges differ"):
            eng.long_edit_compact(timeline, lo, hi, **kw)       # the handle was prepared with a mask
        assert torch.equal(ordinary(), first)
        eng.long_prepare_edit(*args, lo, hi, n_windows=W)
        with pytest.raises(_lib.EngineError, match="prepared by ls_long_prepare_edit"):
            eng.long_edit_compact(timeline, None, None, mask=mask, **kw)       # ... and the other way round
        # the dense form
        eng.long_prepare(*args, n_windows=W)
        with pytest.raises(_lib.EngineError, match="empty"):
            eng.long_edit(timeline, None, None, mask=empty, **kw)
        with pytest.raises(_lib.EngineError, match="exclude each other"):
            eng.long_edit(timeline, lo, hi, mask=mask, **kw)
        for rep in range(2):
            tl, ran = eng.long_edit(timeline, None, None, mask=mask, **kw)
            assert ran == [0, 1, 2]
        assert not diffusion.use_graph or eng.timing()["graph_replayed"] == 3
        assert torch.equal(tl, _edit_m(parts, gpu_test_mask(cfg)))             # the engine's result is edit_long's with the same key
        assert torch.equal(first, _edit_m(parts, gpu_test_mask(cfg), compact=True))
    finally:
        diffusion.noise_source, diffusion.philox_seed = "torch_cpu", None
