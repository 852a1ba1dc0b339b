"""Timeline edits on the GPU (long_form.edit_long -> ls_long_prepare / ls_long_edit, k_edit_gather / k_edit_scatter in csrc/ls_chain.hip).

The contract: with noise_source='torch_cpu' the edited timeline is BIT FOR BIT what the hand-written loop over ``edit_plan`` gives --
``edit_window`` -> the public ddim_sample_loop / p_sample_loop with inpainting_mask / inpainted_motion / origin_x / the window's audio
in model_kwargs and init_image = the slice -> the editable elements written back -- and everything that is not editable is the input's,
bit for bit.  B = 3 (odd: per-clip indexing), W = 3 (94 frames; first, middle and last window), 12 executed steps per window (1000
steps respaced to 100, skip 88; the un-skipped case: a 12-step schedule), both datasets, synthetic weights."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from livelyspeaker_amd import _lib, long_form, synth
from livelyspeaker_amd.cfg_sampler import ClassifierFreeSampleModel
from livelyspeaker_amd.model_util import create_model_and_diffusion, load_model_wo_clip

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B, W, T, S = 3, 3, 34, 30
N = T + (W - 1) * S
SCHEDULES = {"ddim": (1000, "ddim100", "ddim", 88), "ddpm": (1000, "100", "ddpm", 88), "ddim_noskip": (12, "", "ddim", 0)}
RANGES = np.array([(20, 50), (0, 0), (70, 80)])             # clip 0 across the seam 33/34, clip 1 untouched, clip 2 inside own(2)


def _joints(cfg):
    sel = np.ones((B, cfg.njoints), bool)
    sel[2] = False
    sel[2, [1, cfg.njoints - 2]] = True                     # clip 2: two joints only
    return sel


@functools.lru_cache(maxsize=None)
def _start(ds, schedule):
    """Model, schedule, conditioning and the starting timeline (from sample_long) of one (dataset, schedule); built once."""
    steps, respacing, sampler, skip = SCHEDULES[schedule]
    cfg = synth.CONFIGS[ds]
    args = SimpleNamespace(mdm_condm="text", latent_dim=512, ff_size=1024, layers=8, cond_mask_prob=0.1, arch="trans_enc",
                           emb_trans_dec=False, dataset="humanml", lang_model=None, mlpact="silu", diffusion_steps=steps,
                           noise_schedule="cosine", sigma_small=True, lambda_vel=1.0, lambda_rcxyz=0.0, lambda_fc=0.0, njoints=cfg.njoints)
    model, diffusion = create_model_and_diffusion(args, respacing, dataset=ds)
    load_model_wo_clip(model, {k: torch.from_numpy(v) for k, v in synth.make_state_dict(cfg).items()})
    model = ClassifierFreeSampleModel(model).to(DEV)
    model.eval()
    assert diffusion.num_timesteps - skip == 12
    y = {k: torch.from_numpy(v).to(DEV) for k, v in synth.make_long_cond(cfg, B, W).items()}
    torch.manual_seed(41)
    timeline = long_form.sample_long(diffusion, model, y["audio"], y["seed_poses"], y["vid_indices"], y["scale"], emo=y.get("emo"),
                                     sampler=sampler, skip_timesteps=skip, n_windows=W)
    assert timeline.shape == (B, cfg.njoints, cfg.nfeats, N)
    return cfg, model, diffusion, sampler, skip, y, timeline


def _edit(parts, ranges, joints=None, timeline=None, **kw):
    cfg, model, diffusion, sampler, skip, y, tl = parts
    return long_form.edit_long(diffusion, model, tl if timeline is None else timeline, ranges, y["audio"], y["seed_poses"], y["vid_indices"],
                               y["scale"], emo=y.get("emo"), joints=joints, sampler=sampler, skip_timesteps=skip, **kw)


def _by_public_loop(parts, ranges, joints):
    """The definition through today's public API: one sampling call per window of edit_plan.  Returns the edited timeline, the masks
    and the raw samples of the windows that ran."""
    cfg, model, diffusion, sampler, skip, y, timeline = parts
    tl = timeline.clone()
    shape = (B, cfg.njoints, cfg.nfeats, T)
    loop = diffusion.ddim_sample_loop if sampler == "ddim" else diffusion.p_sample_loop
    masks, wins = [], []
    for w in long_form.edit_plan(ranges, W, cfg):
        origin_x, mask, motion = long_form.edit_window(tl, w, ranges, joints, y["seed_poses"], cfg)
        yy = {"audio_input": long_form.window_audio(y["audio"], w, cfg).contiguous(), "origin_x": origin_x, "vid_indices": y["vid_indices"],
              "scale": y["scale"], "inpainting_mask": mask, "inpainted_motion": motion}
        if "emo" in y:
            yy["emo"] = y["emo"][:, w:w + 1].expand(B, T).contiguous()
        s = loop(model, shape, clip_denoised=False, model_kwargs={"y": yy}, skip_timesteps=skip, init_image=motion if skip > 0 else None,
                 progress=False, dump_steps=None, noise=None, const_noise=False).contiguous()
        tl[..., w * S:w * S + T] = torch.where(mask, motion, s)
        masks.append(mask)
        wins.append(s)
    return tl, masks, torch.stack(wins)


@functools.lru_cache(maxsize=None)
def _case(ds, schedule):
    """The edit of RANGES on (ds, schedule), by the public loop and by edit_long (twice: the second call replays the captured loop)."""
    parts = _start(ds, schedule)
    joints = _joints(parts[0])
    torch.manual_seed(23)
    want, masks, want_w = _by_public_loop(parts, RANGES, joints)
    got = []
    for _ in range(2):
        torch.manual_seed(23)
        got.append(_edit(parts, RANGES, joints, return_windows=True))
    return parts, masks, want, want_w, got, parts[1].model.engine().timing()


def _check_bitwise(ds, schedule):
    parts, masks, want, want_w, got, t = _case(ds, schedule)
    timeline = parts[-1]
    # the comparison exercises the branch: a window that both keeps and edits, and a clip that keeps everything everywhere
    assert len(masks) == 3
    assert any(bool(m.any()) and not bool(m.all()) for m in masks)
    assert all(bool(m[1].all()) for m in masks)
    for rep, (tl, ran, wins) in enumerate(got):
        assert ran == [0, 1, 2] and tl.shape == timeline.shape and tl.device == timeline.device and wins.shape == want_w.shape
        assert bool(torch.isfinite(tl).all())
        print(f"{ds} {schedule} rep {rep}: max |edit_long - public loop| = {float((tl - want).abs().max()):.3e}, "
              f"raw windows {float((wins - want_w).abs().max()):.3e}")
        assert torch.equal(wins, want_w), (rep, float((wins - want_w).abs().max()))
        assert torch.equal(tl, want), (rep, float((tl - want).abs().max()))
    assert t["n_segments"] == 3 and t["n_step_launches"] == 3 * 12
    if parts[2].use_graph:
        assert t["graph_replayed"] == 3                      # no window of the second call captured anything


@pytest.mark.parametrize("schedule", ["ddim", "ddpm"])
@pytest.mark.parametrize("ds", ["ted", "beat"])
def test_edit_is_bitwise_the_public_loop(ds, schedule):
    _check_bitwise(ds, schedule)


@pytest.mark.engine_path_auto
def test_contract_on_the_kernels_auto_picks_for_a_small_batch():
    """B = 3 under `auto` runs the sample-split kernel, whose hand-off tags advance per window.  A model of its own: the cached ones
    hold engines pinned to the fused kernel."""
    parts = _start.__wrapped__("ted", "ddim")
    joints = _joints(parts[0])
    torch.manual_seed(29)
    want, _, want_w = _by_public_loop(parts, RANGES, joints)
    for rep in range(2):
        torch.manual_seed(29)
        tl, ran, wins = _edit(parts, RANGES, joints, return_windows=True)
        assert ran == [0, 1, 2] and torch.equal(wins, want_w) and torch.equal(tl, want), (rep, float((tl - want).abs().max()))
    assert parts[1].model.engine().path == "auto"


def test_edit_without_skip_starts_from_x_T_and_is_bitwise_the_public_loop():
    assert SCHEDULES["ddim_noskip"][3] == 0
    _check_bitwise("ted", "ddim_noskip")


@pytest.mark.parametrize("ds,schedule", [("ted", "ddim"), ("ted", "ddpm"), ("beat", "ddim"), ("beat", "ddpm"), ("ted", "ddim_noskip")])
def test_kept_means_kept(ds, schedule):
    parts, _, _, _, got, _ = _case(ds, schedule)
    cfg, timeline = parts[0], parts[-1]
    editable = torch.zeros(timeline.shape, dtype=torch.bool, device=timeline.device)
    joints = torch.from_numpy(_joints(cfg)).to(timeline.device)
    for b, (lo, hi) in enumerate(RANGES):
        editable[b, :, :, lo:hi] = joints[b][:, None, None]
    assert int(editable.sum()) == (30 * cfg.njoints + 10 * 2) * cfg.nfeats
    for tl, _, _ in got:
        assert torch.equal(tl[~editable], timeline[~editable])
        assert torch.equal(tl[1], timeline[1])
        assert not torch.equal(tl[editable], timeline[editable])
        assert not torch.equal(tl[0, :, :, 20:50], timeline[0, :, :, 20:50]) and not torch.equal(tl[2, 1, :, 70:80], timeline[2, 1, :, 70:80])


@pytest.mark.parametrize("ds", ["ted", "beat"])
def test_only_the_touched_windows_run(ds):
    parts = _start(ds, "ddim")
    cfg, model, timeline = parts[0], parts[1], parts[-1]
    before = timeline.clone()
    torch.manual_seed(5)
    tl, ran, wins = _edit(parts, (40, 45), return_windows=True)
    t = model.model.engine().timing()
    assert ran == [1] and wins.shape == (1, B, cfg.njoints, cfg.nfeats, T)
    assert t["n_segments"] == 1 and t["n_step_launches"] == 12
    keep = torch.ones(N, dtype=torch.bool, device=timeline.device)
    keep[40:45] = False
    assert torch.equal(tl[..., keep], timeline[..., keep]) and not torch.equal(tl[..., 40:45], timeline[..., 40:45])
    assert torch.equal(tl[..., 40:45], wins[0][..., 10:15])                     # the raw window holds what was written
    # frames 30..33 are window 0's alone: window 1 does not run
    torch.manual_seed(5)
    tl, ran, wins = _edit(parts, (30, 34), return_windows=True)
    assert ran == [0] and wins.shape[0] == 1 and model.model.engine().timing()["n_segments"] == 1
    assert torch.equal(tl[..., :30], timeline[..., :30]) and torch.equal(tl[..., 34:], timeline[..., 34:])
    assert not torch.equal(tl[..., 30:34], timeline[..., 30:34])
    # without return_windows the call returns the timeline alone, and host inputs give a host result with the same bits
    torch.manual_seed(5)
    again = _edit(parts, (30, 34))
    assert torch.is_tensor(again) and torch.equal(again, tl)
    host = tuple({k: v.cpu() for k, v in p.items()} if isinstance(p, dict) else p for p in parts[:-1]) + (timeline.cpu(),)
    torch.manual_seed(5)
    on_host = _edit(host, (30, 34))
    assert not on_host.is_cuda and torch.equal(on_host, tl.cpu())
    assert torch.equal(timeline, before)                                        # the caller's timeline is never written


@pytest.mark.parametrize("ds", ["ted", "beat"])
def test_philox_is_reproducible_and_a_windows_streams_are_its_own(ds):
    parts = _start(ds, "ddim")
    diffusion, timeline = parts[2], parts[-1]
    diffusion.noise_source, diffusion.philox_seed = "philox", 0x1234_5678_9ABC
    try:
        a = _edit(parts, (40, 45))
        b = _edit(parts, (40, 45))
        assert torch.equal(a, b) and bool(torch.isfinite(a).all()) and not torch.equal(a[..., 40:45], timeline[..., 40:45])
        # window 1 draws the same streams whether or not window 2 runs as well: (seed, clip, w) alone decide them
        both, ran = _edit(parts, np.array([(40, 45), (0, 0), (70, 80)]), return_windows=True)[:2]
        assert ran == [1, 2]
        assert torch.equal(both[0, :, :, 40:45], a[0, :, :, 40:45])
        assert not torch.equal(both[2, :, :, 70:80], timeline[2, :, :, 70:80]) and torch.equal(both[1], timeline[1])
        diffusion.philox_seed = 77
        assert not torch.equal(_edit(parts, (40, 45))[..., 40:45], a[..., 40:45])
    finally:
        diffusion.noise_source, diffusion.philox_seed = "torch_cpu", None


def test_engine_refusals_leave_the_handle_usable():
    parts = _start("ted", "ddim")
    cfg, model, diffusion, sampler, skip, y, timeline = parts
    eng = diffusion._bind_schedule(model.model.engine())
    model.model._cond_key = model.model._prefetched_key = None
    lo, hi = np.array([40, 40, 40], np.int32), np.array([45, 45, 45], np.int32)
    kw = dict(sampler=_lib.LS_SAMPLER_DDIM, skip_timesteps=skip, philox_seed=9, inpaint_noised=True)
    args = (y["audio"].float(), y["seed_poses"].float(), y["vid_indices"], y["scale"].float())
    eng.long_prepare(*args, n_windows=W, audio_lengths=np.full(B, y["audio"].shape[1]))
    with pytest.raises(_lib.EngineError, match="ragged"):
        eng.long_edit(timeline, lo, hi, **kw)
    eng.long_prepare(*args, n_windows=W)
    with pytest.raises(_lib.EngineError, match="empty"):
        eng.long_edit(timeline, lo, lo, **kw)
    with pytest.raises(_lib.EngineError, match="range"):
        eng.long_edit(timeline, lo, hi + N, **kw)
    with pytest.raises(_lib.EngineError, match="DDPM and DDIM"):
        eng.long_edit(timeline, lo, hi, **dict(kw, sampler=_lib.LS_SAMPLER_PLMS))
    tl, ran = eng.long_edit(timeline, lo, hi, **kw)
    assert ran == [1] and bool(torch.isfinite(tl).all())
    assert torch.equal(tl[..., :40], timeline[..., :40]) and torch.equal(tl[..., 45:], timeline[..., 45:])
    assert not torch.equal(tl[..., 40:45], timeline[..., 40:45])
    # the engine's result is edit_long's with the same key
    diffusion.noise_source, diffusion.philox_seed = "philox", 9
    try:
        assert torch.equal(_edit(parts, (40, 45)), tl)
    finally:
        diffusion.noise_source, diffusion.philox_seed = "torch_cpu", None
