"""Script-guided timeline edits on the GPU (long_form.edit_long(sag=, text_features=) -> ls_long_edit_sag; k_edit_start in
csrc/ls_chain.hip).

The contract: with noise_source='torch_cpu' the edited timeline and the raw windows are BIT FOR BIT what the hand-written loop over
``edit_plan`` gives -- ``edit_window`` -> ``sag(...)['output']`` -> ``edit_start`` -> the public ddim_sample_loop / p_sample_loop with
``init_image=`` that start (at skip_timesteps == 0 too) -> the editable elements written back.  No tolerance anywhere.  Shapes, ranges,
schedules, models and the starting timelines are those of tests/test_gpu_long_edit.py (B = 3, W = 3, 12 executed steps)."""
import functools

import numpy as np
import pytest
import torch

from livelyspeaker_amd import _lib, long_form, ref_draws, synth
from livelyspeaker_amd.motionclip_module import Decoder_TRANSFORMER
from test_gpu_long_edit import B, DEV, N, RANGES, S, SCHEDULES, T, W, _joints, _start

pytestmark = pytest.mark.gpu
CASES = [("ted", "ddim"), ("ted", "ddpm"), ("beat", "ddim"), ("beat", "ddpm"), ("ted", "ddim_noskip")]


@functools.lru_cache(maxsize=None)
def _script(ds):
    """The SAG decoder (synthetic weights) and the text features [B, W, 512] of one dataset; built once."""
    cfg = synth.CONFIGS[ds]
    sag = Decoder_TRANSFORMER(njoints=cfg.njoints, nfeats=cfg.nfeats, latent_dim=512, n_pre_poses=4, use_style=False)
    sag.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_sag_state_dict(cfg).items()}, strict=False)
    sag.to(DEV).eval()
    return sag, torch.from_numpy(synth.make_text_features(B * W).reshape(B, W, 512)).to(DEV)


def _edit(parts, ranges, joints=None, **kw):
    cfg, model, diffusion, sampler, skip, y, tl = parts
    return long_form.edit_long(diffusion, model, tl, ranges, y["audio"], y["seed_poses"], y["vid_indices"], y["scale"], emo=y.get("emo"),
                               joints=joints, sampler=sampler, skip_timesteps=skip, **kw)


def _by_host_loop(parts, sag, text, ranges, joints):
    """The definition through the public API: per window of edit_plan, edit_window -> decoder -> edit_start -> one sampling call ->
    write-back.  Returns the edited timeline, the raw windows, and per window (mask, the decoder differs from the slice where editable)."""
    cfg, model, diffusion, sampler, skip, y, timeline = parts
    tl = timeline.clone()
    shape = (B, cfg.njoints, cfg.nfeats, T)
    loop = diffusion.ddim_sample_loop if sampler == "ddim" else diffusion.p_sample_loop
    ones = torch.ones(B, T, device=tl.device).bool()
    seen, wins = [], []
    for w in long_form.edit_plan(ranges, W, cfg):
        origin_x, mask, motion = long_form.edit_window(tl, w, ranges, joints, y["seed_poses"], cfg)
        sag_out = sag({"x": origin_x.clone(), "z": text[:, w].contiguous(), "mask": ones})["output"]
        init = long_form.edit_start(motion, mask, sag_out)
        yy = {"audio_input": long_form.window_audio(y["audio"], w, cfg).contiguous(), "origin_x": origin_x, "vid_indices": y["vid_indices"],
              "scale": y["scale"], "inpainting_mask": mask, "inpainted_motion": motion}
        if "emo" in y:
            yy["emo"] = y["emo"][:, w:w + 1].expand(B, T).contiguous()
        s = loop(model, shape, clip_denoised=False, model_kwargs={"y": yy}, skip_timesteps=skip, init_image=init, progress=False,
                 dump_steps=None, noise=None, const_noise=False).contiguous()
        tl[..., w * S:w * S + T] = torch.where(mask, motion, s)
        seen.append((mask, not torch.equal(sag_out[~mask], motion[~mask]), torch.equal(init[1], motion[1])))
        wins.append(s)
    return tl, torch.stack(wins), seen


@functools.lru_cache(maxsize=None)
def _case(ds, schedule):
    """The scripted edit of RANGES on (ds, schedule), by the host loop and by edit_long (twice: the second call replays the loop)."""
    parts = _start(ds, schedule)
    sag, text = _script(ds)
    joints = _joints(parts[0])
    torch.manual_seed(23)
    want, want_w, seen = _by_host_loop(parts, sag, text, RANGES, joints)
    got = []
    for _ in range(2):
        torch.manual_seed(23)
        got.append(_edit(parts, RANGES, joints, sag=sag, text_features=text, return_windows=True))
    return parts, seen, want, want_w, got, parts[1].model.engine().timing()


@pytest.mark.parametrize("ds,schedule", CASES)
def test_scripted_edit_is_bitwise_the_public_loop(ds, schedule):
    parts, seen, want, want_w, got, t = _case(ds, schedule)
    timeline = parts[-1]
    assert (SCHEDULES[schedule][3] == 0) == (schedule == "ddim_noskip")          # the un-skipped case passes init_image at skip 0
    # the comparison exercises the branch
    assert len(seen) == 3
    assert any(bool(m.any()) and not bool(m.all()) for m, _, _ in seen)         # some window both keeps and edits
    assert all(differs for _, differs, _ in seen)                               # editable elements: the decoder's output is not the slice
    assert all(bool(m[1].all()) and slice_start for m, _, slice_start in seen)  # clip 1 keeps everything and starts from its slice
    for rep, (tl, ran, wins) in enumerate(got):
        assert ran == [0, 1, 2] and tl.shape == timeline.shape and tl.device == timeline.device and wins.shape == want_w.shape
        assert bool(torch.isfinite(tl).all())
        print(f"{ds} {schedule} rep {rep}: max |edit_long(sag) - host loop| = {float((tl - want).abs().max()):.3e}, "
              f"raw windows {float((wins - want_w).abs().max()):.3e}")
        assert torch.equal(wins, want_w), (rep, float((wins - want_w).abs().max()))
        assert torch.equal(tl, want), (rep, float((tl - want).abs().max()))
    assert t["n_segments"] == 3 and t["n_step_launches"] == 3 * 12
    if parts[2].use_graph:
        assert t["graph_replayed"] == 3                      # no window of the second call captured anything


@pytest.mark.parametrize("ds,schedule", CASES)
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
        assert not torch.equal(tl[0, :, :, 20:50], timeline[0, :, :, 20:50]) and not torch.equal(tl[2, 1, :, 70:80], timeline[2, 1, :, 70:80])


@pytest.mark.parametrize("ds", ["ted", "beat"])
def test_the_script_is_heard_and_only_where_it_should_be(ds):
    parts, _, _, _, got, _ = _case(ds, "ddim")
    sag, text = _script(ds)
    joints = _joints(parts[0])
    torch.manual_seed(23)
    plain = _edit(parts, RANGES, joints)
    scripted = got[0][0]
    assert not torch.equal(scripted[0, :, :, 20:50], plain[0, :, :, 20:50]) and not torch.equal(scripted[2, 1, :, 70:80], plain[2, 1, :, 70:80])
    assert torch.equal(scripted[1], plain[1])
    # a range that touches window 1 only: the text of windows 0 and 2 is not heard
    torch.manual_seed(7)
    one, ran = _edit(parts, (40, 45), sag=sag, text_features=text, return_windows=True)[:2]
    assert ran == [1]
    other = text.clone()
    other[:, 0] = -3.0 * text[:, 0] + 1.0
    other[:, 2] = 0.5 - text[:, 2]
    torch.manual_seed(7)
    assert torch.equal(_edit(parts, (40, 45), sag=sag, text_features=other), one)
    other[:, 1] = -text[:, 1]
    torch.manual_seed(7)
    assert not torch.equal(_edit(parts, (40, 45), sag=sag, text_features=other)[..., 40:45], one[..., 40:45])
    # one script for the whole stretch
    torch.manual_seed(7)
    rep = _edit(parts, RANGES, joints, sag=sag, text_features=text[:, 1:2].expand(B, W, 512).contiguous())
    torch.manual_seed(7)
    assert torch.equal(_edit(parts, RANGES, joints, sag=sag, text_features=text[:, 1].contiguous()), rep)


@pytest.mark.engine_path_auto
def test_contract_on_the_kernels_auto_picks_for_a_small_batch():
    """B = 3 under `auto` runs the sample-split kernel.  A model of its own: the cached ones hold engines pinned to the fused kernel."""
    parts = _start.__wrapped__("ted", "ddim")
    sag, text = _script("ted")
    joints = _joints(parts[0])
    torch.manual_seed(29)
    want, want_w, _ = _by_host_loop(parts, sag, text, RANGES, joints)
    for rep in range(2):
        torch.manual_seed(29)
        tl, ran, wins = _edit(parts, RANGES, joints, sag=sag, text_features=text, return_windows=True)
        assert ran == [0, 1, 2] and torch.equal(wins, want_w) and torch.equal(tl, want), (rep, float((tl - want).abs().max()))
    assert parts[1].model.engine().path == "auto"


@pytest.mark.parametrize("ds", ["ted", "beat"])
def test_philox_is_reproducible_and_a_windows_result_is_its_own(ds):
    parts = _start(ds, "ddim")
    sag, text = _script(ds)
    diffusion, timeline = parts[2], parts[-1]
    diffusion.noise_source, diffusion.philox_seed = "philox", 0x1234_5678_9ABC
    try:
        a, ran_a, win_a = _edit(parts, (40, 45), sag=sag, text_features=text, return_windows=True)
        b = _edit(parts, (40, 45), sag=sag, text_features=text)
        assert ran_a == [1] and torch.equal(a, b) and bool(torch.isfinite(a).all()) and not torch.equal(a[..., 40:45], timeline[..., 40:45])
        # clip 0 is edited alike in window 1 whether or not window 2 runs as well: its raw window 1 is the same
        both, ran, win_b = _edit(parts, np.array([(40, 45), (0, 0), (70, 80)]), sag=sag, text_features=text, return_windows=True)
        assert ran == [1, 2]
        assert torch.equal(win_b[0][0], win_a[0][0]) and torch.equal(both[0, :, :, 40:45], a[0, :, :, 40:45])
        assert not torch.equal(both[2, :, :, 70:80], timeline[2, :, :, 70:80]) and torch.equal(both[1], timeline[1])
    finally:
        diffusion.noise_source, diffusion.philox_seed = "torch_cpu", None


def test_engine_refusals_leave_the_handle_usable():
    parts, _, _, _, got, _ = _case("ted", "ddim")
    cfg, model, diffusion, sampler, skip, y, timeline = parts
    sag, text = _script("ted")
    eng = diffusion._bind_schedule(model.model.engine())
    model.model._cond_key = model.model._prefetched_key = None
    sag_eng = sag.engine()
    text_wb = text.permute(1, 0, 2).contiguous()
    sel = _joints(cfg)
    lo = RANGES[:, 0].astype(np.int32)
    hi = np.where(sel.any(axis=1), RANGES[:, 1], RANGES[:, 0]).astype(np.int32)
    shape = (B, cfg.njoints, cfg.nfeats, T)
    torch.manual_seed(23)
    x_init, eps, noise, inz = ref_draws.RefDraws("cpu").edit_windows(diffusion, 3, 12, shape, eng.D, True)
    kw = dict(sampler=_lib.LS_SAMPLER_DDIM, skip_timesteps=skip, inpaint_noised=True, channels=np.repeat(sel, cfg.nfeats, axis=1),
              x_init=x_init, eps_tape=eps, noise_tape=noise, inpaint_noise=inz, use_graph=diffusion.use_graph,
              two_pass_always=diffusion.two_pass_always, device_out=True, return_windows=True)
    args = (y["audio"].float(), y["seed_poses"].float(), y["vid_indices"], y["scale"].float())
    eng.long_prepare(*args, n_windows=W, audio_lengths=np.full(B, y["audio"].shape[1]))
    with pytest.raises(_lib.EngineError, match="ragged"):
        eng.long_edit(timeline, lo, hi, sag=sag_eng, text_features=text_wb, **kw)
    eng.long_prepare(*args, n_windows=W)
    with pytest.raises(_lib.EngineError, match="sag without text_features"):
        eng.long_edit(timeline, lo, hi, sag=sag_eng, **kw)
    with pytest.raises(_lib.EngineError, match="text_features without sag"):
        eng.long_edit(timeline, lo, hi, text_features=text_wb, **kw)
    tl, ran, wins = eng.long_edit(timeline, lo, hi, sag=sag_eng, text_features=text_wb, **kw)
    assert ran == [0, 1, 2]
    assert torch.equal(torch.as_tensor(tl), got[0][0]) and torch.equal(torch.as_tensor(wins), got[0][2])
