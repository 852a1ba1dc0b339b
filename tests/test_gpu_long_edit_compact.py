"""The COMPACT timeline edit on the GPU (long_form.edit_long(compact=True / audio_lengths=) -> ls_long_prepare_edit / ls_long_edit_compact;
the row-table forms of k_edit_gather / k_edit_start / k_edit_scatter, k_cond_gather, the keyed re-noise stream of ls_philox_rows.hip).

The contracts (every comparison is torch.equal, no tolerance anywhere):

1. 'torch_cpu': the edit is BIT FOR BIT the loop over ``edit_plan_compact`` through the public API -- per (w, rows): ``edit_window`` on
   ``timeline[rows]`` -> one ddim_sample_loop / p_sample_loop call at batch len(rows) with those clips' conditioning -> the editable
   elements written back -- and everything not editable is the input's, whole clips outside the plan and frames beyond a ragged
   clip's own included.
2. Where every clip is in every running window, the compact call is the dense call, under 'torch_cpu' and under 'philox'.
3. 'philox': reproducible, and a clip's frames do not depend on the clips beside it nor on its row.
4. Audio at and beyond a clip's length is never read.
5. Only the plan runs: n_segments, n_step_launches, rows_run; the second identical call replays every window.

B = 4, W = 3 (94 frames: first, middle and last window), 12 executed steps per window with the schedules of tests/test_gpu_long_edit.py,
both datasets, synthetic weights."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from livelyspeaker_amd import _lib, long_form, synth
from livelyspeaker_amd.cfg_sampler import ClassifierFreeSampleModel
from livelyspeaker_amd.model_util import create_model_and_diffusion, load_model_wo_clip
from livelyspeaker_amd.motionclip_module import Decoder_TRANSFORMER
from test_gpu_long_edit import SCHEDULES

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B, W, T, S = 4, 3, 34, 30
N = T + (W - 1) * S
EQUAL = np.array([(20, 50), (0, 0), (70, 80), (40, 72)])        # A_0 = {0}, A_1 = {0, 3}, A_2 = {2, 3}: row != clip in two windows
EQUAL_PLAN = [(0, [0]), (1, [0, 3]), (2, [2, 3])]
RAGGED = np.array([(20, 50), (5, 30), (70, 80), (40, 64)])      # with W_b = (3, 1, 3, 2): A_0 = {0, 1}, A_1 = {0, 3}, A_2 = {2}
RAGGED_PLAN = [(0, [0, 1]), (1, [0, 3]), (2, [2])]
WHOLE = np.array([(10, 90)] * B)                                # every clip in every window: the identity tables


def _joints(cfg):
    sel = np.ones((B, cfg.njoints), bool)
    sel[2] = False
    sel[2, [1, cfg.njoints - 2]] = True                         # clip 2: two joints only
    return sel


def _lengths(cfg):
    a = cfg.audio_len
    return [a + 64000, 20000, a + 64000, 60000]


@functools.lru_cache(maxsize=None)
def _model(ds, schedule):
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
    return cfg, model, diffusion, sampler, skip


def _start_of(ds, schedule, ragged=None, mixed_scales=False, fresh=False):
    """Model, schedule, conditioning and the starting timeline of one case.  ragged: None (equal lengths), or the drop_finished flag of
    the sample_long call that makes the timeline; mixed_scales: clips 0, 2, 3 at guidance scale 1, so that the windows of the ragged
    plan decide differently (A_0 = {0, 1} runs both passes, A_1 and A_2 the single-pass form); fresh: a model of its own."""
    cfg, model, diffusion, sampler, skip = (_model.__wrapped__ if fresh else _model)(ds, schedule)
    y = {k: torch.from_numpy(v).to(DEV) for k, v in synth.make_long_cond(cfg, B, W).items()}
    if mixed_scales:
        y["scale"] = torch.tensor([1.0, 1.5, 1.0, 1.0], device=DEV)
    kw = dict(emo=y.get("emo"), sampler=sampler, skip_timesteps=skip)
    torch.manual_seed(41)
    if ragged is None:
        timeline = long_form.sample_long(diffusion, model, y["audio"], y["seed_poses"], y["vid_indices"], y["scale"], n_windows=W, **kw)
        frames = None
    else:
        timeline, frames = long_form.sample_long(diffusion, model, y["audio"], y["seed_poses"], y["vid_indices"], y["scale"],
                                                 audio_lengths=_lengths(cfg), drop_finished=ragged, **kw)
        assert frames.tolist() == [94, 34, 94, 64]
        timeline = timeline.clone()
        for b, f in enumerate(frames):                          # what lies beyond a clip's own frames must come back as given: make it visible
            timeline[b, ..., int(f):] = 3.25 + b
    assert timeline.shape == (B, cfg.njoints, cfg.nfeats, N)
    return cfg, model, diffusion, sampler, skip, y, timeline, frames


_start = functools.lru_cache(maxsize=None)(_start_of)


@functools.lru_cache(maxsize=None)
def _script(ds):
    cfg = synth.CONFIGS[ds]
    sag = Decoder_TRANSFORMER(njoints=cfg.njoints, nfeats=cfg.nfeats, latent_dim=512, n_pre_poses=4, use_style=False)
    sag.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_sag_state_dict(cfg).items()}, strict=False)
    sag.to(DEV).eval()
    return sag, torch.from_numpy(synth.make_text_features(B * W).reshape(B, W, 512)).to(DEV)


def _silenced(audio, lens):
    valid = torch.arange(audio.shape[1], device=audio.device)[None, :] < torch.as_tensor(np.asarray(lens), device=audio.device)[:, None]
    return torch.where(valid, audio, torch.zeros((), device=audio.device))


def _edit(parts, ranges, joints=None, timeline=None, audio=None, **kw):
    cfg, model, diffusion, sampler, skip, y, tl, frames = parts
    return long_form.edit_long(diffusion, model, tl if timeline is None else timeline, ranges, y["audio"] if audio is None else audio,
                               y["seed_poses"], y["vid_indices"], y["scale"], emo=y.get("emo"), joints=joints, sampler=sampler,
                               skip_timesteps=skip, **kw)


def _by_public_loop(parts, ranges, joints, lens=None, sag=None, text=None):
    """The definition through the public API: one sampling call per (w, rows) of edit_plan_compact, on the rows alone.  Returns the
    edited timeline, the plan, the packed raw samples and the masks."""
    cfg, model, diffusion, sampler, skip, y, timeline, frames = parts
    tl = timeline.clone()
    audio = y["audio"] if lens is None else _silenced(y["audio"], lens)
    loop = diffusion.ddim_sample_loop if sampler == "ddim" else diffusion.p_sample_loop
    plan = long_form.edit_plan_compact(ranges, W, cfg, joints=joints, frames=frames)
    masks, wins = [], []
    for w, rows in plan:
        idx = torch.tensor(rows, device=tl.device)
        A = len(rows)
        origin_x, mask, motion = long_form.edit_window(tl[idx], w, ranges[rows], None if joints is None else joints[rows], y["seed_poses"][idx], cfg)
        yy = {"audio_input": long_form.window_audio(audio[idx], w, cfg).contiguous(), "origin_x": origin_x,
              "vid_indices": y["vid_indices"][idx].contiguous(), "scale": y["scale"][idx].contiguous(), "inpainting_mask": mask,
              "inpainted_motion": motion}
        if "emo" in y:
            yy["emo"] = y["emo"][idx, w:w + 1].expand(A, T).contiguous()
        init = motion if skip > 0 else None
        if sag is not None:
            sag_out = sag({"x": origin_x.clone(), "z": text[idx, w].contiguous(), "mask": torch.ones(A, T, device=tl.device).bool()})["output"]
            assert bool(torch.isfinite(sag_out).all())
            init = long_form.edit_start(motion, mask, sag_out)
        s = loop(model, (A, cfg.njoints, cfg.nfeats, T), clip_denoised=False, model_kwargs={"y": yy}, skip_timesteps=skip, init_image=init,
                 progress=False, dump_steps=None, noise=None, const_noise=False).contiguous()
        tl[idx, :, :, w * S:w * S + T] = torch.where(mask, motion, s)
        masks.append(mask)
        wins.append(s)
    return tl, plan, torch.cat(wins), masks


def _editable(cfg, ranges, joints, device):
    ed = torch.zeros((B, cfg.njoints, cfg.nfeats, N), dtype=torch.bool, device=device)
    sel = torch.ones(B, cfg.njoints, dtype=torch.bool) if joints is None else torch.from_numpy(joints)
    for b, (lo, hi) in enumerate(ranges):
        ed[b, :, :, lo:hi] = sel[b].to(device)[:, None, None]
    return ed


def _check_contract_1(parts, ranges, joints, want_plan, seed=23, **kw):
    """Contract 1 and 5 on one case: the public loop, then edit_long twice (the second call replays every window)."""
    cfg, model, diffusion, sampler, skip, y, timeline, frames = parts
    lens = kw.get("audio_lengths")
    sag_kw = {k: kw[k] for k in ("sag", "text_features") if k in kw}
    torch.manual_seed(seed)
    want, plan, want_w, masks = _by_public_loop(parts, ranges, joints, lens, sag_kw.get("sag"), sag_kw.get("text_features"))
    assert plan == want_plan                                    # neither an empty nor a dense plan passes
    n_pairs = sum(len(rows) for _, rows in plan)
    assert want_w.shape == (n_pairs, cfg.njoints, cfg.nfeats, T)
    assert any(bool(m.any()) and not bool(m.all()) for m in masks)
    before = timeline.clone()
    eng = model.model.engine()
    for rep in range(2):
        torch.manual_seed(seed)
        tl, ran, wins = _edit(parts, ranges, joints, return_windows=True, compact=True, **kw)
        assert ran == plan and tl.shape == timeline.shape and tl.device == timeline.device and wins.shape == want_w.shape
        assert bool(torch.isfinite(tl).all())
        print(f"{cfg.name} rep {rep}: max |compact edit - public loop| = {float((tl - want).abs().max()):.3e}, "
              f"raw windows {float((wins - want_w).abs().max()):.3e}")
        assert torch.equal(wins, want_w), (rep, float((wins - want_w).abs().max()))
        assert torch.equal(tl, want), (rep, float((tl - want).abs().max()))
        t = eng.timing()
        assert t["n_segments"] == len(plan) and t["n_step_launches"] == len(plan) * 12 and eng.rows_run == n_pairs
    if diffusion.use_graph:
        assert t["graph_replayed"] == len(plan)                 # no window of the second call captured anything
    assert torch.equal(timeline, before)                        # the caller's timeline is never written
    ed = _editable(cfg, ranges, joints, timeline.device)
    assert torch.equal(tl[~ed], timeline[~ed]) and not torch.equal(tl[ed], timeline[ed])
    return tl


@pytest.mark.parametrize("schedule", ["ddim", "ddpm"])
@pytest.mark.parametrize("ds", ["ted", "beat"])
def test_equal_lengths_are_bitwise_the_public_loop_on_the_rows(ds, schedule):
    parts = _start(ds, schedule)
    timeline = parts[6]
    tl = _check_contract_1(parts, EQUAL, _joints(parts[0]), EQUAL_PLAN)
    assert torch.equal(tl[1], timeline[1])                      # clip 1 is in no window
    assert not torch.equal(tl[0, :, :, 20:50], timeline[0, :, :, 20:50]) and not torch.equal(tl[2, 1, :, 70:80], timeline[2, 1, :, 70:80])
    assert torch.equal(tl[2, 0], timeline[2, 0])                # a joint of clip 2 that is not selected


def test_edit_without_skip_starts_from_x_T():
    assert SCHEDULES["ddim_noskip"][3] == 0
    _check_contract_1(_start("ted", "ddim_noskip"), EQUAL, None, EQUAL_PLAN)


@pytest.mark.parametrize("ds", ["ted", "beat"])
def test_a_ragged_batch_is_edited_and_nothing_beyond_a_clips_length_is_read(ds):
    parts = _start(ds, "ddim", True, True)
    cfg, timeline, frames, y = parts[0], parts[6], parts[7], parts[5]
    lens = _lengths(cfg)
    tl = _check_contract_1(parts, RAGGED, None, RAGGED_PLAN, audio_lengths=lens)
    for b, f in enumerate(frames):                              # frames beyond frames[b]: bit for bit as given
        assert torch.equal(tl[b, ..., int(f):], timeline[b, ..., int(f):]) and (b in (0, 2) or bool((tl[b, ..., int(f):] == 3.25 + b).all()))
    # contract 4: NaN from each clip's own length on changes nothing
    poisoned = y["audio"].clone()
    for b, n in enumerate(lens):
        poisoned[b, n:] = float("nan")
    assert bool(torch.isnan(poisoned).any())
    torch.manual_seed(23)
    again = _edit(parts, RAGGED, audio=poisoned, audio_lengths=lens)        # audio_lengths alone implies the compact form
    assert bool(torch.isfinite(again).all()) and torch.equal(again, tl)
    # the ranges are checked against each clip's own frames, ahead of the engine
    with pytest.raises(ValueError, match="frames"):
        _edit(parts, np.array([(20, 50), (5, 40), (70, 80), (40, 64)]), audio_lengths=lens)


def test_a_ragged_timeline_made_without_drop_finished():
    parts = _start("ted", "ddim", False, True)
    _check_contract_1(parts, RAGGED, _joints(parts[0]), RAGGED_PLAN, audio_lengths=_lengths(parts[0]))


@pytest.mark.parametrize("ds", ["ted", "beat"])
def test_identity_tables_reproduce_the_dense_call(ds):
    parts = _start(ds, "ddim")
    diffusion, timeline = parts[2], parts[6]
    assert long_form.edit_plan_compact(WHOLE, W, parts[0]) == [(w, [0, 1, 2, 3]) for w in range(W)]
    for source in ("torch_cpu", "philox"):
        diffusion.noise_source, diffusion.philox_seed = source, (0x1234_5678_9ABC if source == "philox" else None)
        try:
            torch.manual_seed(31)
            dense, ran, dense_w = _edit(parts, WHOLE, return_windows=True)
            torch.manual_seed(31)
            tl, plan, wins = _edit(parts, WHOLE, return_windows=True, compact=True)
            assert ran == [0, 1, 2] and [w for w, _ in plan] == ran
            assert torch.equal(wins, dense_w.reshape(W * B, *dense_w.shape[2:])), (source, float((wins.reshape(dense_w.shape) - dense_w).abs().max()))
            assert torch.equal(tl, dense) and not torch.equal(tl[..., 10:90], timeline[..., 10:90]), source
        finally:
            diffusion.noise_source, diffusion.philox_seed = "torch_cpu", None


@pytest.mark.parametrize("ds", ["ted", "beat"])
def test_philox_draws_follow_the_clip_not_the_row(ds):
    parts = _start(ds, "ddim")
    diffusion, timeline = parts[2], parts[6]
    with_0 = np.array([(40, 45), (0, 0), (40, 45), (0, 0)])     # A_1 = {0, 2}: clip 2 at row 1
    with_3 = np.array([(0, 0), (0, 0), (40, 45), (40, 45)])     # A_1 = {2, 3}: clip 2 at row 0
    diffusion.noise_source, diffusion.philox_seed = "philox", 0x1234_5678_9ABC
    try:
        a, plan_a, win_a = _edit(parts, with_0, return_windows=True, compact=True)
        b = _edit(parts, with_0, compact=True)
        assert plan_a == [(1, [0, 2])] and torch.equal(a, b) and bool(torch.isfinite(a).all())
        c, plan_c, win_c = _edit(parts, with_3, return_windows=True, compact=True)
        assert plan_c == [(1, [2, 3])]
        assert not torch.equal(a[2, :, :, 40:45], timeline[2, :, :, 40:45])
        assert torch.equal(win_a[1], win_c[0])                  # clip 2's raw window, at row 1 and at row 0
        assert torch.equal(a[2], c[2])
        assert torch.equal(a[3], timeline[3]) and torch.equal(c[0], timeline[0]) and torch.equal(a[1], timeline[1])
        assert not torch.equal(win_a[0], win_c[1])              # other clips, other streams
        diffusion.philox_seed = 77
        assert not torch.equal(_edit(parts, with_0, compact=True)[2, :, :, 40:45], a[2, :, :, 40:45])
    finally:
        diffusion.noise_source, diffusion.philox_seed = "torch_cpu", None


def test_a_scripted_compact_edit_is_bitwise_the_public_loop_with_the_decoder():
    parts = _start("ted", "ddim")
    sag, text = _script("ted")
    poisoned = text.clone()                                     # rows of pairs outside the plan are not used
    used = torch.zeros(B, W, dtype=torch.bool)
    for w, rows in EQUAL_PLAN:
        used[rows, w] = True
    poisoned[~used.to(DEV)] = float("nan")
    assert int(used.sum()) == 5
    _check_contract_1(parts, EQUAL, _joints(parts[0]), EQUAL_PLAN, sag=sag, text_features=poisoned)


@pytest.mark.engine_path_auto
def test_contract_on_the_kernels_auto_picks_per_window_batch():
    """Under `auto` batches 1 and 2 run the sample-split kernel at their own slicings, with hand-off tags that advance per window.
    A model of its own: the cached ones hold engines pinned to the fused kernel."""
    parts = _start_of("ted", "ddim", fresh=True)
    _check_contract_1(parts, EQUAL, _joints(parts[0]), EQUAL_PLAN, seed=29)
    assert parts[1].model.engine().path == "auto"


def test_engine_refusals_leave_the_handle_usable():
    parts = _start("ted", "ddim")
    cfg, model, diffusion, sampler, skip, y, timeline, _ = parts
    diffusion.noise_source, diffusion.philox_seed = "philox", 9
    try:
        dense_before = _edit(parts, (40, 45))
        eng = diffusion._bind_schedule(model.model.engine())
        model.model._cond_key = model.model._prefetched_key = None
        lo, hi = EQUAL[:, 0].astype(np.int32), EQUAL[:, 1].astype(np.int32)
        kw = dict(sampler=_lib.LS_SAMPLER_DDIM, skip_timesteps=skip, philox_seed=9, inpaint_noised=True, device_out=True)
        args = (y["audio"].float(), y["seed_poses"].float(), y["vid_indices"], y["scale"].float())
        eng.long_prepare(*args, n_windows=W)
        with pytest.raises(_lib.EngineError, match="before ls_long_prepare_edit"):
            eng.long_edit_compact(timeline, lo, hi, **kw)
        with pytest.raises(_lib.EngineError, match="empty"):
            eng.long_prepare_edit(*args, lo, lo, n_windows=W)
        with pytest.raises(_lib.EngineError, match="range"):
            eng.long_prepare_edit(*args, lo, hi + N, n_windows=W)
        eng.long_prepare_edit(*args, lo, hi, n_windows=W)
        assert [(w, rows.tolist()) for w, rows in eng.edit_plan] == EQUAL_PLAN
        with pytest.raises(_lib.EngineError, match="before ls_long_prepare"):
            eng.long_edit(timeline, lo, hi, **kw)                           # the dense edit needs every clip-window's features
        other = hi.copy()
        other[0] += 1
        with pytest.raises(_lib.EngineError, match="ranges differ"):
            eng.long_edit_compact(timeline, lo, other, **kw)
        with pytest.raises(_lib.EngineError, match="channels differ"):
            eng.long_edit_compact(timeline, lo, hi, channels=np.ones((B, cfg.njoints * cfg.nfeats), np.uint8), **kw)
        with pytest.raises(_lib.EngineError, match="DDPM and DDIM"):
            eng.long_edit_compact(timeline, lo, hi, **dict(kw, sampler=_lib.LS_SAMPLER_PLMS))
        sag, text = _script("ted")
        with pytest.raises(_lib.EngineError, match="sag without text_features"):
            eng.long_edit_compact(timeline, lo, hi, sag=sag.engine(), **kw)
        with pytest.raises(_lib.EngineError, match="text_features without sag"):
            eng.long_edit_compact(timeline, lo, hi, text_features=text.permute(1, 0, 2).contiguous(), **kw)
        tl, plan = eng.long_edit_compact(timeline, lo, hi, **kw)            # the handle still holds its plan
        assert [(w, rows.tolist()) for w, rows in plan] == EQUAL_PLAN and bool(torch.isfinite(tl).all())
        assert torch.equal(tl, _edit(parts, EQUAL, compact=True))           # the engine's result is edit_long's with the same key
        assert torch.equal(_edit(parts, (40, 45)), dense_before)            # and a following dense edit gives its own bits
    finally:
        diffusion.noise_source, diffusion.philox_seed = "torch_cpu", None
