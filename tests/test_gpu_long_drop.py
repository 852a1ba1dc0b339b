"""sample_long(audio_lengths=, drop_finished=True) on the GPU (ls_long_prepare_ragged, k_long_gather_clips, the ragged k_chain_window).

The contract: with noise_source='torch_cpu' the timeline and the raw windows are BIT FOR BIT the window-by-window loop of public
sampling calls in which window w runs only the clips that still have audio -- one call at batch B_w on the slot-ordered active
subset (long_form.plan_drop), audio counting as zero beyond each clip's length, the prefix poses carried per clip, the results
scattered back to the caller's order.  B = 5 with window counts [2, 3, 1, 3, 1]: unsorted, with ties, one pair of clips finishes
first and another runs to the end, so the batches are 5, 3, 2.  Every comparison is torch.equal."""
import numpy as np
import pytest
import torch

from livelyspeaker_amd import long_form, synth
from livelyspeaker_amd.motionclip_module import Decoder_TRANSFORMER
from test_gpu_long_form import DEV, _inputs, _long, _parts, _window_by_window
from test_long_drop_host import lengths_for

pytestmark = pytest.mark.gpu
COUNTS = [2, 3, 1, 3, 1]


def _sample(diffusion, model, cfg, rows, audio_w, prefix, y, w, sampler, skip, sag, text, offset):
    """One public sampling call for window w on the clips `rows` (slot order)."""
    n = rows.numel()
    shape = (n, cfg.njoints, cfg.nfeats, cfg.nframes)
    origin_x = torch.zeros(shape, device=prefix.device)
    origin_x[..., :cfg.n_pre_seq] = prefix
    yy = {"audio_input": audio_w[rows].contiguous(), "origin_x": origin_x, "vid_indices": y["vid_indices"][rows].contiguous(),
          "scale": y["scale"][rows].contiguous()}
    if "emo" in y:
        yy["emo"] = y["emo"][rows, w:w + 1].expand(n, cfg.nframes).contiguous()
    if offset is not None:
        diffusion.sample_offset = offset
    init = None
    if sag is not None:
        init = sag({"x": origin_x.clone(), "z": text[rows, w].contiguous(), "mask": torch.ones(n, cfg.nframes, device=prefix.device).bool()})["output"]
    loop = diffusion.ddim_sample_loop if sampler == "ddim" else diffusion.p_sample_loop
    return loop(model, shape, clip_denoised=False, model_kwargs={"y": yy}, skip_timesteps=skip, init_image=init, progress=False,
                dump_steps=None, noise=None, const_noise=False).contiguous()


def _drop_loop(diffusion, model, cfg, y, lens, sampler, skip, sag=None, text=None, philox_base=None):
    """The loop the dropping call stands for: (timeline, windows) in the caller's clip order, zero where a clip has no window."""
    order, _, active, _ = long_form.plan_drop(lens, cfg)
    dev, B, W, T, npre = y["audio"].device, len(lens), len(active), cfg.nframes, cfg.n_pre_seq
    valid = torch.arange(y["audio"].shape[1], device=dev)[None, :] < torch.as_tensor(np.asarray(lens), device=dev)[:, None]
    audio = torch.where(valid, y["audio"], torch.zeros((), device=dev))
    order = torch.as_tensor(order, device=dev)
    wins = torch.zeros((W, B, cfg.njoints, cfg.nfeats, T), device=dev)
    timeline = torch.zeros((B, cfg.njoints, cfg.nfeats, T + (W - 1) * (T - npre)), device=dev)
    prefix = y["seed_poses"][order]
    for w, n in enumerate(int(v) for v in active):
        rows = order[:n]
        s = _sample(diffusion, model, cfg, rows, long_form.window_audio(audio, w, cfg), prefix[:n], y, w, sampler, skip, sag, text,
                    None if philox_base is None else philox_base + (w << 48))
        wins[w, rows] = s
        if w == 0:
            timeline[rows, :, :, :T] = s
        else:
            timeline[rows, :, :, T + (w - 1) * (T - npre):T + w * (T - npre)] = s[..., npre:]
        prefix = s[..., T - npre:]
    return timeline, wins


def _drop(diffusion, model, y, lens, sampler, skip, **kw):
    return _long(diffusion, model, y, sampler, skip, audio_lengths=lens, drop_finished=True, **kw)


def _check_zeros(cfg, lens, tl, frames, wins):
    plans = long_form.plan_lengths(lens, cfg)
    assert frames.dtype == np.int32 and frames.tolist() == [f for _, f in plans]
    for b, (Wb, fb) in enumerate(plans):
        assert not bool(tl[b, ..., fb:].any()) and bool(tl[b, ..., :fb].abs().sum() > 0)
        assert not bool(wins[Wb:, b].any()) and bool(wins[:Wb, b].abs().sum() > 0)
    assert bool(torch.isfinite(tl).all()) and bool(torch.isfinite(wins).all())


def _check_contract(ds, schedule, counts=COUNTS, seed=17):
    cfg, model, diffusion, sampler, skip = _parts(ds, schedule)
    B, W = len(counts), max(counts)
    y = _inputs(cfg, B, W)
    lens = lengths_for(counts, cfg)
    active = long_form.plan_drop(lens, cfg)[2].tolist()
    torch.manual_seed(seed)
    want_tl, want_w = _drop_loop(diffusion, model, cfg, y, lens, sampler, skip)
    repeated = sum(1 for n in active if active.count(n) >= 2)      # windows whose batch size serves two or more windows
    for rep in range(2):
        torch.manual_seed(seed)
        tl, frames, wins = _drop(diffusion, model, y, lens, sampler, skip, return_windows=True)
        assert tl.shape == want_tl.shape and wins.shape == want_w.shape and tl.device == y["audio"].device
        assert torch.equal(wins, want_w), (rep, float((wins - want_w).abs().max()))
        assert torch.equal(tl, want_tl), (rep, float((tl - want_tl).abs().max()))
        t = model.model.engine().timing()
        assert t["n_segments"] == W and t["n_step_launches"] == W * (diffusion.num_timesteps - skip)
        if diffusion.use_graph:                             # a batch captured in the first call is replayed from its second window on
            assert t["graph_replayed"] == (repeated if rep else repeated - len({n for n in active if active.count(n) >= 2})), (rep, t)
    _check_zeros(cfg, lens, tl, frames, wins)
    for b, Wb in enumerate(counts):                         # the oracle's windows differ from one another (the check has teeth)
        assert all(not torch.equal(want_w[w, b], want_w[w + 1, b]) for w in range(Wb - 1))
    return cfg, model, diffusion, y, lens, tl, wins


@pytest.mark.parametrize("schedule", ["ddim", "ddpm"])
@pytest.mark.parametrize("ds", ["ted", "beat"])
def test_dropping_call_is_bitwise_the_loop_over_the_active_clips(ds, schedule):
    _check_contract(ds, schedule)


@pytest.mark.engine_path_auto
@pytest.mark.parametrize("ds", ["ted", "beat"])
def test_contract_on_the_kernels_auto_picks_at_5_then_3_then_2_clips(ds):
    _check_contract(ds, "ddim")


def test_a_batch_size_that_serves_two_windows_is_captured_once_and_replayed():
    """Window counts [3, 1, 3]: batches 3, 2, 2 -- the loop at batch 2 is captured at window 1 and replayed at window 2, beside
    window 0's plain launches at batch 3 (the handle's graph cache)."""
    _check_contract("ted", "ddim", counts=[3, 1, 3], seed=4)


@pytest.mark.parametrize("ds", ["ted", "beat"])
def test_zeros_shapes_nan_tails_and_no_graph(ds):
    cfg, model, diffusion, sampler, skip = _parts(ds, "ddim")
    y = _inputs(cfg, 5, 3)
    lens = lengths_for(COUNTS, cfg)
    torch.manual_seed(8)
    tl, frames, wins = _drop(diffusion, model, y, lens, sampler, skip, return_windows=True)
    _check_zeros(cfg, lens, tl, frames, wins)
    assert tl.shape == (5, cfg.njoints, cfg.nfeats, 34 + 2 * 30) and wins.shape == (3, 5, cfg.njoints, cfg.nfeats, 34)
    # samples beyond a clip's length are never read: NaN there changes nothing
    audio = y["audio"].clone()
    for b, n in enumerate(lens):
        audio[b, int(n):] = float("nan")
    torch.manual_seed(8)
    tl2, frames2, wins2 = _drop(diffusion, model, dict(y, audio=audio), lens, sampler, skip, return_windows=True)
    assert torch.equal(tl2, tl) and torch.equal(wins2, wins) and np.array_equal(frames2, frames)
    assert bool(torch.isnan(audio).any()) and bool(torch.isfinite(tl2).all())
    # without return_windows: (timeline, frames)
    torch.manual_seed(8)
    res = _drop(diffusion, model, y, lens, sampler, skip)
    assert len(res) == 2 and torch.equal(res[0], tl)
    # stream launches give the bits of the captured loops
    diffusion.use_graph = False
    torch.manual_seed(8)
    tl3, _, wins3 = _drop(diffusion, model, y, lens, sampler, skip, return_windows=True)
    assert torch.equal(tl3, tl) and torch.equal(wins3, wins)
    assert model.model.engine().timing()["graph_replayed"] == 0


@pytest.mark.parametrize("ds", ["ted", "beat"])
def test_philox_streams_follow_the_slot(ds):
    cfg, model, diffusion, sampler, skip = _parts(ds, "ddim")
    diffusion.noise_source = "philox"
    diffusion.philox_seed = 0x1234_5678_9ABC
    y = _inputs(cfg, 5, 3)
    # a batch that is already longest-first: the draws, and on the pinned kernel path the bits, of the call that drops nothing
    counts = [3, 3, 2, 1, 1]
    lens = lengths_for(counts, cfg)
    assert long_form.plan_drop(lens, cfg)[0].tolist() == [0, 1, 2, 3, 4]
    tl, frames, wins = _drop(diffusion, model, y, lens, sampler, skip, return_windows=True)
    full_tl, full_frames, full_w = _long(diffusion, model, y, sampler, skip, audio_lengths=lens, return_windows=True)
    assert np.array_equal(frames, full_frames)
    for b, Wb in enumerate(counts):
        assert torch.equal(tl[b, ..., :frames[b]], full_tl[b, ..., :frames[b]]), b
        assert torch.equal(wins[:Wb, b], full_w[:Wb, b]), b
    _check_zeros(cfg, lens, tl, frames, wins)
    again = _drop(diffusion, model, y, lens, sampler, skip)[0]
    assert torch.equal(again, tl)                                     # reproducible
    # ... and the loop of plain Philox calls at the documented offsets
    want_tl, want_w = _drop_loop(diffusion, model, cfg, y, lens, sampler, skip, philox_base=0)
    diffusion.sample_offset = 0
    assert torch.equal(wins, want_w) and torch.equal(tl, want_tl)
    # any other order: the call on the slot-ordered inputs, scattered back
    lens_u = lengths_for(COUNTS, cfg)
    order = torch.as_tensor(long_form.plan_drop(lens_u, cfg)[0], device=DEV)
    tl_u, frames_u, wins_u = _drop(diffusion, model, y, lens_u, sampler, skip, return_windows=True)
    ys = {k: v[order].contiguous() for k, v in y.items()}
    tl_s, frames_s, wins_s = _drop(diffusion, model, ys, lens_u[order.cpu().numpy()], sampler, skip, return_windows=True)
    assert torch.equal(tl_u[order], tl_s) and torch.equal(wins_u[:, order], wins_s) and np.array_equal(frames_u[order.cpu().numpy()], frames_s)
    _check_zeros(cfg, lens_u, tl_u, frames_u, wins_u)
    diffusion.philox_seed = 77
    assert not torch.equal(_drop(diffusion, model, y, lens_u, sampler, skip)[0], tl_u)


@pytest.mark.parametrize("ds", ["ted", "beat"])
def test_sag_chain_is_bitwise_the_decoder_then_refine_loop_on_the_active_clips(ds):
    cfg, model, diffusion, sampler, skip = _parts(ds, "ddim")
    sag = Decoder_TRANSFORMER(njoints=cfg.njoints, nfeats=cfg.nfeats, latent_dim=512, n_pre_poses=4, use_style=False)
    sag.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_sag_state_dict(cfg).items()}, strict=False)
    sag.to(DEV).eval()
    B, W = 5, 3
    y = _inputs(cfg, B, W)
    lens = lengths_for(COUNTS, cfg)
    text = torch.from_numpy(synth.make_text_features(B * W).reshape(B, W, 512)).to(DEV)
    torch.manual_seed(21)
    want_tl, want_w = _drop_loop(diffusion, model, cfg, y, lens, sampler, skip, sag=sag, text=text)
    for rep in range(2):
        torch.manual_seed(21)
        tl, _, wins = _drop(diffusion, model, y, lens, sampler, skip, sag=sag, text_features=text, return_windows=True)
        assert torch.equal(wins, want_w) and torch.equal(tl, want_tl), (rep, float((wins - want_w).abs().max()))
    torch.manual_seed(21)
    assert not torch.equal(_drop(diffusion, model, y, lens, sampler, skip)[0], tl)       # the decoder's init_image matters


@pytest.mark.parametrize("ds", ["ted", "beat"])
def test_host_inputs_encoder_chunk_handle_reuse_and_scoring(ds):
    cfg, model, diffusion, sampler, skip = _parts(ds, "ddim")
    y = _inputs(cfg, 5, 3)
    lens = lengths_for(COUNTS, cfg)
    torch.manual_seed(9)
    tl, frames, wins = _drop(diffusion, model, y, lens, sampler, skip, return_windows=True)
    # ten clip-windows through the encoder as 2, 2, 2, 2, 2 (chunks that straddle windows)
    torch.manual_seed(9)
    assert torch.equal(_drop(diffusion, model, y, lens, sampler, skip, encoder_chunk=2)[0], tl)
    torch.manual_seed(9)
    assert torch.equal(_drop(diffusion, model, y, lens, sampler, skip, encoder_chunk=3)[0], tl)
    # host inputs: a host result with the same bits
    yh = {k: v.cpu() for k, v in y.items()}
    torch.manual_seed(9)
    host_tl, host_frames, host_w = _drop(diffusion, model, yh, lens, sampler, skip, return_windows=True)
    assert not host_tl.is_cuda and not host_w.is_cuda
    assert torch.equal(host_tl, tl.cpu()) and torch.equal(host_w, wins.cpu()) and np.array_equal(host_frames, frames)
    # the chain behind it takes the result as it is
    res = long_form.score_timeline(tl, y["audio"], dataset=ds, frames=frames, audio_lengths=lens)
    first = res["pose" if ds == "ted" else "pred_euler"]
    assert first.shape[0] == 5 and bool(torch.isfinite(torch.as_tensor(res["beat_mask"]).float()).all())
    # the handle afterwards: a plain long call and a plain sampling call give what a fresh handle gives
    y2 = {k: (v[:, :2].contiguous() if k == "emo" else v) for k, v in y.items()}
    torch.manual_seed(9)
    plain_long = _long(diffusion, model, y2, sampler, skip, n_windows=2)
    torch.manual_seed(9)
    plain, _ = _window_by_window(diffusion, model, cfg, y, 1, sampler, skip)
    _, fresh_model, fresh_diffusion, _, _ = _parts(ds, "ddim")
    torch.manual_seed(9)
    assert torch.equal(_long(fresh_diffusion, fresh_model, y2, sampler, skip, n_windows=2), plain_long)
    torch.manual_seed(9)
    fresh_plain, _ = _window_by_window(fresh_diffusion, fresh_model, cfg, y, 1, sampler, skip)
    assert torch.equal(fresh_plain, plain)
    # ... and the dropping call again, behind them
    torch.manual_seed(9)
    assert torch.equal(_drop(diffusion, model, y, lens, sampler, skip)[0], tl)
