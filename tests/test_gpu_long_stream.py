"""Streaming long-form synthesis on the GPU (long_form.open_stream -> ls_long_stream_open / ls_long_stream_push, the session of
csrc/ls_chain_api.cpp with all slots fed alike).

The contract: the frames of all pushes and the close, concatenated, are BIT FOR BIT the timeline ``sample_long`` gives for the concatenated
audio (same model, schedule, conditioning and seed; no n_windows, no audio_lengths), whatever the chunking.  B = 3 (odd: per-clip
indexing), 12 executed steps per window (1000 steps respaced to 100, skip 88), both datasets, synthetic weights;
L = audio_len + 2 * 32000 - 5000: three windows, the last one zero-padded."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from livelyspeaker_amd import _lib, long_form, synth
from livelyspeaker_amd.cfg_sampler import ClassifierFreeSampleModel
from livelyspeaker_amd.model_util import create_model_and_diffusion, load_model_wo_clip
from livelyspeaker_amd.motionclip_module import Decoder_TRANSFORMER

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B, W, T, S, STRIDE = 3, 3, 34, 30, 32000
SCHEDULES = {"ddim": (1000, "ddim100", "ddim", 88), "ddpm": (1000, "100", "ddpm", 88)}


def _length(cfg):
    return cfg.audio_len + 2 * STRIDE - 5000


def _edge_chunks(cfg):
    """Window 0 and window 1 each complete exactly on a chunk's last sample; the close runs the padded window 2."""
    head = [1, cfg.audio_len - 1, STRIDE - 1, 1]
    return head + [_length(cfg) - sum(head)]


@functools.lru_cache(maxsize=None)
def _parts(ds, schedule):
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
    y = {k: torch.from_numpy(v).to(DEV) for k, v in synth.make_long_cond(cfg, B, 6).items()}      # audio for up to six windows
    return cfg, model, diffusion, sampler, skip, y


def _sample_long(parts, audio, emo=None, **kw):
    cfg, model, diffusion, sampler, skip, y = parts
    return long_form.sample_long(diffusion, model, audio, y["seed_poses"], y["vid_indices"], y["scale"], emo=emo, sampler=sampler,
                                 skip_timesteps=skip, **kw)


def _stream(parts, audio, sizes, emo=None, sag=None, text=None, seen=None):
    """Feed ``audio`` in chunks of ``sizes`` samples, then close.  ``emo`` [B] is held from open_stream on; ``emo`` [B, W] / ``text``
    [B, W, 512] pass, with every push and with the close, the value of the window that call would start.  Returns the list of frame
    tensors (pushes, then the close) and the stream."""
    cfg, model, diffusion, sampler, skip, y = parts
    assert sum(sizes) == audio.shape[1]
    per_window = emo is not None and emo.ndim == 2
    st = long_form.open_stream(diffusion, model, y["seed_poses"], y["vid_indices"], y["scale"], emo=None if per_window else emo,
                               sampler=sampler, skip_timesteps=skip, sag=sag)

    def held():
        w = st.windows_run
        kw = {}
        if per_window and w < emo.shape[1]:
            kw["emo"] = emo[:, w]
        if text is not None and w < text.shape[1]:
            kw["text_features"] = text[:, w]
        return kw

    outs, pos = [], 0
    for n in sizes:
        outs.append(st.push(audio[:, pos:pos + n], **held()))
        pos += n
        if seen is not None:
            seen(st, outs[-1])
    outs.append(st.close(**held()))
    assert st.samples_in == audio.shape[1] and st.frames_out == sum(int(o.shape[3]) for o in outs)
    assert st.windows_run == long_form.plan_windows(audio.shape[1], cfg)[0]
    return outs, st


def _emo(parts):
    return parts[5]["emo"][:, :W].contiguous() if "emo" in parts[5] else None


@pytest.mark.parametrize("schedule", ["ddim", "ddpm"])
@pytest.mark.parametrize("ds", ["ted", "beat"])
def test_stream_is_bitwise_sample_long(ds, schedule):
    parts = _parts(ds, schedule)
    cfg, model = parts[0], parts[1]
    audio = parts[5]["audio"][:, :_length(cfg)].contiguous()
    emo = _emo(parts)                                       # BEAT: a different id per window
    assert emo is None or not torch.equal(emo[:, 0], emo[:, 1])
    torch.manual_seed(31)
    want = _sample_long(parts, audio, emo=emo)
    assert want.shape == (B, cfg.njoints, cfg.nfeats, T + 2 * S)
    for rep in range(2):                                    # the second stream replays the captured loop from its first window on
        torch.manual_seed(31)
        outs, st = _stream(parts, audio, _edge_chunks(cfg), emo=emo)
        assert [int(o.shape[3]) for o in outs] == [0, T, 0, S, 0, S]
        assert all(o.shape[:3] == want.shape[:3] and o.device == audio.device for o in outs)
        got = torch.cat(outs, dim=3)
        print(f"{ds} {schedule} rep {rep}: max |stream - sample_long| = {float((got - want).abs().max()):.3e}")
        assert bool(torch.isfinite(got).all()) and torch.equal(got, want), (rep, float((got - want).abs().max()))
    info = model.model.engine().long_stream_info()
    assert (info["samples_in"], info["windows_run"], info["frames_out"]) == (st.samples_in, 3, T + 2 * S)


@pytest.mark.parametrize("ds", ["ted", "beat"])
def test_the_chunking_cannot_matter(ds):
    parts = _parts(ds, "ddim")
    cfg, diffusion = parts[0], parts[2]
    L = _length(cfg)
    audio = parts[5]["audio"][:, :L].contiguous()
    emo = None if _emo(parts) is None else _emo(parts)[:, 0].contiguous()          # one id per clip: a push here may run two windows
    diffusion.noise_source, diffusion.philox_seed = "philox", 0x2468_ACE0_1357
    try:
        want = _sample_long(parts, audio, emo=emo)
        chunkings = {"edges": _edge_chunks(cfg), "all at once": [L], "4000 samples": [4000] * (L // 4000) + [L % 4000]}
        for name, sizes in chunkings.items():
            outs, _ = _stream(parts, audio, sizes, emo=emo)
            got = torch.cat(outs, dim=3)
            assert torch.equal(got, want), (name, float((got - want).abs().max()))
        assert [int(o.shape[3]) for o in outs[:9]] == [0] * 9 and int(outs[9].shape[3]) == T      # 10 x 4000 >= audio_len
        diffusion.philox_seed = 99
        assert not torch.equal(torch.cat(_stream(parts, audio, [L], emo=emo)[0], dim=3), want)
    finally:
        diffusion.noise_source, diffusion.philox_seed = "torch_cpu", None


def test_sag_chain_is_bitwise_sample_long():
    parts = _parts("ted", "ddim")
    cfg = parts[0]
    sag = Decoder_TRANSFORMER(njoints=cfg.njoints, nfeats=cfg.nfeats, latent_dim=512, n_pre_poses=4, use_style=False)
    sag.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_sag_state_dict(cfg).items()}, strict=False)
    sag.to(DEV).eval()
    text = torch.from_numpy(synth.make_text_features(B * W).reshape(B, W, 512)).to(DEV)
    assert not torch.equal(text[:, 0], text[:, 1])
    audio = parts[5]["audio"][:, :_length(cfg)].contiguous()
    torch.manual_seed(37)
    want = _sample_long(parts, audio, sag=sag, text_features=text)
    torch.manual_seed(37)
    plain = _sample_long(parts, audio)
    assert not torch.equal(plain, want)                     # the decoder's init_image matters
    torch.manual_seed(37)
    outs, _ = _stream(parts, audio, _edge_chunks(cfg), sag=sag, text=text)
    got = torch.cat(outs, dim=3)
    assert torch.equal(got, want), float((got - want).abs().max())


@pytest.mark.parametrize("ds", ["ted", "beat"])
def test_short_and_exact_streams(ds):
    parts = _parts(ds, "ddim")
    cfg = parts[0]
    emo = None if _emo(parts) is None else _emo(parts)[:, 0].contiguous()
    # shorter than one window: no push returns frames, the close returns all 34
    audio = parts[5]["audio"][:, :20000].contiguous()
    torch.manual_seed(43)
    want = _sample_long(parts, audio, emo=emo)
    torch.manual_seed(43)
    outs, _ = _stream(parts, audio, [5000, 0, 15000], emo=emo)
    assert [int(o.shape[3]) for o in outs] == [0, 0, 0, T] and torch.equal(outs[-1], want)
    # host inputs: host frames with the same bits
    host = parts[:5] + ({k: v.cpu() for k, v in parts[5].items()},)
    torch.manual_seed(43)
    outs, _ = _stream(host, audio.cpu().numpy(), [5000, 0, 15000], emo=None if emo is None else emo.cpu())
    assert all(not o.is_cuda for o in outs) and torch.equal(outs[-1], want.cpu())
    # exactly audio_len + 32000 samples: two windows, nothing left for the close
    audio = parts[5]["audio"][:, :cfg.audio_len + STRIDE].contiguous()
    torch.manual_seed(47)
    want = _sample_long(parts, audio, emo=emo)
    torch.manual_seed(47)
    outs, _ = _stream(parts, audio, [cfg.audio_len + STRIDE - 1, 1], emo=emo)
    assert [int(o.shape[3]) for o in outs] == [T, S, 0] and outs[-1].shape == (B, cfg.njoints, cfg.nfeats, 0)
    assert torch.equal(torch.cat(outs, dim=3), want)


def test_memory_is_bounded_and_the_captured_loop_is_replayed():
    parts = _parts("ted", "ddim")
    cfg, model, diffusion = parts[0], parts[1], parts[2]
    L = cfg.audio_len + 5 * STRIDE                          # six windows
    audio = parts[5]["audio"][:, :L].contiguous()
    assert audio.shape[1] == L
    eng = lambda: model.model.engine()                      # noqa: E731
    seen = []

    def note(st, frames):
        if int(frames.shape[3]):
            seen.append((st.windows_run, eng().long_stream_info()["device_bytes"], eng().timing()["graph_replayed"], eng().timing()["n_segments"]))

    diffusion.noise_source, diffusion.philox_seed = "philox", 5
    try:
        sizes = [STRIDE] * (L // STRIDE) + [L % STRIDE]     # equal chunks; every push completes at most one window
        outs, st = _stream(parts, audio, sizes, seen=note)
        assert torch.equal(torch.cat(outs, dim=3), _sample_long(parts, audio))
    finally:
        diffusion.noise_source, diffusion.philox_seed = "torch_cpu", None
    assert [s[0] for s in seen] == [1, 2, 3, 4, 5, 6] and int(outs[-1].shape[3]) == 0
    by_window = {s[0] - 1: s for s in seen}
    assert by_window[1][1] == by_window[5][1] > 0           # the bytes the stream holds after window 1 and after window 5
    ring = (cfg.audio_len + STRIDE + 3) // 4 * 4
    assert by_window[5][1] >= B * (ring + cfg.audio_len + T * 256) * 4
    assert all(s[3] == 1 for s in seen)
    if diffusion.use_graph:
        assert all(s[2] == 1 for s in seen[1:])             # every window after the first capture replays it


def test_a_plain_sampling_call_ends_the_stream_and_the_handle_stays_usable():
    parts = _parts("ted", "ddim")
    cfg, model, diffusion, sampler, skip, y = parts
    audio = y["audio"][:, :_length(cfg)].contiguous()
    st = long_form.open_stream(diffusion, model, y["seed_poses"], y["vid_indices"], y["scale"], sampler=sampler, skip_timesteps=skip)
    torch.manual_seed(3)
    assert st.push(audio[:, :cfg.audio_len]).shape[3] == T
    shape = (B, cfg.njoints, cfg.nfeats, T)
    origin_x = torch.zeros(shape, device=DEV)
    origin_x[..., :cfg.n_pre_seq] = y["seed_poses"]
    yy = {"audio_input": audio[:, :cfg.audio_len].contiguous(), "origin_x": origin_x, "vid_indices": y["vid_indices"], "scale": y["scale"]}
    s = diffusion.ddim_sample_loop(model, shape, clip_denoised=False, model_kwargs={"y": yy}, skip_timesteps=skip, init_image=None,
                                   progress=False, dump_steps=None, noise=None, const_noise=False)       # ls_prepare: the stream is over
    assert bool(torch.isfinite(s).all())
    with pytest.raises(_lib.EngineError, match="ended by a call that replaced"):
        st.push(audio[:, cfg.audio_len:cfg.audio_len + STRIDE])
    with pytest.raises(_lib.EngineError, match="ended by a call that replaced"):
        st.close()
    # the handle stays usable: sample_long on it gives the bits it gives on an engine that never streamed
    torch.manual_seed(53)
    after = _sample_long(parts, audio)
    fresh = _parts.__wrapped__("ted", "ddim")
    torch.manual_seed(53)
    assert torch.equal(after, _sample_long(fresh, audio))
    # ... and so does a new stream
    torch.manual_seed(53)
    outs, _ = _stream(parts, audio, _edge_chunks(cfg))
    assert torch.equal(torch.cat(outs, dim=3), after)


@pytest.mark.engine_path_auto
def test_contract_on_the_kernels_auto_picks_for_a_small_batch():
    """B = 3 under `auto` runs the sample-split kernel, whose hand-off tags advance per window and now across pushes.  A model of its
    own: the cached ones hold engines pinned to the fused kernel."""
    parts = _parts.__wrapped__("ted", "ddim")
    cfg = parts[0]
    audio = parts[5]["audio"][:, :_length(cfg)].contiguous()
    torch.manual_seed(59)
    want = _sample_long(parts, audio)
    for rep in range(2):
        torch.manual_seed(59)
        outs, _ = _stream(parts, audio, _edge_chunks(cfg))
        got = torch.cat(outs, dim=3)
        assert torch.equal(got, want), (rep, float((got - want).abs().max()))
    assert parts[1].model.engine().path == "auto"
