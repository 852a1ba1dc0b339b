"""The session pool on the GPU (long_form.open_pool -> ls_long_pool_open / _join / _push, k_pool_gather / k_pool_scatter in csrc/ls_chain.hip).

The contract: every round of ``pool_plan`` is one public sampling call at its batch on the active slots' windows, and a pool that is
used like a stream is that stream, bit for bit.  Capacity 4, 12 executed steps per window (1000 steps respaced to 100, skip 88), both
datasets, synthetic weights.  The staggered schedule (tests/test_long_pool_host.py) runs rounds at batch 1, 3, 1, 1, 2: speakers that
join late, leave early, a reused slot, a gap in the slots, non-contiguous active slots, and a speaker with scale 1 beside others at 1.5."""
import functools

import numpy as np
import pytest
import torch

from livelyspeaker_amd import _lib, long_form, synth
from livelyspeaker_amd.motionclip_module import Decoder_TRANSFORMER
from test_gpu_long_stream import B, DEV, S, STRIDE, T, W, _edge_chunks, _emo, _length, _parts, _sample_long, _stream
from test_long_pool_host import HostPool, staggered

pytestmark = pytest.mark.gpu
CAP = 4
SPEAKERS = {"A": 0, "B": 1, "C": 2, "D": 3}


@functools.lru_cache(maxsize=None)
def _speakers(ds):
    """Four speakers' conditioning and audio; B talks at scale 1, the others at 1.5: the single-pass decision differs between rounds."""
    cfg = synth.CONFIGS[ds]
    y = {k: torch.from_numpy(v).to(DEV) for k, v in synth.make_long_cond(cfg, 4, 4, seed=synth.SEED_COND + 4100).items()}
    y["scale"] = torch.tensor([1.5, 1.0, 1.5, 1.5], device=DEV)
    return y


def _join(pool, y, name, slot=None):
    i = SPEAKERS[name]
    emo = {"emo": y["emo"][i, 0]} if "emo" in y else {}
    return pool.join(y["seed_poses"][i], y["vid_indices"][i], y["scale"][i], slot=slot, **emo)


def _run_staggered(parts, y, seen=None):
    """The staggered schedule through a pool: every speaker's concatenated frames."""
    cfg, model, diffusion, sampler, skip, _ = parts
    pool = long_form.open_pool(diffusion, model, CAP, sampler=sampler, skip_timesteps=skip)
    who, fed = {}, {k: 0 for k in SPEAKERS}                 # slot -> speaker; samples fed per speaker
    got = {k: [] for k in SPEAKERS}

    def call(lengths, closing):
        st = pool.slots
        rounds, frames = long_form.pool_plan(st["samples_in"], st["windows_run"], lengths, closing, st["open"], cfg)
        audio = torch.zeros(CAP, max(lengths), device=DEV)
        for s, n in enumerate(lengths):
            if n:
                audio[s, :n] = y["audio"][SPEAKERS[who[s]], fed[who[s]]:fed[who[s]] + n]
                fed[who[s]] += n
        return rounds, frames, audio

    for event, payload in staggered(cfg.audio_len):
        if event == "join":
            s = _join(pool, y, *payload)
            who[s] = payload[0]
            continue
        if event == "push":
            rounds, frames, audio = call(payload[0], [0] * CAP)
            assert rounds == payload[1]
            out, counts = pool.push(audio, payload[0])
        elif event == "leave":
            slot = next(s for s, k in who.items() if k == payload[0] and pool.slots["open"][s])
            rounds, frames, _ = call([0] * CAP, [int(s == slot) for s in range(CAP)])
            tail = pool.leave(slot)
            out, counts = torch.zeros((CAP,) + tuple(tail.shape), device=DEV), np.zeros(CAP, np.int32)
            out[slot], counts[slot] = tail, tail.shape[2]
            assert not pool.slots["open"][slot]
        else:
            rounds, frames, _ = call([0] * CAP, [int(o) for o in pool.slots["open"]])
            out, counts = pool.close()
        assert counts.tolist() == frames.tolist() and out.shape == (CAP, cfg.njoints, cfg.nfeats, int(frames.max()))
        for s in range(CAP):
            assert not bool(out[s, :, :, int(counts[s]):].any())        # zero behind a slot's own frames
            if counts[s]:
                got[who[s]].append(out[s, :, :, :int(counts[s])])
        if seen is not None:
            seen(event, rounds, model.model.engine())
    return {k: torch.cat(v, dim=2) for k, v in got.items()}


def _log(AL):
    """The schedule's rounds from the host plan alone: per round, in order, its (speaker, window, samples that speaker has been fed) rows."""
    pool, who, fed, log = HostPool(CAP, AL), {}, {k: 0 for k in SPEAKERS}, []
    for event, payload in staggered(AL):
        if event == "join":
            who[pool.join(payload[1])] = payload[0]
            continue
        lengths = payload[0] if event == "push" else [0] * CAP
        closing = [int(event == "close" or (event == "leave" and who.get(s) == payload[0])) * int(pool.open[s]) for s in range(CAP)]
        before = pool.ran.copy()
        for s, n in enumerate(lengths):
            if n:
                fed[who[s]] += n
        rounds, _ = pool.push(lengths, closing)
        for r, slots in enumerate(rounds):
            log.append([(who[s], int(before[s]) + r, fed[who[s]]) for s in slots])
    return log


@functools.lru_cache(maxsize=None)
def _oracle(ds, schedule, seed, log=None):
    """One public sampling call per logged round, at its batch: the active slots' windows (zero-padded behind a speaker's last sample),
    their previous result's last four frames (or seed poses) as the origin_x prefix, their speaker ids, scales and (BEAT) emotion ids.
    ``log``: the rounds as a tuple of tuples of rows (default: the staggered schedule's).  Under ``'philox'`` round q draws at the
    pool's key: ``sample_offset = q << 48``."""
    parts, y = _parts(ds, schedule), _speakers(ds)
    cfg, model, diffusion, sampler, skip, _ = parts
    log = _log(cfg.audio_len) if log is None else log
    loop = diffusion.ddim_sample_loop if sampler == "ddim" else diffusion.p_sample_loop
    last, frames = {}, {k: [] for k in SPEAKERS}
    torch.manual_seed(seed)
    for q, rows in enumerate(log):
        diffusion.sample_offset = q << 48
        idx = torch.tensor([SPEAKERS[k] for k, _, _ in rows], device=DEV)
        shape = (len(rows), cfg.njoints, cfg.nfeats, T)
        origin_x = torch.zeros(shape, device=DEV)
        audio = torch.zeros(len(rows), cfg.audio_len, device=DEV)
        for i, (k, w, n) in enumerate(rows):
            origin_x[i, :, :, :cfg.n_pre_seq] = last[k][..., T - cfg.n_pre_seq:] if w else y["seed_poses"][SPEAKERS[k]]
            audio[i] = long_form.window_audio(y["audio"][SPEAKERS[k]:SPEAKERS[k] + 1, :n], w, cfg)[0]
        yy = {"audio_input": audio, "origin_x": origin_x, "vid_indices": y["vid_indices"][idx].contiguous(), "scale": y["scale"][idx].contiguous()}
        if "emo" in y:
            yy["emo"] = y["emo"][idx, 0:1].expand(len(rows), T).contiguous()
        x = loop(model, shape, clip_denoised=False, model_kwargs={"y": yy}, skip_timesteps=skip, init_image=None, progress=False,
                 dump_steps=None, noise=None, const_noise=False).contiguous()
        for i, (k, w, _) in enumerate(rows):
            last[k] = x[i]
            frames[k].append(x[i] if w == 0 else x[i, :, :, cfg.n_pre_seq:])
    diffusion.sample_offset = 0
    return {k: torch.cat(v, dim=2) for k, v in frames.items() if v}, [len(r) for r in log]


@pytest.mark.parametrize("schedule", ["ddim", "ddpm"])
@pytest.mark.parametrize("ds", ["ted", "beat"])
def test_staggered_schedule_is_bitwise_the_loop_of_public_calls(ds, schedule):
    parts, y = _parts(ds, schedule), _speakers(ds)
    want, batches = _oracle(ds, schedule, 61)
    assert batches == [1, 3, 1, 1, 2]
    torch.manual_seed(61)
    got = _run_staggered(parts, y)
    assert [int(got[k].shape[2]) for k in "ABCD"] == [T + S, T + S, T + 2 * S, T]
    for k in "ABCD":
        print(f"{ds} {schedule} speaker {k}: max |pool - public loops| = {float((got[k] - want[k]).abs().max()):.3e}")
        assert bool(torch.isfinite(got[k]).all()) and torch.equal(got[k], want[k]), (k, float((got[k] - want[k]).abs().max()))


def _pool_as_stream(parts, audio, sizes, emo=None, sag=None, text=None):
    """Three slots joined in order and fed the same chunk sizes, then closed: ``_stream``'s calls through a pool of four."""
    cfg, model, diffusion, sampler, skip, y = parts
    host = not audio.is_cuda if torch.is_tensor(audio) else True
    audio = torch.as_tensor(audio)
    pool = long_form.open_pool(diffusion, model, CAP, sampler=sampler, skip_timesteps=skip, sag=sag)
    for b in range(B):
        assert pool.join(y["seed_poses"][b], y["vid_indices"][b], y["scale"][b], emo=None if emo is None else emo[b]) == b

    def held():
        w = int(pool.slots["windows_run"][0])
        if text is None or w >= text.shape[1]:
            return {}
        return {"text_features": torch.cat([text[:, w], text.new_zeros(CAP - B, 512)])}

    outs, pos = [], 0
    for n in sizes:
        chunk = audio.new_zeros(CAP, n)
        chunk[:B] = audio[:, pos:pos + n]
        frames, counts = pool.push(chunk, [n] * B + [0] * (CAP - B), **held())
        assert counts[:B].tolist() == [frames.shape[3]] * B and counts[B:].tolist() == [0] * (CAP - B) and frames.is_cuda != host
        outs.append(frames[:B])
        pos += n
    if held():
        pool.push(audio.new_zeros(CAP, 0), [0] * CAP, **held())      # the close takes no conditioning: hold the last window's first
    frames, counts = pool.close()
    outs.append(frames[:B])
    assert pool.slots["samples_in"].tolist() == [audio.shape[1]] * B + [0] and not pool.slots["open"].any()
    return outs, pool


@pytest.mark.parametrize("noise", ["torch_cpu", "philox"])
@pytest.mark.parametrize("ds", ["ted", "beat"])
def test_used_like_a_stream_it_is_a_stream(ds, noise):
    parts = _parts(ds, "ddim")
    cfg, diffusion = parts[0], parts[2]
    audio = parts[5]["audio"][:, :_length(cfg)].contiguous()
    emo = None if _emo(parts) is None else _emo(parts)[:, 0].contiguous()
    if noise == "philox":
        diffusion.noise_source, diffusion.philox_seed = "philox", 0x1357_2468_ACE0
    try:
        torch.manual_seed(67)
        want = torch.cat(_stream(parts, audio, _edge_chunks(cfg), emo=emo)[0], dim=3)
        if ds == "ted":
            torch.manual_seed(67)
            assert torch.equal(want, _sample_long(parts, audio, emo=emo))
        torch.manual_seed(67)
        outs, _ = _pool_as_stream(parts, audio, _edge_chunks(cfg), emo=emo)
    finally:
        diffusion.noise_source, diffusion.philox_seed = "torch_cpu", None
    assert [int(o.shape[3]) for o in outs] == [0, T, 0, S, 0, S]
    got = torch.cat(outs, dim=3)
    assert torch.equal(got, want), float((got - want).abs().max())


def test_sag_chain_is_bitwise_the_stream():
    parts = _parts("ted", "ddim")
    cfg = parts[0]
    sag = Decoder_TRANSFORMER(njoints=cfg.njoints, nfeats=cfg.nfeats, latent_dim=512, n_pre_poses=4, use_style=False)
    sag.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_sag_state_dict(cfg).items()}, strict=False)
    sag.to(DEV).eval()
    text = torch.from_numpy(synth.make_text_features(B * W).reshape(B, W, 512)).to(DEV)
    audio = parts[5]["audio"][:, :_length(cfg)].contiguous()
    torch.manual_seed(71)
    want = torch.cat(_stream(parts, audio, _edge_chunks(cfg), sag=sag, text=text)[0], dim=3)
    torch.manual_seed(71)
    plain = torch.cat(_stream(parts, audio, _edge_chunks(cfg))[0], dim=3)
    assert not torch.equal(plain, want)                     # the decoder's init_image matters
    torch.manual_seed(71)
    outs, _ = _pool_as_stream(parts, audio, _edge_chunks(cfg), sag=sag, text=text)
    got = torch.cat(outs, dim=3)
    assert torch.equal(got, want), float((got - want).abs().max())


def test_philox_is_keyed_by_the_pool():
    parts, y = _parts("ted", "ddim"), _speakers("ted")
    diffusion = parts[2]
    diffusion.noise_source, diffusion.philox_seed = "philox", 0xFEED_5EED
    try:
        first = _run_staggered(parts, y)
        again = _run_staggered(parts, y)
        diffusion.philox_seed = 99
        other = _run_staggered(parts, y)
    finally:
        diffusion.noise_source, diffusion.philox_seed = "torch_cpu", None
    for k in "ABCD":
        assert bool(torch.isfinite(first[k]).all()) and torch.equal(first[k], again[k]) and not torch.equal(first[k], other[k]), k


def test_memory_is_bounded_and_a_batch_met_before_is_replayed():
    """Rounds at batch 1, 3, 1, 1, 2 on one set of buffers: a stale address in a kept graph would show as wrong bits or a fault."""
    parts, y = _parts("ted", "ddim"), _speakers("ted")
    cfg, diffusion = parts[0], parts[2]
    seen = []

    def note(event, rounds, eng):
        if event in ("push", "leave"):
            seen.append(([len(r) for r in rounds], eng.long_pool_info()["device_bytes"], eng.timing()["graph_replayed"], eng.timing()["n_segments"]))

    want, _ = _oracle("ted", "ddim", 61)
    torch.manual_seed(61)
    got = _run_staggered(parts, y, seen=note)
    for k in "ABCD":
        assert torch.equal(got[k], want[k]), k
    assert [s[0] for s in seen] == [[1], [3, 1], [1], [2]] and [s[3] for s in seen] == [1, 2, 1, 1]
    assert seen[0][1] == seen[-1][1] > 0                    # the bytes the pool holds after the first and after the last push
    ring = (cfg.audio_len + STRIDE + 3) // 4 * 4
    assert seen[0][1] >= CAP * (ring + cfg.audio_len + T * 256) * 4
    if diffusion.use_graph:
        assert [s[2] for s in seen] == [0, 1, 0, 0]         # {C} replays {A}'s loop; {B} alone (scale 1) runs the single-pass form: another loop


def test_state_and_refusals():
    parts, y = _parts("ted", "ddim"), _speakers("ted")
    cfg, model, diffusion, sampler, skip, y3 = parts
    AL = cfg.audio_len
    pool = long_form.open_pool(diffusion, model, CAP, sampler=sampler, skip_timesteps=skip)
    assert _join(pool, y, "A") == 0
    with pytest.raises(ValueError, match="occupied"):
        _join(pool, y, "B", slot=0)
    with pytest.raises(_lib.EngineError, match="occupied"):
        model.model.engine().long_pool_join(0, y["seed_poses"][1], y["vid_indices"][1:2], y["scale"][1:2])
    with pytest.raises(ValueError):
        pool.push(torch.zeros(CAP, 10, device=DEV), [0, 10, 0, 0])      # samples for a free slot
    torch.manual_seed(73)
    frames, counts = pool.push(y["audio"][:, :AL].contiguous(), [AL, 0, 0, 0])
    assert counts.tolist() == [T, 0, 0, 0] and bool(torch.isfinite(frames).all())
    # a plain sampling call ends the pool; the handle stays usable
    audio = y3["audio"][:, :_length(cfg)].contiguous()
    torch.manual_seed(79)
    after = _sample_long(parts, audio)
    with pytest.raises(_lib.EngineError, match="ended by a call that replaced"):
        pool.push(torch.zeros(CAP, 10, device=DEV), [10, 0, 0, 0])
    with pytest.raises(_lib.EngineError, match="ended by a call that replaced"):
        _join(pool, y, "B")
    torch.manual_seed(79)
    outs, _ = _pool_as_stream(parts, audio, [audio.shape[1]])
    assert torch.equal(torch.cat(outs, dim=3), after)
    # BEAT joins need emo; 'torch_device' is refused
    beat = _parts("beat", "ddim")
    yb = _speakers("beat")
    with pytest.raises(ValueError, match="emo"):
        long_form.open_pool(beat[2], beat[1], CAP, sampler="ddim", skip_timesteps=beat[4]).join(yb["seed_poses"][0], yb["vid_indices"][0], 1.5)
    diffusion.noise_source = "torch_device"
    try:
        with pytest.raises(NotImplementedError):
            long_form.open_pool(diffusion, model, CAP)
    finally:
        diffusion.noise_source = "torch_cpu"
    # host inputs give host outputs with the same bits
    host = parts[:5] + ({k: v.cpu() for k, v in y3.items()},)
    short = y3["audio"][:, :20000].contiguous()
    torch.manual_seed(83)
    dev_outs, _ = _pool_as_stream(parts, short, [5000, 0, 15000])
    torch.manual_seed(83)
    host_outs, _ = _pool_as_stream(host, short.cpu().numpy(), [5000, 0, 15000])
    assert [int(o.shape[3]) for o in host_outs] == [0, 0, 0, T] and all(not o.is_cuda for o in host_outs)
    assert torch.equal(host_outs[-1], dev_outs[-1].cpu())


@pytest.mark.engine_path_auto
def test_contract_on_the_kernels_auto_picks_for_small_batches():
    """Batches 1 .. 3 under `auto` run the sample-split kernel, whose hand-off tags advance per round and across pushes.  A model of
    its own: the cached ones hold engines pinned to the fused kernel."""
    parts = _parts.__wrapped__("ted", "ddim")
    cfg = parts[0]
    audio = parts[5]["audio"][:, :_length(cfg)].contiguous()
    torch.manual_seed(89)
    want = torch.cat(_stream(parts, audio, _edge_chunks(cfg))[0], dim=3)
    for rep in range(2):
        torch.manual_seed(89)
        outs, _ = _pool_as_stream(parts, audio, _edge_chunks(cfg))
        got = torch.cat(outs, dim=3)
        assert torch.equal(got, want), (rep, float((got - want).abs().max()))
    assert parts[1].model.engine().path == "auto"
