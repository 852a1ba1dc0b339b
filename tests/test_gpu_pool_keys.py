"""The keyed session pool on the GPU (``long_form.open_pool(noise_keys='clip')`` -> ls_long_pool_keyed / ls_long_pool_set_key, the key
table of ls_long_pool_keys, the draws of csrc/ls_philox_rows.hip).

The contract: the clip in a slot draws in its own window w at ``key + (w << 48)``, so its frames do not depend on the other slots, the
slot index, the chunking or the pool's age; every round is the public sampling call at its batch with ``row_keys`` = the round's
rows of the key table, and a pool joined in order with default keys is ``sample_long`` at ``sample_offset`` = the first key -- all bit
for bit.  The shapes of tests/test_gpu_long_pool.py: capacity 4, 12 executed steps per window, both datasets, synthetic weights."""
import functools

import numpy as np
import pytest
import torch

from livelyspeaker_amd import _lib, long_form
from test_gpu_long_pool import CAP, SPEAKERS, _log, _speakers
from test_gpu_long_stream import B, DEV, S, STRIDE, T, _edge_chunks, _emo, _length, _parts, _sample_long
from test_long_pool_host import staggered

pytestmark = pytest.mark.gpu
SEED = 0xC11B_5EED_2026
KEYS = {"A": 11, "B": (1 << 32) + 5, "C": (1 << 48) - 1, "D": 3}       # B above 2^32, C the largest key


class _philox:
    def __init__(self, diffusion, offset=0):
        self.d, self.offset = diffusion, offset

    def __enter__(self):
        self.d.noise_source, self.d.philox_seed, self.d.sample_offset = "philox", SEED, self.offset

    def __exit__(self, *exc):
        self.d.noise_source, self.d.philox_seed, self.d.sample_offset = "torch_cpu", None, 0
        return False


def _join(pool, y, name, slot=None, key=None):
    i = SPEAKERS[name]
    emo = {"emo": y["emo"][i, 0]} if "emo" in y else {}
    return pool.join(y["seed_poses"][i], y["vid_indices"][i], y["scale"][i], slot=slot, **({} if key is None else {"key": key}), **emo)


def _run(parts, y, events, keys, noise_keys="clip"):
    """(event, payload) pairs through a pool -- ("join", (speaker, slot)), ("push", {speaker: samples}), ("leave", speaker), ("close",
    None) -- : every speaker's frames, one tensor per stay in the pool, and the pool.  ``keys``: speaker -> key, or None for the defaults."""
    cfg, model, diffusion, sampler, skip, _ = parts
    pool = long_form.open_pool(diffusion, model, CAP, sampler=sampler, skip_timesteps=skip, noise_keys=noise_keys)
    who, fed, got = {}, {}, {}

    def take(out, counts):
        for s in range(CAP):
            if counts[s]:
                got[who[s]][-1].append(out[s, :, :, :int(counts[s])])

    for event, payload in events:
        if event == "join":
            name, slot = payload
            s = _join(pool, y, name, slot, None if keys is None or noise_keys is None else keys[name])
            who[s], fed[name] = name, 0
            got.setdefault(name, []).append([])
            if noise_keys is not None and keys is not None:
                assert int(pool.slots["key"][s]) == keys[name]
        elif event == "push":
            lengths = [payload.get(who.get(s), 0) if pool.slots["open"][s] else 0 for s in range(CAP)]
            audio = torch.zeros(CAP, max(lengths), device=DEV)
            for s, n in enumerate(lengths):
                if n:
                    audio[s, :n] = y["audio"][SPEAKERS[who[s]], fed[who[s]]:fed[who[s]] + n]
                    fed[who[s]] += n
            take(*pool.push(audio, lengths))
        elif event == "leave":
            slot = next(s for s, k in who.items() if k == payload and pool.slots["open"][s])
            tail = pool.leave(slot)
            if tail.shape[2]:
                got[payload][-1].append(tail)
        else:
            take(*pool.close())
    J, F = cfg.njoints, cfg.nfeats
    return {k: [torch.cat(v, dim=2) if v else torch.zeros(J, F, 0, device=DEV) for v in stays] for k, stays in got.items()}, pool


def _staggered_events(AL):
    """tests/test_long_pool_host.py's schedule in ``_run``'s events: rounds at batch 1, 3, 1, 1, 2."""
    who, events = {}, []
    slots = {"A": 0, "B": 1, "C": 3, "D": 1}
    for event, payload in staggered(AL):
        if event == "join":
            who[slots[payload[0]]] = payload[0]
            events.append(("join", payload))
        elif event == "push":
            events.append(("push", {who[s]: n for s, n in enumerate(payload[0]) if n}))
        elif event == "leave":
            events.append(("leave", payload[0]))
        else:
            events.append(("close", None))
    return events


@functools.lru_cache(maxsize=None)
def _public_calls(ds, schedule):
    """One public sampling call per logged round of the staggered schedule, at its batch, like ``_oracle`` of
    tests/test_gpu_long_pool.py -- with ``row_keys = key[speaker] + (window << 48)``."""
    parts, y = _parts(ds, schedule), _speakers(ds)
    cfg, model, diffusion, sampler, skip, _ = parts
    loop = diffusion.ddim_sample_loop if sampler == "ddim" else diffusion.p_sample_loop
    last, frames = {}, {k: [] for k in SPEAKERS}
    with _philox(diffusion):
        for rows in _log(cfg.audio_len):
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
            diffusion.row_keys = [KEYS[k] + (w << 48) for k, w, _ in rows]
            try:
                x = loop(model, shape, clip_denoised=False, model_kwargs={"y": yy}, skip_timesteps=skip, init_image=None, progress=False,
                         dump_steps=None, noise=None, const_noise=False).contiguous()
            finally:
                diffusion.row_keys = None
            for i, (k, w, _) in enumerate(rows):
                last[k] = x[i]
                frames[k].append(x[i] if w == 0 else x[i, :, :, cfg.n_pre_seq:])
    return {k: torch.cat(v, dim=2) for k, v in frames.items()}


@pytest.mark.parametrize("schedule", ["ddim", "ddpm"])
@pytest.mark.parametrize("ds", ["ted", "beat"])
def test_keyed_pool_is_bitwise_the_loop_of_keyed_public_calls(ds, schedule):
    parts, y = _parts(ds, schedule), _speakers(ds)
    want = _public_calls(ds, schedule)
    with _philox(parts[2]):
        got, pool = _run(parts, y, _staggered_events(parts[0].audio_len), KEYS)
    assert pool.slots["key"].tolist() == [KEYS["A"], KEYS["D"], 0, KEYS["C"]]
    assert [int(got[k][0].shape[2]) for k in "ABCD"] == [T + S, T + S, T + 2 * S, T]
    for k in "ABCD":
        d = float((got[k][0] - want[k]).abs().max())
        print(f"{ds} {schedule} speaker {k} (key {KEYS[k]}): max |keyed pool - keyed public calls| = {d:.3e}")
        assert bool(torch.isfinite(got[k][0]).all()) and torch.equal(got[k][0], want[k]), (k, d)


@pytest.mark.parametrize("ds", ["ted", "beat"])
def test_in_lockstep_with_default_keys_it_is_sample_long(ds):
    """Three slots joined in order (default keys o, o + 1, o + 2) and fed alike in uneven chunks, against ``sample_long`` on the
    concatenated audio at ``sample_offset = o`` under the same seed."""
    parts = _parts(ds, "ddim")
    cfg, model, diffusion, sampler, skip, y = parts
    audio = y["audio"][:, :_length(cfg)].contiguous()
    emo = None if _emo(parts) is None else _emo(parts)[:, 0].contiguous()
    o = 9
    with _philox(diffusion, offset=o):
        want = _sample_long(parts, audio, emo=emo)
        pool = long_form.open_pool(diffusion, model, CAP, sampler=sampler, skip_timesteps=skip, noise_keys="clip")
        for b in range(B):
            assert pool.join(y["seed_poses"][b], y["vid_indices"][b], y["scale"][b], emo=None if emo is None else emo[b]) == b
        assert pool.slots["key"].tolist() == [o, o + 1, o + 2, 0]
        outs, pos = [], 0
        for n in _edge_chunks(cfg):
            chunk = audio.new_zeros(CAP, n)
            chunk[:B] = audio[:, pos:pos + n]
            frames, counts = pool.push(chunk, [n] * B + [0])
            outs.append(frames[:B])
            pos += n
        outs.append(pool.close()[0][:B])
    assert [int(o_.shape[3]) for o_ in outs] == [0, T, 0, S, 0, S]
    got = torch.cat(outs, dim=3)
    print(f"{ds}: max |keyed pool in lockstep - sample_long| = {float((got - want).abs().max()):.3e}")
    assert torch.equal(got, want), float((got - want).abs().max())


def _xy(parts, y, noise_keys, crowded):
    """Speakers A and C for two windows each, at batch 2: alone in slots 0, 1 of a fresh pool, or in slots 1, 2 of a pool whose slot 0
    holds D, who has run two windows alone and gets no sample afterwards."""
    AL = parts[0].audio_len
    feed = ("push", {"A": AL + STRIDE, "C": AL + STRIDE})
    if crowded:
        events = [("join", ("D", 0)), ("push", {"D": AL + STRIDE}), ("join", ("A", 1)), ("join", ("C", 2)), feed, ("close", None)]
    else:
        events = [("join", ("A", 0)), ("join", ("C", 1)), feed, ("close", None)]
    got, pool = _run(parts, y, events, KEYS, noise_keys)
    assert pool.slots["windows_run"].tolist() == ([2, 2, 2, 0] if crowded else [2, 2, 0, 0])
    assert parts[1].model.engine().long_pool_info()["rounds"] == (4 if crowded else 2)      # the pool's age differs
    return got["A"][0], got["C"][0]


@pytest.mark.parametrize("ds", ["ted", "beat"])
def test_frames_do_not_depend_on_the_schedule(ds):
    parts, y = _parts(ds, "ddim"), _speakers(ds)
    with _philox(parts[2]):
        alone, crowded = _xy(parts, y, "clip", False), _xy(parts, y, "clip", True)
        plain = _xy(parts, y, None, False), _xy(parts, y, None, True)
    for i, k in enumerate("AC"):
        assert alone[i].shape[2] == T + S and bool(torch.isfinite(alone[i]).all())
        assert torch.equal(alone[i], crowded[i]), (k, float((alone[i] - crowded[i]).abs().max()))
        # ... which the pool's own round index does not give: the same two runs without keys differ, and differ from the keyed ones
        assert not torch.equal(plain[0][i], plain[1][i]) and not torch.equal(plain[0][i], alone[i]), k


@pytest.mark.parametrize("ds", ["ted", "beat"])
def test_a_clip_that_joins_again_under_its_key_repeats_itself(ds):
    parts, y = _parts(ds, "ddim"), _speakers(ds)
    AL = parts[0].audio_len
    events = [("join", ("A", 0)), ("push", {"A": AL + STRIDE}), ("leave", "A"),
              ("join", ("B", 0)), ("push", {"B": AL}), ("leave", "B"),             # someone else in between: another speaker, scale and key
              ("join", ("A", 0)), ("push", {"A": AL}), ("push", {"A": STRIDE}), ("close", None)]
    with _philox(parts[2]):
        got, pool = _run(parts, y, events, KEYS)
    first, again = got["A"]
    assert first.shape[2] == T + S and got["B"][0].shape[2] == T
    assert torch.equal(first, again), float((first - again).abs().max())
    assert not torch.equal(first[..., :T], got["B"][0])


def test_engine_refusals():
    parts, y = _parts("ted", "ddim"), _speakers("ted")
    cfg, model, diffusion, sampler, skip, _ = parts
    AL = cfg.audio_len
    with _philox(diffusion):
        pool = long_form.open_pool(diffusion, model, CAP, sampler=sampler, skip_timesteps=skip, noise_keys="clip")
        assert _join(pool, y, "A") == 0 and _join(pool, y, "B", key=77) == 1
        assert pool.slots["key"].tolist() == [0, 77, 0, 0]
        eng = model.model.engine()
        with pytest.raises(_lib.EngineError, match="first join"):
            eng.long_pool_keyed(False)
        with pytest.raises(_lib.EngineError, match="2\\^48"):
            eng.long_pool_set_key(0, 1 << 48)
        with pytest.raises(_lib.EngineError, match="not open"):
            eng.long_pool_set_key(2, 5)
        pool.push(y["audio"][:, :AL].contiguous(), [AL, 0, 0, 0])
        with pytest.raises(_lib.EngineError, match="has run a window"):
            eng.long_pool_set_key(0, 5)
        eng.long_pool_set_key(1, 78)                            # slot 1 has not run a window yet
        plain = long_form.open_pool(diffusion, model, CAP, sampler=sampler, skip_timesteps=skip)
        _join(plain, y, "A")
        with pytest.raises(_lib.EngineError, match="not keyed"):
            eng.long_pool_set_key(0, 5)
        # row keys of a sampling call: a count that is not the batch, and a noise mode that is not PHILOX
        eng.prepare({k: v for k, v in _one_call(cfg).items()})
        with pytest.raises(_lib.EngineError, match="row keys"):
            eng.sample(sampler=_lib.LS_SAMPLER_DDIM, philox_seed=1, skip_timesteps=skip, row_keys=[1, 2, 3])
        with pytest.raises(_lib.EngineError, match="sample_offset"):
            eng.sample(sampler=_lib.LS_SAMPLER_DDIM, philox_seed=1, sample_offset=4, skip_timesteps=skip, row_keys=[1, 2])
        with pytest.raises(_lib.EngineError, match="PLMS"):
            eng.sample(sampler=_lib.LS_SAMPLER_PLMS, plms_order=2, philox_seed=1, skip_timesteps=skip, row_keys=[1, 2])
        out = eng.sample(sampler=_lib.LS_SAMPLER_DDIM, philox_seed=1, skip_timesteps=skip, row_keys=[1, 2])
        assert np.array_equal(out, eng.sample(sampler=_lib.LS_SAMPLER_DDIM, philox_seed=1, sample_offset=1, skip_timesteps=skip))


def _one_call(cfg):
    from livelyspeaker_amd import synth
    return synth.make_cond(cfg, 2)
