"""Live sessions fed at the microphone's rate (long_form.open_stream / open_pool with input_sr=): the chunks pass through the session's
audio_io.ResampleStream on the engine's device, so the frames are BIT FOR BIT those of a plain session fed ``audio_io.resample(whole,
input_sr)`` -- and so those of ``sample_long`` on it.  TED synthetic model, B = 2, 12 executed steps per window, 'philox'; 48 kHz int16
stereo in chunks of uneven sizes."""
import numpy as np
import pytest
import torch

from livelyspeaker_amd import audio_io, long_form
from test_gpu_long_stream import DEV, S, STRIDE, T, _parts

pytestmark = pytest.mark.gpu
B, SR = 2, 48000


def _mic(n16, rows, seed):
    """int16 stereo [rows, 3 * n16 - 1, 2] at 48 kHz: ceil(n / 3) = n16 samples at 16 kHz."""
    rng = np.random.default_rng(seed)
    return (8000 * rng.standard_normal((rows, 3 * n16 - 1, 2))).clip(-32768, 32767).astype(np.int16)


def _two(parts):
    cfg, model, diffusion, sampler, skip, y = parts
    return cfg, model, diffusion, sampler, skip, {k: v[:B].contiguous() for k, v in y.items()}


def _philox(diffusion, seed):
    diffusion.noise_source, diffusion.philox_seed = "philox", seed


def test_stream_at_48k_is_bitwise_the_stream_fed_the_resampled_audio():
    parts = _two(_parts("ted", "ddim"))
    cfg, model, diffusion, sampler, skip, y = parts
    L16 = cfg.audio_len + STRIDE - 5000                                   # two windows, the second zero-padded
    mic = _mic(L16, B, 11)
    whole, n16 = audio_io.resample(torch.from_numpy(mic).to(DEV), SR)
    assert n16.tolist() == [L16] * B and whole.shape == (B, L16)
    args = (diffusion, model, y["seed_poses"], y["vid_indices"], y["scale"])
    kw = dict(sampler=sampler, skip_timesteps=skip)
    _philox(diffusion, 0x5EED)
    try:
        want = long_form.sample_long(*args[:2], whole, *args[2:], **kw)
        assert want.shape[3] == T + S
        plain = long_form.open_stream(*args, **kw)                         # input_sr=None: the path as it was
        assert plain._in is None
        frames = [plain.push(whole[:, :30000]), plain.push(whole[:, 30000:]), plain.close()]
        assert torch.equal(torch.cat(frames, dim=3), want)
        for on_device in (True, False):
            st = long_form.open_stream(*args, input_sr=SR, input_channels=2, **kw)
            sizes = [50000, 1, 0, 60000, 65536]
            sizes.append(mic.shape[1] - sum(sizes))
            outs, pos = [], 0
            for n in sizes:
                chunk = mic[:, pos:pos + n]
                outs.append(st.push(torch.from_numpy(chunk.copy()).to(DEV) if on_device else chunk))
                pos += n
                assert st.input_samples_in == pos and st.samples_in == audio_io.resample_plan(SR, 16000, 0, pos)[1]
                if n == 1:                                                  # a refused push leaves the session and its resampler as they were
                    before = (st.input_samples_in, st.samples_in, st._in.samples_in.tolist(), st._in.info())
                    with pytest.raises(ValueError, match="BEAT conditioning"):
                        st.push(mic[:, pos:pos + 500], emo=torch.zeros(B, dtype=torch.long))
                    with pytest.raises(ValueError, match="channels"):
                        st.push(mic[:, pos:pos + 500, :1])
                    after = (st.input_samples_in, st.samples_in, st._in.samples_in.tolist(), st._in.info())
                    assert str(before) == str(after)
            with pytest.raises(ValueError, match="BEAT conditioning"):       # ... and so does a refused close: the tail is still owed
                st.close(emo=torch.zeros(B, dtype=torch.long))
            assert st._in.samples_in.tolist() == [pos] * B and st._in.info()["samples_in"].tolist() == [pos] * B and not st._closed
            outs.append(st.close())
            assert st.samples_in == L16 and st.windows_run == 2
            assert all(o.is_cuda == on_device for o in outs)
            got = torch.cat([o.to(DEV) for o in outs], dim=3)
            print(f"on_device={on_device}: max |48 kHz stream - sample_long| = {float((got - want).abs().max()):.3e}")
            assert torch.equal(got, want)
            with pytest.raises(RuntimeError):
                st.push(mic[:, :10])
    finally:
        diffusion.noise_source, diffusion.philox_seed = "torch_cpu", None


def _clip_alone(parts, audio16, i, key):
    """Clip i through a plain keyed pool of its own, fed 16 kHz audio in two chunks: its frames [J, F, k]."""
    cfg, model, diffusion, sampler, skip, y = parts
    pool = long_form.open_pool(diffusion, model, 2, sampler=sampler, skip_timesteps=skip, noise_keys="clip")
    assert pool._in is None and "input_samples_in" not in pool.slots
    slot = pool.join(y["seed_poses"][i], y["vid_indices"][i], y["scale"][i], key=key)
    n, got = audio16.shape[0], []
    for a, b in ((0, n // 3), (n // 3, n)):
        chunk = torch.zeros(2, b - a, device=DEV)
        chunk[slot] = audio16[a:b]
        frames, counts = pool.push(chunk, [b - a if s == slot else 0 for s in range(2)])
        got.append(frames[slot, :, :, :int(counts[slot])])
    got.append(pool.leave(slot))
    pool.close()
    return torch.cat(got, dim=2)


def test_pool_at_48k_with_a_slot_that_is_joined_again():
    parts = _two(_parts("ted", "ddim"))
    cfg, model, diffusion, sampler, skip, y = parts
    n16 = {"A": cfg.audio_len + 9000, "B": 20000, "C": 15000}            # A: two windows; B leaves early; C takes B's slot
    mics = {k: _mic(n, 1, 23 + i)[0] for i, (k, n) in enumerate(n16.items())}
    cond = {"A": 0, "B": 1, "C": 1}
    keys = {"A": 5, "B": 6, "C": 7}
    _philox(diffusion, 0xABCDEF)
    try:
        want = {}
        for k in n16:
            a16, n = audio_io.resample(torch.from_numpy(mics[k][None]).to(DEV), SR)
            assert n[0] == n16[k]
            want[k] = _clip_alone(parts, a16[0], cond[k], keys[k])
        assert want["A"].shape[2] == T + S and want["B"].shape[2] == T and want["C"].shape[2] == T
        pool = long_form.open_pool(diffusion, model, 2, sampler=sampler, skip_timesteps=skip, noise_keys="clip", input_sr=SR, input_channels=2)
        got, pos, who = {k: [] for k in n16}, {k: 0 for k in n16}, {}

        def join(k):
            i = cond[k]
            who[pool.join(y["seed_poses"][i], y["vid_indices"][i], y["scale"][i], key=keys[k])] = k

        def push(sizes):                                                    # {clip: frames at 48 kHz}
            lens = [sizes.get(who.get(s), 0) for s in range(2)]
            chunk = np.zeros((2, max(lens), 2), np.int16)
            for s in range(2):
                if lens[s]:
                    k = who[s]
                    chunk[s, :lens[s]] = mics[k][pos[k]:pos[k] + lens[s]]
                    pos[k] += lens[s]
            frames, counts = pool.push(torch.from_numpy(chunk).to(DEV), lens)
            for s in range(2):
                if counts[s]:
                    got[who[s]].append(frames[s, :, :, :int(counts[s])])

        join("A")
        push({"A": 40001})
        join("B")                                                           # joins at a later push
        push({"A": 65536, "B": 30000})
        assert pool.slots["input_samples_in"].tolist() == [105537, 30000]
        with pytest.raises(ValueError, match="given"):                      # a refused push: nothing reaches the resampler
            pool.push(np.zeros((2, 100, 2), np.int16), [100, 100], given=[True, True, False])
        with pytest.raises(ValueError, match="BEAT conditioning"):
            pool.push(np.zeros((2, 100, 2), np.int16), [100, 100], emo=torch.zeros(2, dtype=torch.long))
        assert pool.slots["input_samples_in"].tolist() == [105537, 30000] and pool._in.info()["samples_in"].tolist() == [105537, 30000]
        push({"B": mics["B"].shape[0] - 30000, "A": 7})
        slot_b = next(s for s, k in who.items() if k == "B")
        got["B"].append(pool.leave(slot_b))                                 # B leaves early: its resampler finishes first
        assert pool.slots["input_samples_in"][slot_b] == 0 and not pool.slots["open"][slot_b]
        join("C")                                                           # the same slot, a new clip: the resampler starts at sample 0
        assert who[slot_b] == "C"
        push({"A": 30000, "C": 20000})
        push({"A": mics["A"].shape[0] - pos["A"], "C": mics["C"].shape[0] - 20000})
        frames, counts = pool.close()
        for s in range(2):
            if counts[s]:
                got[who[s]].append(frames[s, :, :, :int(counts[s])])
        for k in n16:
            cat = torch.cat(got[k], dim=2)
            print(f"clip {k}: {cat.shape[2]} frames, max |pool at 48 kHz - clip alone| = {float((cat - want[k]).abs().max()):.3e}")
            assert torch.equal(cat, want[k]), k
    finally:
        diffusion.noise_source, diffusion.philox_seed = "torch_cpu", None
