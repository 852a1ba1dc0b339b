"""Pinned poses for frames a session has yet to make, on the GPU (long_form.open_pool(pins=H) / LongPool.pin -> ls_long_pool_pins /
_pin / _unpin, k_pool_pin_store / k_pool_pin_clear / k_pool_pin_gather in csrc/ls_chain.hip).

The contract: every call of ``pool_pin_plan`` is one public sampling call at its batch -- a pinned call with ``inpainting_mask`` true
exactly on the pinned elements of the frames its window owns and ``inpainted_motion`` the pinned values there -- and a pool that is
never pinned is the pool it was.  Capacity 4, 12 executed steps per window (1000 steps respaced to 100, skip 88), both datasets,
synthetic weights, horizon 64 (the ring holds 64 frames, so frame 67 sits where frame 3 sat)."""
import numpy as np
import pytest
import torch

from livelyspeaker_amd import _lib, long_form
from test_gpu_long_pool import CAP, SPEAKERS, _join, _speakers
from test_gpu_long_stream import B, DEV, S, STRIDE, T, _edge_chunks, _emo, _length, _parts
from test_long_pool_host import HostPool, staggered
from test_long_pool_pins_host import EXPECTED_CALLS, HORIZON, owned, pinned_schedule

pytestmark = pytest.mark.gpu


def _target(cfg, speaker, frames, kind):
    """The poses [J, F, K] a pin event asks for and its mask (None: the whole pose; 'feature': one feature of one joint)."""
    g = torch.Generator().manual_seed(7000 + 131 * SPEAKERS[speaker] + int(frames[0]))
    poses = (torch.rand(cfg.njoints, cfg.nfeats, len(frames), generator=g) * 2 - 1).to(DEV)
    if kind == "pose":
        return poses, None
    mask = torch.zeros(cfg.njoints, cfg.nfeats, len(frames), dtype=torch.bool, device=DEV)
    mask[cfg.njoints // 2, cfg.nfeats - 1, :] = True
    return poses, mask


def _run(parts, y, events, pins=HORIZON, noise_keys=None, keys=None, seen=None):
    """The events through a pool: every speaker's concatenated frames.  ``pin`` / ``unpin`` events name a speaker."""
    cfg, model, diffusion, sampler, skip, _ = parts
    pool = long_form.open_pool(diffusion, model, CAP, sampler=sampler, skip_timesteps=skip, pins=pins, noise_keys=noise_keys)
    who, fed, got = {}, {k: 0 for k in SPEAKERS}, {k: [] for k in SPEAKERS}
    slot_of = lambda name: next(s for s, k in who.items() if k == name and pool.slots["open"][s])      # noqa: E731

    def audio_for(lengths):
        audio = torch.zeros(CAP, max(lengths), device=DEV)
        for s, n in enumerate(lengths):
            if n:
                audio[s, :n] = y["audio"][SPEAKERS[who[s]], fed[who[s]]:fed[who[s]] + n]
                fed[who[s]] += n
        return audio

    for event, payload in events:
        if event == "join":
            i = SPEAKERS[payload[0]]
            kw = {"emo": y["emo"][i, 0]} if "emo" in y else {}
            if keys is not None:
                kw["key"] = keys[payload[0]]
            s = pool.join(y["seed_poses"][i], y["vid_indices"][i], y["scale"][i], slot=payload[1], **kw)
            who[s] = payload[0]
            assert pins is None or pool.slots["pins"][s] == 0          # a join starts with no pin
            continue
        if event == "pin":
            poses, mask = _target(cfg, *payload)
            pool.pin(slot_of(payload[0]), payload[1], poses, mask)
            continue
        if event == "unpin":
            pool.unpin(slot_of(payload[0]), payload[1])
            continue
        if event == "push":
            out, counts = pool.push(audio_for(payload[0]), payload[0])
        elif event == "leave":
            slot = slot_of(payload[0])
            tail = pool.leave(slot)
            out, counts = torch.zeros((CAP,) + tuple(tail.shape), device=DEV), np.zeros(CAP, np.int32)
            out[slot], counts[slot] = tail, tail.shape[2]
            assert pins is None or pool.slots["pins"][slot] == 0       # leaving drops the pins the clip never reached
        else:
            out, counts = pool.close()
        for s in range(CAP):
            if counts[s]:
                got[who[s]].append(out[s, :, :, :int(counts[s])])
        if seen is not None:
            seen(event, pool)
    return {k: torch.cat(v, dim=2) for k, v in got.items() if v}


def _calls_log(cfg, events):
    """The schedule's calls from the host plan alone: per call, in order, (pinned, rows) with rows of (speaker, window, samples that
    speaker has been fed, {frame: (values [J, F], mask [J, F])} of the pinned frames the window owns)."""
    AL = cfg.audio_len
    pool, who, fed, log = HostPool(CAP, AL), {}, {k: 0 for k in SPEAKERS}, []
    store = [{} for _ in range(CAP)]
    for event, payload in events:
        if event == "join":
            s = pool.join(payload[1])
            who[s], store[s] = payload[0], {}
            continue
        if event in ("pin", "unpin"):
            s = next(s for s, k in who.items() if k == payload[0] and pool.open[s])
            if event == "unpin":
                for n in payload[1]:
                    store[s].pop(n, None)
                continue
            poses, mask = _target(cfg, *payload)
            for k, n in enumerate(payload[1]):
                v, m = store[s].get(n, (torch.zeros(cfg.njoints, cfg.nfeats, device=DEV), torch.zeros(cfg.njoints, cfg.nfeats, dtype=torch.bool, device=DEV)))
                mk = torch.ones_like(m) if mask is None else mask[..., k]
                store[s][n] = (torch.where(mk, poses[..., k], v), m | mk)
            continue
        lengths = payload[0] if event == "push" else [0] * CAP
        closing = [int(event == "close" or (event == "leave" and who.get(s) == payload[0])) * int(pool.open[s]) for s in range(CAP)]
        before = pool.ran.copy()
        for s, n in enumerate(lengths):
            if n:
                fed[who[s]] += n
        rounds, _ = pool.push(lengths, closing)
        calls = long_form.pool_pin_plan(before, [sum(s in r for r in rounds) for s in range(CAP)], [set(d) for d in store], cfg)
        for r, pinned, slots in calls:
            rows = []
            for s in slots:
                w = int(before[s]) + r
                mine = {n: store[s].pop(n) for n in sorted(store[s]) if pinned and owned(w)[0] <= n < owned(w)[1]}
                assert bool(mine) == pinned
                rows.append((who[s], w, fed[who[s]], mine))
            log.append((pinned, rows))
        for s in range(CAP):
            if closing[s]:
                store[s] = {}
    return log


def _oracle(parts, y, log, seed):
    """One public sampling call per logged call, at its batch, in order: ``_oracle`` of test_gpu_long_pool.py, a pinned call with
    ``inpainting_mask`` / ``inpainted_motion`` built by the rule -- true and the pinned value on the pinned elements of the frames the
    window owns (its prefix frames are never kept), zero elsewhere.  Under ``'philox'`` call q draws at ``sample_offset = q << 48``."""
    cfg, model, diffusion, sampler, skip, _ = parts
    loop = diffusion.ddim_sample_loop if sampler == "ddim" else diffusion.p_sample_loop
    last, frames = {}, {k: [] for k in SPEAKERS}
    torch.manual_seed(seed)
    for q, (pinned, rows) in enumerate(log):
        diffusion.sample_offset = q << 48
        idx = torch.tensor([SPEAKERS[k] for k, _, _, _ in rows], device=DEV)
        shape = (len(rows), cfg.njoints, cfg.nfeats, T)
        origin_x = torch.zeros(shape, device=DEV)
        audio = torch.zeros(len(rows), cfg.audio_len, device=DEV)
        keep, motion = torch.zeros(shape, dtype=torch.bool, device=DEV), torch.zeros(shape, device=DEV)
        for i, (k, w, n, mine) in enumerate(rows):
            origin_x[i, :, :, :cfg.n_pre_seq] = last[k][..., T - cfg.n_pre_seq:] if w else y["seed_poses"][SPEAKERS[k]]
            audio[i] = long_form.window_audio(y["audio"][SPEAKERS[k]:SPEAKERS[k] + 1, :n], w, cfg)[0]
            for frame, (v, m) in mine.items():
                assert owned(w)[0] <= frame < owned(w)[1]
                keep[i, :, :, frame - S * w] = m
                motion[i, :, :, frame - S * w] = torch.where(m, v, torch.zeros_like(v))
        yy = {"audio_input": audio, "origin_x": origin_x, "vid_indices": y["vid_indices"][idx].contiguous(), "scale": y["scale"][idx].contiguous()}
        if pinned:
            yy["inpainting_mask"], yy["inpainted_motion"] = keep, motion
        if "emo" in y:
            yy["emo"] = y["emo"][idx, 0:1].expand(len(rows), T).contiguous()
        x = loop(model, shape, clip_denoised=False, model_kwargs={"y": yy}, skip_timesteps=skip, init_image=None, progress=False,
                 dump_steps=None, noise=None, const_noise=False).contiguous()
        for i, (k, w, _, _) in enumerate(rows):
            last[k] = x[i]
            frames[k].append(x[i] if w == 0 else x[i, :, :, cfg.n_pre_seq:])
    diffusion.sample_offset = 0
    return {k: torch.cat(v, dim=2) for k, v in frames.items() if v}


def _check_pins_hold(cfg, got, events, schedule="ddim"):
    """The returned frames sit on the pinned values.  At the last step (t = 0) neither tree re-noises, so pred_xstart IS the pinned
    value there.  DDIM then returns ``x_0 * sqrt(acp_prev) + sqrt(1 - acp_prev) * eps`` with ``acp_prev = 1.0``: x_0 itself, exactly.
    DDPM returns the posterior mean ``c1 x_0 + c2 x_t`` with ``c2 = 0`` (``1 - acp_prev``) and ``c1 = beta_0 / (1 - acp_0)``, which is 1
    up to one rounding of its fp32 cast: at most 2^-23 |x_0| + one rounding of the product, below 2^-22 for poses in [-1, 1]."""
    tol = 0.0 if schedule == "ddim" else 2.0 ** -22
    for event, payload in events:
        if event == "pin":
            poses, mask = _target(cfg, *payload)
            at = got[payload[0]][:, :, payload[1]]
            err = (at - poses).abs() if mask is None else (at - poses).abs()[mask]
            print(f"pinned {payload}: max |frame - pose| on the pinned elements = {float(err.max()):.3e} (bound {tol:.3e})")
            assert float(err.max()) <= tol, payload


@pytest.mark.parametrize("schedule", ["ddim", "ddpm"])
@pytest.mark.parametrize("ds", ["ted", "beat"])
def test_pinned_schedule_is_bitwise_the_loop_of_public_calls(ds, schedule):
    parts, y = _parts(ds, schedule), _speakers(ds)
    cfg = parts[0]
    events = pinned_schedule(cfg.audio_len)
    log = _calls_log(cfg, events)
    assert [(p, len(r)) for p, r in log] == [(p, len(s)) for calls in EXPECTED_CALLS for _, p, s in calls]
    want = _oracle(parts, y, log, 61)
    torch.manual_seed(61)
    got = _run(parts, y, events)
    assert [int(got[k].shape[2]) for k in "ABCD"] == [T + S, T + S, T + 2 * S, T]
    for k in "ABCD":
        print(f"{ds} {schedule} speaker {k}: max |pool - public loops| = {float((got[k] - want[k]).abs().max()):.3e}")
        assert bool(torch.isfinite(got[k]).all()) and torch.equal(got[k], want[k]), (k, float((got[k] - want[k]).abs().max()))
    _check_pins_hold(cfg, got, events, schedule)
    # frame 67 of C pins one feature of one joint where frame 3 (the same ring position) pinned the whole pose: the rest of the
    # pose must be free again, so it is what the public loop gave (checked above) and not the pose of frame 3
    assert not torch.equal(got["C"][:, :, 67], got["C"][:, :, 3])


@pytest.mark.parametrize("ds", ["ted", "beat"])
def test_pinned_schedule_under_philox_is_keyed_by_the_call(ds):
    parts, y = _parts(ds, "ddim"), _speakers(ds)
    cfg, diffusion = parts[0], parts[2]
    events = pinned_schedule(cfg.audio_len)
    diffusion.noise_source, diffusion.philox_seed = "philox", 0x51DE_CA11
    try:
        want = _oracle(parts, y, _calls_log(cfg, events), 0)
        got = _run(parts, y, events)
    finally:
        diffusion.noise_source, diffusion.philox_seed, diffusion.sample_offset = "torch_cpu", None, 0
    for k in "ABCD":
        print(f"{ds} philox speaker {k}: max |pool - public loops| = {float((got[k] - want[k]).abs().max()):.3e}")
        assert bool(torch.isfinite(got[k]).all()) and torch.equal(got[k], want[k]), (k, float((got[k] - want[k]).abs().max()))
    _check_pins_hold(cfg, got, events)


@pytest.mark.parametrize("ds", ["ted", "beat"])
def test_a_pool_that_is_never_pinned_is_the_pool_it_was(ds):
    parts, y = _parts(ds, "ddim"), _speakers(ds)
    events = staggered(parts[0].audio_len)
    torch.manual_seed(97)
    plain = _run(parts, y, events, pins=None)
    torch.manual_seed(97)
    armed = _run(parts, y, events, pins=HORIZON)
    for k in "ABCD":
        assert torch.equal(plain[k], armed[k]), k


@pytest.mark.parametrize("ds", ["ted", "beat"])
def test_keyed_pool_a_pinned_clip_does_not_depend_on_its_neighbours(ds):
    parts, y = _parts(ds, "ddim"), _speakers(ds)
    cfg, diffusion = parts[0], parts[2]
    AL = cfg.audio_len
    keys = {"A": 11, "B": 22, "C": 33}

    def events(names):
        """The speakers joined in order and fed alike: two windows each; A is pinned in both of its windows, so each of its calls is
        a pinned call at batch 1 whoever runs beside it, and the others' calls are plain calls of the others alone."""
        on = [int(i < len(names)) for i in range(CAP)]
        ev = [("join", (k, None)) for k in names]
        if "A" in names:
            ev += [("pin", ("A", [10], "pose")), ("pin", ("A", [50], "feature"))]
        return ev + [("push", ([AL * o for o in on], None)), ("push", ([STRIDE * o for o in on], None)), ("close", [])]

    diffusion.noise_source, diffusion.philox_seed = "philox", 0xC11F_0001
    try:
        alone = _run(parts, y, events("A"), noise_keys="clip", keys=keys)
        beside = _run(parts, y, events("ABC"), noise_keys="clip", keys=keys)
        others = _run(parts, y, events("BC"), noise_keys="clip", keys=keys)
    finally:
        diffusion.noise_source, diffusion.philox_seed = "torch_cpu", None
    assert torch.equal(alone["A"], beside["A"]) and int(alone["A"].shape[2]) == T + S
    _check_pins_hold(cfg, beside, events("A"))
    for k in "BC":
        assert torch.equal(beside[k], others[k]), k


def _stream_pins(cfg):
    """Pins of the stream test, every clip alike: frame 33 (window 0 owns it, window 1 starts from it) as a whole pose, frame 36
    (window 1) as one feature of one joint; window 2 runs plain."""
    g = torch.Generator().manual_seed(9001)
    poses = (torch.rand(B, cfg.njoints, cfg.nfeats, 2, generator=g) * 2 - 1).to(DEV)
    mask = torch.ones(B, cfg.njoints, cfg.nfeats, 2, dtype=torch.bool, device=DEV)
    mask[..., 1] = False
    mask[:, cfg.njoints // 2, cfg.nfeats - 1, 1] = True
    return [33, 36], poses, mask


@pytest.mark.parametrize("ds", ["ted", "beat"])
def test_a_pinned_stream_is_the_pool_used_like_a_stream(ds):
    parts = _parts(ds, "ddim")
    cfg, model, diffusion, sampler, skip, y = parts
    audio = y["audio"][:, :_length(cfg)].contiguous()
    emo = None if _emo(parts) is None else _emo(parts)[:, 0].contiguous()
    frames, poses, mask = _stream_pins(cfg)
    for sizes in (_edge_chunks(cfg), [STRIDE + 17, _length(cfg) - STRIDE - 17]):
        torch.manual_seed(101)
        st = long_form.open_stream(diffusion, model, y["seed_poses"], y["vid_indices"], y["scale"], emo=emo, sampler=sampler, skip_timesteps=skip, pins=HORIZON)
        st.pin(frames, poses, mask)
        assert st.pins == 2
        outs, pos = [], 0
        for n in sizes:
            outs.append(st.push(audio[:, pos:pos + n]))
            pos += n
        outs.append(st.close())
        assert st.pins == 0
        want = torch.cat(outs, dim=3)
        assert int(want.shape[3]) == T + 2 * S
        torch.manual_seed(101)
        pool = long_form.open_pool(diffusion, model, CAP, sampler=sampler, skip_timesteps=skip, pins=HORIZON)
        for b in range(B):
            assert pool.join(y["seed_poses"][b], y["vid_indices"][b], y["scale"][b], emo=None if emo is None else emo[b]) == b
            pool.pin(b, frames, poses[b], mask[b])
        outs, pos = [], 0
        for n in sizes:
            chunk = audio.new_zeros(CAP, n)
            chunk[:B] = audio[:, pos:pos + n]
            outs.append(pool.push(chunk, [n] * B + [0] * (CAP - B))[0][:B])
            pos += n
        outs.append(pool.close()[0][:B])
        got = torch.cat(outs, dim=3)
        assert torch.equal(got, want), (sizes, float((got - want).abs().max()))
        at = want[:, :, :, frames]
        assert float((at - poses).abs()[mask].max()) == 0.0


def test_unpin_counts_and_a_reused_slot():
    parts, y = _parts("ted", "ddim"), _speakers("ted")
    cfg, model, diffusion, sampler, skip, _ = parts
    AL = cfg.audio_len
    one = lambda n: [n, 0, 0, 0]        # noqa: E731

    def fresh(pins):
        pool = long_form.open_pool(diffusion, model, CAP, sampler=sampler, skip_timesteps=skip, pins=pins)
        assert _join(pool, y, "A") == 0
        return pool

    def two_windows(pool):
        torch.manual_seed(103)
        frames, counts = pool.push(y["audio"][:, :AL + STRIDE].contiguous(), one(AL + STRIDE))
        assert counts.tolist() == one(T + S)
        return frames[0]

    plain = two_windows(fresh(None))
    # an unpin before the owning window runs gives the unpinned bits
    pool = fresh(HORIZON)
    pool.pin(0, [10, 40], *_target(cfg, "A", [10, 40], "pose"))
    assert pool.slots["pins"].tolist() == one(2)
    pool.unpin(0, [10])
    assert pool.slots["pins"].tolist() == one(1)
    pool.unpin(0)
    assert pool.slots["pins"].tolist() == one(0)
    assert torch.equal(two_windows(pool), plain)
    # the count goes down as windows spend their pins, is 0 after the leave, and a join into the freed slot starts with none
    pool = fresh(HORIZON)
    pool.pin(0, [10, 40], *_target(cfg, "A", [10, 40], "pose"))
    torch.manual_seed(103)
    first, counts = pool.push(y["audio"][:, :AL].contiguous(), one(AL))
    assert counts.tolist() == one(T) and pool.slots["pins"].tolist() == one(1)              # window 0 spent frame 10
    assert not torch.equal(first[0], plain[:, :, :T]) and torch.equal(first[0][:, :, 10], _target(cfg, "A", [10, 40], "pose")[0][:, :, 0])
    pool.pin(0, [90], *_target(cfg, "A", [90], "feature"))                                  # window 2 would own it; the clip never gets there
    assert pool.slots["pins"].tolist() == one(2)
    with pytest.raises(ValueError, match="outside"):
        pool.pin(0, [33], *_target(cfg, "A", [33], "pose"))                                 # already returned
    with pytest.raises(_lib.EngineError, match="outside"):
        model.model.engine().long_pool_pin(0, [33], _target(cfg, "A", [33], "pose")[0])     # the engine refuses it too
    with pytest.raises(_lib.EngineError, match="twice"):
        model.model.engine().long_pool_pin(0, [41, 41], _target(cfg, "A", [41, 42], "pose")[0])
    with pytest.raises(_lib.EngineError, match="not open"):
        model.model.engine().long_pool_pin(2, [41], _target(cfg, "A", [41], "pose")[0])
    assert pool.slots["pins"].tolist() == one(2)
    tail = pool.leave(0)                                                                    # exactly AL samples: nothing is owed
    assert tail.shape[2] == 0 and pool.slots["pins"].tolist() == one(0) and not pool.slots["open"][0]
    assert _join(pool, y, "A") == 0 and pool.slots["pins"].tolist() == one(0)
    assert torch.equal(two_windows(pool), plain)                                            # no pin of the clip before it is left in the ring


@pytest.mark.parametrize("order", ["pinned_then_plain", "plain_then_pinned"])
@pytest.mark.parametrize("ds", ["ted", "beat"])
def test_one_stream_push_runs_a_pinned_and_a_plain_window(ds, order):
    """One push that completes windows 0 and 1, one of them pinned: two loops at the stream's batch, the inpainting one and the plain
    one, back to back with no host wait between them -- the stream keeps both captured loops, as a pool does.  A third window, of the
    other kind than window 1, then replays the loop window 0 captured.  Bitwise the pool used like a stream."""
    parts = _parts(ds, "ddim")
    cfg, model, diffusion, sampler, skip, y = parts
    AL = cfg.audio_len
    audio = y["audio"][:, :AL + 2 * STRIDE].contiguous()
    emo = None if _emo(parts) is None else _emo(parts)[:, 0].contiguous()
    g = torch.Generator().manual_seed(9002)
    poses = (torch.rand(B, cfg.njoints, cfg.nfeats, 1, generator=g) * 2 - 1).to(DEV)
    # (frame pinned ahead of the push or None, samples pushed): windows 0 and 1 in one push, window 2 in the next
    steps = {"pinned_then_plain": [(10, AL + STRIDE), (70, STRIDE)], "plain_then_pinned": [(40, AL + STRIDE), (None, STRIDE)]}[order]
    torch.manual_seed(107)
    st = long_form.open_stream(diffusion, model, y["seed_poses"], y["vid_indices"], y["scale"], emo=emo, sampler=sampler, skip_timesteps=skip, pins=HORIZON)
    outs, pos = [], 0
    for frame, n in steps:
        if frame is not None:
            st.pin([frame], poses)
        outs.append(st.push(audio[:, pos:pos + n]))
        pos += n
        assert st.pins == 0
    outs.append(st.close())
    want = torch.cat(outs, dim=3)
    assert [int(o.shape[3]) for o in outs] == [T + S, S, 0]
    if diffusion.use_graph:             # window 2 is of window 0's kind: its loop is still there
        assert model.model.engine().timing()["graph_replayed"] == 1
    torch.manual_seed(107)
    pool = long_form.open_pool(diffusion, model, CAP, sampler=sampler, skip_timesteps=skip, pins=HORIZON)
    for b in range(B):
        assert pool.join(y["seed_poses"][b], y["vid_indices"][b], y["scale"][b], emo=None if emo is None else emo[b]) == b
    outs, pos = [], 0
    for frame, n in steps:
        for b in range(B if frame is not None else 0):
            pool.pin(b, [frame], poses[b])
        chunk = audio.new_zeros(CAP, n)
        chunk[:B] = audio[:, pos:pos + n]
        outs.append(pool.push(chunk, [n] * B + [0] * (CAP - B))[0][:B])
        pos += n
    outs.append(pool.close()[0][:B])
    got = torch.cat(outs, dim=3)
    assert torch.equal(got, want), (order, float((got - want).abs().max()))
    for frame, _ in steps:
        if frame is not None:
            assert float((want[:, :, :, frame] - poses[..., 0]).abs().max()) == 0.0, frame
