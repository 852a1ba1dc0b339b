"""The post-processing stream on the GPU (postprocess.open_post_stream -> ls_post_stream_open / _push, csrc/ls_post_stream.hip), alone
and owned by a long-form session (long_form.open_stream / open_pool with post=).

The contract: per slot, everything a stream returns, concatenated over the pushes and the finish, is BIT FOR BIT what the existing
timeline entries give for the whole series (``ted_postprocess_timeline``; ``beat_postprocess_timeline`` + ``beat_metrics_timeline``'s
beat_mask; ``frames=`` for clips of different lengths), under any chunking -- also past the timeline entries' 4096 frames.  Equality is
``np.array_equal`` throughout.  Inputs: smoothed random walks around zero, plus a G22 fixture timeline in one TED slot."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import timeline_restatement as T
from livelyspeaker_amd import beat_metrics as bm, long_form, postprocess as pp, synth
from livelyspeaker_amd.cfg_sampler import ClassifierFreeSampleModel
from livelyspeaker_amd.model_util import create_model_and_diffusion, load_model_wo_clip

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TED_N = (150, 97, 4)
TED_KEYS = ("aligned_motions", "pose", "angle_diff")
BEAT_KEYS = ("decoded_motions", "pred_euler")
STRIDE = 32000


def _walk(rng, S, J, F, N, step=0.02, smooth=4):
    z = np.cumsum(rng.standard_normal((S * J * F, N + smooth)) * step, axis=1)
    w = np.stack([np.convolve(r, np.ones(smooth) / smooth, mode="valid") for r in z])[:, :N]
    return (w - w.mean(axis=1, keepdims=True)).reshape(S, J, F, N).astype(np.float32)


def _np(v):
    return v.detach().cpu().numpy() if hasattr(v, "detach") else np.asarray(v)


class Series:
    """One series' outputs as the pushes return them: rows of the per-frame outputs, beat entries, beat times."""

    def __init__(self, keys, beat):
        self.rows, self.mask, self.times, self.next, self.beat = {k: [] for k in keys}, [], [], 0, beat

    def take(self, out, s, k):
        for key, rows in self.rows.items():
            v = _np(out[key][s])
            assert not v[k:].any(), key                                 # zero behind the slot's count
            rows.append(v[:k])
        first, count = int(out["beat_first"][s]), int(out["beat_count"][s])
        assert first == self.next
        m = _np(out["beat_mask"][s])
        assert m.dtype == bool and not m[..., count:].any()
        self.mask.append(m[..., :count])
        self.next = first + count
        if not self.beat:
            assert out["motion_beat_times"][s] == [float(first + q) / 15.0 for q in np.nonzero(m[:count])[0]]
            self.times += out["motion_beat_times"][s]

    def cat(self):
        return {k: np.concatenate(v) for k, v in self.rows.items()}, np.concatenate(self.mask, axis=-1)


def _schedule(N, sizes, late=()):
    """Per-slot chunk lists -> the pushes (counts [S], finish [S]).  A slot's series ends with its last chunk, or, for the slots in
    ``late``, with a push of its own that brings no frame."""
    sizes = [list(c) for c in sizes]
    assert [sum(c) for c in sizes] == list(N)
    for s in late:
        sizes[s].append(0)
    P = max(len(c) for c in sizes)
    return [(np.array([c[p] if p < len(c) else 0 for c in sizes]), np.array([p == len(c) - 1 for c in sizes])) for p in range(P)]


def _chunks(n, head, rest):
    """``head``, then chunks of ``rest``, cut to n frames in all (an idle push, 0, stays where ``head`` has it)."""
    out = []
    for c in head:
        out.append(min(c, n - sum(out)))
    while sum(out) < n:
        out.append(min(rest, n - sum(out)))
    while len(out) > 1 and out[-1] == 0:
        out.pop()
    return out


def _schedules(N):
    """The issue's chunkings: at once, all ones, [34, 30, 30, ...], [63, 1, 1, 64, ...] (crosses the 64-frame tile on both sides), and a
    ragged one with idle pushes and slots that finish in different pushes."""
    ragged = [_chunks(N[0], [0, 50, 0, 3, 0], 70), _chunks(N[1], [N[1] // 2, 0, 0, 1, 2], 33), _chunks(N[2], [1, 0, 2], 1)]
    return {"at_once": _schedule(N, [[n] for n in N]),
            "ones": _schedule(N, [[1] * n for n in N]),
            "windows": _schedule(N, [_chunks(n, [34], 30) for n in N]),
            "tile_edges": _schedule(N, [_chunks(n, [63, 1, 1, 64], 64) for n in N]),
            "ragged": _schedule(N, ragged, late=(1,))}


def _run(ps, x, pushes, keys, starts=None, got=None):
    """Feed the series x [S, J, F, N_max] (a device tensor) along ``pushes``, from frame ``starts[s]`` on; returns each slot's Series
    (``got``: the ones to continue)."""
    S = x.shape[0]
    at = np.zeros(S, np.int64) if starts is None else np.array(starts)
    got = [Series(keys, ps.dataset == "beat") for _ in range(S)] if got is None else got
    for counts, finish in pushes:
        K = int(counts.max())
        frames = torch.full((S,) + tuple(x.shape[1:3]) + (K,), float("nan"), device=DEV)        # behind a count: never read
        for s in range(S):
            frames[s, :, :, :counts[s]] = x[s, :, :, at[s]:at[s] + counts[s]]
        before = ps.frames_in
        out = ps.push(frames, counts, finish)
        assert np.array_equal(ps.frames_in, np.where(finish, 0, before + counts))
        for s in range(S):
            if counts[s] or out["beat_count"][s]:
                got[s].take(out, s, int(counts[s]))
        at += counts
    return got


@functools.lru_cache(maxsize=None)
def _ted_case():
    rng = np.random.default_rng(20261021)
    x = _walk(rng, 3, 9, 3, max(TED_N))
    g = T.g22("ted")[T.CASES[0]][0]
    x[1, :, :, :94] = g                                                  # the fixture timeline, continued by its own walk
    x[1, :, :, 94:] += g[:, :, 93:94] - x[1, :, :, 93:94]
    xd = torch.from_numpy(x).to(DEV)
    want = pp.ted_postprocess_timeline(xd, frames=TED_N)
    mask = _np(want["beat_mask"])
    for s, n in enumerate(TED_N):                                        # a condition on the input, decided by the existing kernel
        if n >= 64:
            assert mask[s, :n].sum() >= 3 and (~mask[s, 2:n - 1]).sum() >= 3
    return xd, {k: _np(v) if k != "motion_beat_times" else v for k, v in want.items()}


def _check_ted(got, want, s, n):
    rows, mask = got.cat()
    for k in TED_KEYS:
        assert np.array_equal(rows[k], want[k][s, :n]), (k, s)
    assert np.array_equal(mask, want["beat_mask"][s, :n]), s
    assert got.times == want["motion_beat_times"][s], s


@pytest.mark.parametrize("name", ["at_once", "ones", "windows", "tile_edges", "ragged"])
def test_ted_stream_is_bitwise_the_timeline_under_any_chunking(name):
    x, want = _ted_case()
    with pp.open_post_stream("ted", 3) as ps:
        got = _run(ps, x, _schedules(TED_N)[name], TED_KEYS)
        assert not ps.frames_in.any()
    for s, n in enumerate(TED_N):
        _check_ted(got[s], want, s, n)


@functools.lru_cache(maxsize=None)
def _beat_case(J, order):
    N = (80, 41, 2 * order + 2)
    rng = np.random.default_rng(20261021 + 10 * J + order)
    x = _walk(rng, 3, J, 6, max(N), step=0.05)
    x[:, :, 0] += 1.0                                                    # around the identity's rot6d (1, 0, 0, 0, 1, 0)
    x[:, :, 4] += 1.0
    xd = torch.from_numpy(x).to(DEV)
    series = bm.BEAT_SERIES_JOINTS if J == 47 else (0, 1, 2, 3, 4, 2)
    post = pp.beat_postprocess_timeline(xd, frames=N)
    mask = _np(bm.beat_metrics_timeline(post["pred_euler"], joints=J, series_joints=series, order=order, want=("beat_mask",), frames=N)["beat_mask"])
    assert mask[0].sum() >= 6 and mask[1].sum() >= 3
    return xd, N, series, {"decoded_motions": _np(post["decoded_motions"]), "pred_euler": _np(post["pred_euler"]), "beat_mask": mask.astype(bool)}


def _check_beat(got, want, s, n):
    rows, mask = got.cat()
    for k in BEAT_KEYS:
        assert np.array_equal(rows[k], want[k][s, :n]), (k, s)
    assert mask.shape == (6, n - 1) and np.array_equal(mask, want["beat_mask"][s, :, :n - 1]), s


@pytest.mark.parametrize("J,order,name", [(47, o, n) for o in (1, 2, 3) for n in ("at_once", "ones", "windows", "tile_edges", "ragged")] +
                         [(5, 2, "ragged")])
def test_beat_stream_is_bitwise_the_timeline_under_any_chunking(J, order, name):
    x, N, series, want = _beat_case(J, order)
    with pp.open_post_stream("beat", 3, order=order, series_joints=series, joints=J) as ps:
        got = _run(ps, x, _schedules(N)[name], BEAT_KEYS)
    for s, n in enumerate(N):
        _check_beat(got[s], want, s, n)


def test_a_finished_slot_starts_a_new_series_while_the_others_continue():
    x, want = _ted_case()
    ps = pp.open_post_stream("ted", 3)
    # slot 1 runs the 4-frame series of slot 2's input first, finishes it, then runs its own 97 frames; slots 0 and 2 just continue
    first = torch.stack([x[0], x[2], x[2]])
    a = _run(ps, first, [(np.array([40, 3, 1]), np.zeros(3, bool)), (np.array([30, 1, 1]), np.array([False, True, False]))], TED_KEYS)
    assert ps.frames_in.tolist() == [70, 0, 2]
    rest = _schedule((80, 97, 2), [[50, 30], [34, 63], [1, 1]])
    b = _run(ps, x, rest, TED_KEYS, starts=(70, 0, 2), got=[a[0], Series(TED_KEYS, False), a[2]])
    assert ps.close() is None and not ps.frames_in.any()             # every series has finished: nothing is pending
    _check_ted(a[1], want, 2, 4)
    _check_ted(b[1], want, 1, 97)
    _check_ted(b[0], want, 0, TED_N[0])
    _check_ted(b[2], want, 2, TED_N[2])


def test_finish_and_close_emit_the_pending_minima():
    """``finish(slot)`` and ``close()`` are pushes without frames: BEAT's up to ``order`` pending entries, clamped at the last velocity."""
    x, _, series, _ = _beat_case(47, 3)
    N = (20, 9)
    post = pp.beat_postprocess_timeline(x[:2, :, :, :20].contiguous(), frames=N)
    mask = _np(bm.beat_metrics_timeline(post["pred_euler"], series_joints=series, order=3, want=("beat_mask",), frames=N)["beat_mask"]).astype(bool)
    want = {"decoded_motions": _np(post["decoded_motions"]), "pred_euler": _np(post["pred_euler"]), "beat_mask": mask}
    ps = pp.open_post_stream("beat", 2, order=3, series_joints=series)
    got = _run(ps, x[:2], [(np.array(N), np.zeros(2, bool))], BEAT_KEYS)
    tail = ps.finish(0)
    assert tail["beat_count"].tolist() == [3, 0] and ps.frames_in.tolist() == [0, 9]
    got[0].take(tail, 0, 0)
    tail = ps.close()
    assert tail["beat_first"].tolist() == [0, 5] and tail["beat_count"].tolist() == [0, 3]
    got[1].take(tail, 1, 0)
    for s, n in enumerate(N):
        _check_beat(got[s], want, s, n)
    with pytest.raises(RuntimeError):
        ps.push(x[:2, :, :, :1].contiguous())


def test_a_series_longer_than_the_timeline_entries_take():
    N, M = 4200, pp.TIMELINE_MAX_FRAMES
    x = torch.from_numpy(_walk(np.random.default_rng(7), 1, 9, 3, N)).to(DEV)
    with pp.open_post_stream("ted", 1) as ps:
        nbytes = ps.device_bytes()
        got = _run(ps, x, _schedule((N,), [_chunks(N, [], 250)]), TED_KEYS)[0]
        assert ps.device_bytes() == nbytes
    rows, mask = got.cat()
    assert mask.shape == (N,) and all(v.shape[0] == N for v in rows.values())
    head = pp.ted_postprocess_timeline(x[..., :M])
    for k in TED_KEYS:
        assert np.array_equal(rows[k][:M], _np(head[k])[0]), k
    assert np.array_equal(mask[:M - 1], _np(head["beat_mask"])[0, :M - 1])
    # a frame's numbers depend on at most 2 frames to its left: from frame 106 on, the series [104, 4200) agrees with the stream
    tail = pp.ted_postprocess_timeline(x[..., N - M:])
    for k in TED_KEYS:
        assert np.array_equal(rows[k][N - M + 2:], _np(tail[k])[0, 2:]), k
    assert np.array_equal(mask[N - M + 2:], _np(tail["beat_mask"])[0, 2:])


@functools.lru_cache(maxsize=None)
def _parts(ds):
    """Synthetic weights, 2 executed steps per window (1000 steps respaced to 100, skip 98), B = 2."""
    cfg = synth.CONFIGS[ds]
    args = SimpleNamespace(mdm_condm="text", latent_dim=512, ff_size=1024, layers=8, cond_mask_prob=0.1, arch="trans_enc",
                           emb_trans_dec=False, dataset="humanml", lang_model=None, mlpact="silu", diffusion_steps=1000,
                           noise_schedule="cosine", sigma_small=True, lambda_vel=1.0, lambda_rcxyz=0.0, lambda_fc=0.0, njoints=cfg.njoints)
    model, diffusion = create_model_and_diffusion(args, "ddim100", dataset=ds)
    load_model_wo_clip(model, {k: torch.from_numpy(v) for k, v in synth.make_state_dict(cfg).items()})
    model = ClassifierFreeSampleModel(model).to(DEV)
    model.eval()
    y = {k: torch.from_numpy(v).to(DEV) for k, v in synth.make_long_cond(cfg, 3, 4).items()}
    return cfg, model, diffusion, y


def test_open_stream_with_post_returns_the_timeline_post_processing():
    cfg, model, diffusion, y = _parts("ted")
    B, skip = 2, diffusion.num_timesteps - 2
    cond = (y["seed_poses"][:B], y["vid_indices"][:B], y["scale"][:B])
    audio = y["audio"][:B, :cfg.audio_len + 2 * STRIDE - 5000].contiguous()       # three windows, the last one zero-padded
    torch.manual_seed(5)
    want = long_form.sample_long(diffusion, model, audio, *cond, sampler="ddim", skip_timesteps=skip)
    assert want.shape[3] == 94
    chunk = int(0.37 * 16000)

    def stream(post):
        torch.manual_seed(5)
        st = long_form.open_stream(diffusion, model, *cond, sampler="ddim", skip_timesteps=skip, post=post)
        outs = [st.push(audio[:, p:p + chunk]) for p in range(0, audio.shape[1], chunk)] + [st.close()]
        return outs

    plain = stream(None)
    assert all(torch.is_tensor(o) for o in plain) and torch.equal(torch.cat(plain, dim=3), want)
    outs = stream("ted")
    assert torch.equal(torch.cat([f for f, _ in outs], dim=3), want)
    got = [Series(("pose", "angle_diff", "aligned_motions"), False) for _ in range(B)]
    for f, d in outs:
        assert d["pose"].device == f.device and tuple(d["pose"].shape) == (B, f.shape[3], 10, 3)
        for s in range(B):
            got[s].take(d, s, int(f.shape[3]))
    ref = pp.ted_postprocess_timeline(want)
    ref = {k: _np(v) if k != "motion_beat_times" else v for k, v in ref.items()}
    for s in range(B):
        _check_ted(got[s], ref, s, 94)


def test_open_pool_with_post_follows_slots_that_leave_and_rejoin():
    cfg, model, diffusion, y = _parts("beat")
    AL, skip = cfg.audio_len, diffusion.num_timesteps - 2
    # (event, payload): speakers 0 and 1 staggered; 1 leaves (a padded window), 2 joins into its slot; the close ends 0 and 2
    events = [("join", 0), ("push", {0: AL}), ("join", 1), ("push", {0: STRIDE, 1: AL + 1000}), ("leave", 1), ("join", 2),
              ("push", {0: STRIDE, 2: AL}), ("close", None)]

    def run(post):
        torch.manual_seed(9)
        pool = long_form.open_pool(diffusion, model, 2, sampler="ddim", skip_timesteps=skip, post=post)
        who, fed, frames = {}, {}, {}
        got = {i: Series(BEAT_KEYS, True) for i in range(3)}
        for event, payload in events:
            if event == "join":
                s = pool.join(y["seed_poses"][payload], y["vid_indices"][payload], y["scale"][payload], emo=y["emo"][payload, 0])
                who[s], fed[payload], frames[payload] = payload, 0, []
                continue
            if event == "push":
                lengths = [payload.get(who.get(s), 0) for s in range(2)]
                audio = torch.zeros(2, max(lengths), device=DEV)
                for s, n in enumerate(lengths):
                    if n:
                        audio[s, :n] = y["audio"][who[s], fed[who[s]]:fed[who[s]] + n]
                        fed[who[s]] += n
                res = pool.push(audio, lengths)
                f, counts = res[0], res[1]
            elif event == "leave":
                slot = next(s for s, i in who.items() if i == payload)
                res = pool.leave(slot)
                f, counts = torch.zeros((2,) + tuple(res.shape if post is None else res[0].shape), device=DEV), np.zeros(2, np.int32)
                f[slot], counts[slot] = (res if post is None else res[0]), (res if post is None else res[0]).shape[2]
                if post is not None:
                    assert res[1].tolist() == counts.tolist()
            else:
                res = pool.close()
                f, counts = res[0], res[1]
            for s in range(2):
                if counts[s]:
                    frames[who[s]].append(f[s, :, :, :int(counts[s])])
            if post is not None:
                d = res[2]
                for s in range(2):
                    if s in who and (counts[s] or d["beat_count"][s]):
                        got[who[s]].take(d, s, int(counts[s]))
        return {i: torch.cat(v, dim=2) for i, v in frames.items()}, got

    plain, _ = run(None)
    frames, got = run("beat")
    assert [plain[i].shape[2] for i in range(3)] == [94, 64, 34]
    for i in range(3):
        assert torch.equal(frames[i], plain[i]), i
        n = frames[i].shape[2]
        post = pp.beat_postprocess_timeline(frames[i][None])
        mask = _np(bm.beat_metrics_timeline(post["pred_euler"], want=("beat_mask",))["beat_mask"]).astype(bool)
        _check_beat(got[i], {"decoded_motions": _np(post["decoded_motions"]), "pred_euler": _np(post["pred_euler"]), "beat_mask": mask}, 0, n)
