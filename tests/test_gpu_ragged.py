"""Clips of different lengths in one call, on the GPU: ls_onsets_ragged, the three ragged timeline entries, ls_ted_beat_align on a
zero-padded mask, and the Python chain above them (score_timeline, sample_long).

One yardstick, no new tolerance: on a clip's valid range every output of a ragged call equals BIT FOR BIT what the existing
equal-length entry point returns for that clip alone at its own length (those entry points are pinned to the reference by
test_gpu_onsets.py and test_gpu_timeline.py); beyond it the output is 0 (floats, byte masks) or -1 (the onset slabs).  The padded
inputs carry NaN beyond every clip's valid length, so a read past a clip's end shows up as a NaN or as a changed bit.  The solo
references are computed once per module and only read."""
import functools

import numpy as np
import pytest
import torch

import onsets_restatement as R
import timeline_restatement as T
from livelyspeaker_amd import _lib, audio_onsets as ao, beat_metrics as bm, long_form, postprocess as pp
from test_gpu_onsets import ENVELOPES, LENGTHS, OUTPUTS, SR, clips, host, restated
from test_gpu_timeline import MET_KEYS, TED_KEYS, seeded_onsets, seeded_target, synthetic

pytestmark = pytest.mark.gpu
SLABS = ("onset_raw", "onset_bt", "onset_bt_rms")
FMAX = 11025.0


def padded(rows, width, axis=-1):
    """Rows of different lengths along ``axis`` stacked into one array of that width, NaN beyond each row's own length."""
    shape = list(rows[0].shape)
    shape[axis] = width
    out = np.full([len(rows)] + shape, np.nan, np.float32)
    for b, r in enumerate(rows):
        idx = [b] + [slice(None)] * r.ndim
        idx[1 + (axis % r.ndim)] = slice(0, r.shape[axis])
        out[tuple(idx)] = r
    return out


def check_rows(got, solo, valid, fill, name):
    """got [B, W, ...] against one solo result [1, valid[b], ...] per clip: equal bits on the valid range, ``fill`` beyond it."""
    got = host(got)
    for b, n in enumerate(valid):
        want = host(solo[b])
        assert want.shape[0] == 1 and want.shape[1] == n, (name, b, want.shape, n)
        assert got.dtype == want.dtype and np.array_equal(got[b, :n], want[0], equal_nan=False), (name, b)
        assert (got[b, n:] == fill).all(), (name, b)


# ---- onsets --------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def solo_onsets(L, pad, which=0):
    y = clips(L)[which]
    return {k: host(v) for k, v in ao.audio_onsets(y[None, :L], SR, pad_mode=pad, fmax=FMAX, want=OUTPUTS).items()}


def check_onsets(got, solos, lengths):
    F = [1 + n // 512 for n in lengths]
    for k in ("mel_db", "rms", "oenv"):
        check_rows(got[k], [s[k] for s in solos], F, 0.0, k)
        assert all(np.isfinite(host(got[k])[b, :f]).all() for b, f in enumerate(F)), k
    for k in SLABS:
        check_rows(got[k], [s[k] for s in solos], F, -1, k)
    want = np.array([int(s["count"][0]) for s in solos], np.int32)
    assert np.array_equal(host(got["count"]), want) and np.array_equal(got["counts"], want)
    for b, c in enumerate(want):                         # within the valid range, the slab's own tail is -1 as well
        assert all((host(got[k])[b, c:] == -1).all() and (host(got[k])[b, :c] >= 0).all() for k in SLABS)


@pytest.mark.parametrize("pad", ["constant", "reflect"])
def test_onsets_of_six_lengths_in_one_call(pad):
    audio = padded([clips(L)[0] for L in LENGTHS], 100000)
    assert audio.shape == (6, 100000) and np.isnan(audio[:5, -1]).all()
    got = ao.audio_onsets(audio, SR, pad_mode=pad, fmax=FMAX, want=OUTPUTS, lengths=LENGTHS)
    assert host(got["mel_db"]).shape == (6, 196, 128) and host(got["onset_raw"]).shape == (6, 196)
    solos = [solo_onsets(L, pad) for L in LENGTHS]
    check_onsets(got, solos, LENGTHS)
    assert host(got["count"]).sum() > 0
    dev = ao.audio_onsets(torch.from_numpy(audio).cuda(), SR, pad_mode=pad, fmax=FMAX, want=OUTPUTS, lengths=np.array(LENGTHS))
    for k in OUTPUTS:
        assert dev[k].is_cuda and np.array_equal(host(dev[k]), host(got[k])), k
    times = ao.onset_times(audio, SR, pad_mode=pad, fmax=FMAX, lengths=LENGTHS)
    for b, s in enumerate(solos):
        assert np.array_equal(times[b], s["onset_raw"][0, :s["count"][0]] * 512 / float(SR)), b
    # independently of the solo call: the float64 restatement, under the inequality of test_gpu_onsets.test_envelope_rms_and_picks
    for b, L in enumerate(LENGTHS):
        r = restated(L, pad, FMAX)[0]
        (o64, e64), (o32, e32) = r[np.float64], r[np.float32]
        n64, f = R.normalise(o64), 1 + L // 512
        host_env = np.abs(R.normalise(o32.astype(np.float64)) - n64).max()
        err_env = np.abs(R.normalise(host(got["oenv"])[b, :f].astype(np.float64)) - n64).max()
        host_rms = np.abs(e32 - e64).max() / e64.max()
        err_rms = np.abs(host(got["rms"])[b, :f] - e64).max() / e64.max()
        print(f"L={L} {pad}: envelope device {err_env:.3e} host-f32 {host_env:.3e}; rms device {err_rms:.3e} host-f32 {host_rms:.3e}")
        assert err_env <= max(4 * host_env, 1e-6)
        assert err_rms <= max(4 * host_rms, 1e-6)


def test_onsets_at_the_frame_count_steps_and_below_one_fft_frame():
    lengths = [1, 511, 512, 513, 1024, 1025]             # F_b = 1, 1, 2, 2, 3, 3: clips shorter than the FFT frame, F_b < 3
    rows = [R.test_clip(70 + i, n, SR) for i, n in enumerate(lengths)]
    audio = padded(rows, 1025)
    got = ao.audio_onsets(audio, SR, pad_mode="constant", fmax=FMAX, want=OUTPUTS, lengths=lengths)
    assert host(got["oenv"]).shape == (6, 3)
    solos = [{k: host(v) for k, v in ao.audio_onsets(y[None], SR, pad_mode="constant", fmax=FMAX, want=OUTPUTS).items()} for y in rows]
    check_onsets(got, solos, lengths)


@pytest.mark.parametrize("sr_pick", [16000, 22050])
def test_given_envelopes_cut_to_different_lengths(sr_pick):
    frames = [12, 5, 1, 8, 3, 12, 7]
    env = padded([ENVELOPES[b, :n] for b, n in enumerate(frames)], 12)
    want = ("oenv", "count", "onset_raw", "onset_bt")
    got = ao.audio_onsets(onset_envelope=env, sr=sr_pick, want=want, lengths=frames)
    solos = [{k: host(v) for k, v in ao.audio_onsets(onset_envelope=ENVELOPES[b:b + 1, :n], sr=sr_pick, want=want).items()}
             for b, n in enumerate(frames)]
    check_rows(got["oenv"], [s["oenv"] for s in solos], frames, 0.0, "oenv")
    for k in ("onset_raw", "onset_bt"):
        check_rows(got[k], [s[k] for s in solos], frames, -1, k)
    assert np.array_equal(host(got["count"]), [int(s["count"][0]) for s in solos]) and host(got["count"]).sum() > 0
    full = ao.audio_onsets(onset_envelope=ENVELOPES, sr=sr_pick, want=want)
    assert np.array_equal(host(got["onset_raw"])[[0, 5]], host(full["onset_raw"])[[0, 5]])      # the two rows left whole
    dev = ao.audio_onsets(onset_envelope=torch.from_numpy(env).cuda(), sr=sr_pick, want=want, lengths=frames)
    for k in want:
        assert dev[k].is_cuda and np.array_equal(host(dev[k]), host(got[k])), k


# ---- TED timelines -------------------------------------------------------------------------------------------------------------------
TED_FRAMES = [4, 34, 63, 64, 65, 131]
BEAT_FRAMES = [6, 34, 64, 65, 131]


@pytest.fixture(scope="module")
def ted_case():
    """(padded timeline with NaN tails, per-clip timelines, per-clip solo results)."""
    rows = [synthetic("ted", 1, n) for n in TED_FRAMES]
    return padded([r[0] for r in rows], 131), rows, [pp.ted_postprocess_timeline(r) for r in rows]


def check_ted(got, solos, frames):
    for k in TED_KEYS:
        check_rows(got[k], [s[k] for s in solos], frames, 0, k)
    assert got["motion_beat_times"] == [s["motion_beat_times"][0] for s in solos]


def test_ted_timelines_of_six_lengths_in_one_call(ted_case):
    tl, _, solos = ted_case
    assert tl.shape == (6, 9, 3, 131) and np.isnan(tl[0, :, :, 4:]).all()
    got = pp.ted_postprocess_timeline(tl, frames=TED_FRAMES)
    assert got["pose"].shape == (6, 131, 10, 3) and got["beat_mask"].dtype == bool
    check_ted(got, solos, TED_FRAMES)
    for b, n in enumerate(TED_FRAMES):
        if n >= 34:
            assert got["beat_mask"][b].sum() > 0, b
    dev = pp.ted_postprocess_timeline(torch.from_numpy(tl).cuda(), frames=torch.tensor(TED_FRAMES))
    for k in TED_KEYS:
        assert dev[k].is_cuda and np.array_equal(host(dev[k]), got[k]), k
    assert dev["motion_beat_times"] == got["motion_beat_times"]
    no_pose = pp.ted_postprocess_timeline(tl, frames=TED_FRAMES, want_pose=False)
    assert no_pose["pose"] is None and np.array_equal(no_pose["beat_mask"], got["beat_mask"])


def test_ted_beat_align_on_the_zero_padded_mask_is_the_solo_sum(ted_case):
    """ls_ted_beat_align needs no ragged twin: a frame without a beat enters the minimum as +inf."""
    tl, _, solos = ted_case
    mask = pp.ted_postprocess_timeline(tl, frames=TED_FRAMES)["beat_mask"]
    counts = [5, 12, 0, 24, 7, 20]
    slab, count = T.onset_slab(np.random.default_rng(31), 6, 24, counts, 280)       # frames to 9 s: past the longest clip's last pose
    total, beats = pp.ted_beat_align(mask, slab, count)
    for b, s in enumerate(solos):
        t1, n1 = pp.ted_beat_align(s["beat_mask"], slab[b:b + 1], count[b:b + 1])
        assert total[b] == t1[0] and beats[b] == n1[0] == s["beat_mask"].sum(), b
    assert total[2] == 0.0 and (beats[1:] > 0).all() and (total[[1, 3, 4, 5]] > 0).all()
    want, acc = pp.BeatConsistency(), pp.BeatConsistency()
    for b, s in enumerate(solos):
        want.push_timeline(s["beat_mask"], slab[b:b + 1], count[b:b + 1])
    acc.push_timeline(mask, slab, count, frames=TED_FRAMES)
    assert (acc.num_beats, acc.motion_beats_sum) == (want.num_beats, want.motion_beats_sum) == (int(count[beats > 0].sum()), int(mask.sum()))
    assert abs(acc.score() - want.score()) <= 1e-12


# ---- BEAT timelines ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def beat_case():
    """Per clip: the timeline, its solo post-processing, onsets, target and semantic planes, and the solo metrics (order 2)."""
    out = []
    for i, n in enumerate(BEAT_FRAMES):
        tl = synthetic("beat", 1, n)
        post = pp.beat_postprocess_timeline(tl)
        onsets = seeded_onsets(1, n / 15.0, 300 + i)
        target, semantic = seeded_target(post["pred_euler"], 400 + i)
        out.append((tl, post, onsets, target, semantic, bm.beat_metrics_timeline(post["pred_euler"], target, semantic, onsets)))
    return out


def ragged_beat_inputs(beat_case):
    tl = padded([c[0][0] for c in beat_case], 131)
    pred = padded([c[1]["pred_euler"][0] for c in beat_case], 131, axis=0)       # NaN tails: the metrics never read them either
    target = padded([c[3][0] for c in beat_case], 131, axis=0)
    semantic = padded([c[4][0] for c in beat_case], 131, axis=0)
    return tl, pred, target, semantic, [c[2][0] for c in beat_case]


def check_metrics(got, solos, frames, keys=MET_KEYS):
    for k in keys:
        if k in ("srgr_sum", "align"):
            want = np.concatenate([s[k] for s in solos])
            assert host(got[k]).dtype == want.dtype and np.array_equal(host(got[k]), want), k
        elif k == "success":
            check_rows(got[k], [s[k] for s in solos], frames, 0, k)
        else:                                              # [B, 6, N - 1]: the frame axis is the last
            check_rows(np.swapaxes(host(got[k]), 1, 2), [np.swapaxes(s[k], 1, 2) for s in solos], [n - 1 for n in frames], 0, k)


def test_beat_timelines_of_five_lengths_in_one_call(beat_case):
    tl, pred, target, semantic, onsets = ragged_beat_inputs(beat_case)
    assert tl.shape == (5, 47, 6, 131) and np.isnan(pred[0, 6:]).all() and np.isnan(semantic[0, 6:]).all()
    post = pp.beat_postprocess_timeline(tl, frames=BEAT_FRAMES)
    for k in ("decoded_motions", "pred_euler"):
        check_rows(post[k], [c[1][k] for c in beat_case], BEAT_FRAMES, 0.0, k)
    got = bm.beat_metrics_timeline(pred, target, semantic, onsets, frames=BEAT_FRAMES)
    assert set(got) == set(MET_KEYS) and got["vel"].shape == (5, 6, 130) and got["success"].shape == (5, 131, 47)
    check_metrics(got, [c[5] for c in beat_case], BEAT_FRAMES)
    assert all(got["beat_mask"][b].sum() > 0 for b in range(1, 5)) and np.isfinite(got["align"]).all() and (got["srgr_sum"] > 0).all()
    dev_post = pp.beat_postprocess_timeline(torch.from_numpy(tl).cuda(), frames=BEAT_FRAMES)
    assert all(dev_post[k].is_cuda and np.array_equal(host(dev_post[k]), post[k]) for k in post)
    dev = bm.beat_metrics_timeline(torch.from_numpy(pred).cuda(), torch.from_numpy(target).cuda(), torch.from_numpy(semantic).cuda(), onsets,
                                   frames=BEAT_FRAMES)
    for k in MET_KEYS:
        assert dev[k].is_cuda and np.array_equal(host(dev[k]), got[k]), k
    only = bm.beat_metrics_timeline(pred, target, semantic, onsets, frames=BEAT_FRAMES, want=("srgr_sum", "align"))     # masks in temporaries
    assert set(only) == {"srgr_sum", "align"} and all(np.array_equal(only[k], got[k]) for k in only)


@pytest.mark.parametrize("order", [1, 40])
def test_beat_minima_of_other_orders_on_two_lengths(order, beat_case):
    frames = [82, 131]                                    # 2 * 40 + 2: the shortest clip order 40 takes; its halo spans the whole clip
    full = beat_case[-1][1]["pred_euler"]                 # the 131-frame clip; its first 82 frames are the other clip
    rows = [np.ascontiguousarray(full[:, :82]), full]
    pred = padded([r[0] for r in rows], 131, axis=0)
    got = bm.beat_metrics_timeline(pred, order=order, want=("vel", "beat_mask"), frames=frames)
    solos = [bm.beat_metrics_timeline(r, order=order, want=("vel", "beat_mask")) for r in rows]
    check_metrics(got, solos, frames, keys=("vel", "beat_mask"))
    assert got["beat_mask"].sum() > 0


# ---- equal lengths, and the old entries ------------------------------------------------------------------------------------------------
def test_equal_lengths_reproduce_the_equal_length_entries():
    tl = synthetic("ted", 3, 65)
    old, new = pp.ted_postprocess_timeline(tl), pp.ted_postprocess_timeline(tl, frames=[65] * 3)
    assert all(np.array_equal(old[k], new[k]) for k in TED_KEYS) and old["motion_beat_times"] == new["motion_beat_times"]
    tl = synthetic("beat", 3, 65)
    old, new = pp.beat_postprocess_timeline(tl), pp.beat_postprocess_timeline(tl, frames=[65] * 3)
    assert all(np.array_equal(old[k], new[k]) for k in old)
    onsets = seeded_onsets(3, 65 / 15.0, 8)
    target, semantic = seeded_target(old["pred_euler"], 9)
    args = (old["pred_euler"], target, semantic, onsets)
    mo, mn = bm.beat_metrics_timeline(*args), bm.beat_metrics_timeline(*args, frames=[65] * 3)
    assert all(mo[k].dtype == mn[k].dtype and np.array_equal(mo[k], mn[k]) for k in MET_KEYS)
    for L, pad in ((2048, "constant"), (36267, "reflect")):
        oo = ao.audio_onsets(clips(L), SR, pad_mode=pad, want=OUTPUTS)
        on = ao.audio_onsets(clips(L), SR, pad_mode=pad, want=OUTPUTS, lengths=[L] * 3)
        assert all(np.array_equal(host(oo[k]), host(on[k])) for k in OUTPUTS + ("counts",)), (L, pad)


def test_without_lengths_the_old_entries_are_called(monkeypatch):
    lib = _lib.load_library()

    def refuse(*a):
        raise AssertionError("a ragged entry was called without lengths")

    for name in ("ls_onsets_ragged", "ls_ted_post_timeline_ragged", "ls_beat_post_timeline_ragged", "ls_beat_metrics_timeline_ragged"):
        monkeypatch.setattr(lib, name, refuse)
    pp.ted_postprocess_timeline(synthetic("ted", 1, 34), frames=None)
    post = pp.beat_postprocess_timeline(synthetic("beat", 1, 34), frames=None)
    bm.beat_metrics_timeline(post["pred_euler"], want=("vel",), frames=None)
    ao.audio_onsets(clips(2048), SR, lengths=None)
    ao.onset_times(clips(2048), SR, lengths=None)
    with pytest.raises(AssertionError, match="ragged entry"):
        pp.ted_postprocess_timeline(synthetic("ted", 1, 34), frames=[34])


# ---- score_timeline --------------------------------------------------------------------------------------------------------------------
SCORE_FRAMES, SCORE_LENGTHS = [34, 131, 65], [36267, 100000, 512 * 40]


def score_audio():
    audio = padded([clips(L)[0] for L in SCORE_LENGTHS], 100000 + 777)          # a row stride beyond the longest clip
    return audio


def test_score_timeline_ted_against_per_clip_calls():
    rows = [synthetic("ted", 1, n) for n in SCORE_FRAMES]
    tl, audio = padded([r[0] for r in rows], 131), score_audio()
    acc = pp.BeatConsistency()
    got = long_form.score_timeline(tl, audio, frames=SCORE_FRAMES, audio_lengths=SCORE_LENGTHS, bc=acc)
    solo_acc, align_sum = pp.BeatConsistency(), 0.0
    for b, (r, L) in enumerate(zip(rows, SCORE_LENGTHS)):
        one = pp.BeatConsistency()
        s = long_form.score_timeline(r, audio[b:b + 1, :L], bc=one)
        assert got["motion_beat_times"][b] == s["motion_beat_times"][0], b
        n = SCORE_FRAMES[b]
        assert np.array_equal(got["pose"][b, :n], s["pose"][0]) and not got["pose"][b, n:].any()
        assert np.array_equal(got["beat_mask"][b, :n], s["beat_mask"][0]) and not got["beat_mask"][b, n:].any()
        solo_acc.num_beats += one.num_beats
        solo_acc.motion_beats_sum += one.motion_beats_sum
        solo_acc.align_sum += one.align_sum
    print("bc", got["bc"], "per clip", solo_acc.score(), "onsets", acc.num_beats, "motion beats", acc.motion_beats_sum)
    assert acc.num_beats == solo_acc.num_beats >= 10 and acc.motion_beats_sum == solo_acc.motion_beats_sum > 0
    assert abs(got["bc"] - solo_acc.score()) <= 1e-12
    dev = long_form.score_timeline(torch.from_numpy(tl).cuda(), torch.from_numpy(audio).cuda(), frames=SCORE_FRAMES,
                                   audio_lengths=SCORE_LENGTHS)
    assert dev["bc"] == got["bc"] and dev["pose"].is_cuda and np.array_equal(host(dev["pose"]), got["pose"])


def test_score_timeline_beat_against_per_clip_calls():
    rows = [synthetic("beat", 1, n) for n in SCORE_FRAMES]
    tl, audio = padded([r[0] for r in rows], 131), score_audio()
    plain = long_form.score_timeline(tl, audio, dataset="beat", frames=SCORE_FRAMES, audio_lengths=SCORE_LENGTHS)
    assert set(plain) == {"pred_euler", "beat_mask", "align"}
    solo_pred = [pp.beat_postprocess_timeline(r)["pred_euler"] for r in rows]
    parts = [seeded_target(p, 500 + b) for b, p in enumerate(solo_pred)]
    target = padded([t[0] for t, _ in parts], 131, axis=0)
    semantic = padded([s[0] for _, s in parts], 131, axis=0)
    got = long_form.score_timeline(tl, audio, dataset="beat", target_euler=target, semantic=semantic, frames=SCORE_FRAMES,
                                   audio_lengths=SCORE_LENGTHS)
    assert np.array_equal(got["align"], plain["align"])
    sums = []
    for b, (r, L) in enumerate(zip(rows, SCORE_LENGTHS)):
        s = long_form.score_timeline(r, audio[b:b + 1, :L], dataset="beat", target_euler=parts[b][0], semantic=parts[b][1])
        n = SCORE_FRAMES[b]
        assert got["align"].dtype == s["align"].dtype and got["align"][b] == s["align"][0] and np.isfinite(s["align"][0]), b
        assert np.array_equal(got["pred_euler"][b, :n], s["pred_euler"][0]) and not got["pred_euler"][b, n:].any()
        assert np.array_equal(got["beat_mask"][b, :, :n - 1], s["beat_mask"][0]) and not got["beat_mask"][b, :, n - 1:].any()
        sums.append(bm.beat_metrics_timeline(solo_pred[b], parts[b][0], parts[b][1], want=("srgr_sum",))["srgr_sum"][0])
    want = float(np.array(sums, np.float32).astype(np.float64).sum()) / (sum(SCORE_FRAMES) * 47)
    print("srgr", got["srgr"], "from the solo sums", want)
    assert got["srgr"] == want and want > 0


# ---- sample_long -----------------------------------------------------------------------------------------------------------------------
def test_sample_long_with_audio_lengths_is_the_zero_tailed_call():
    from test_gpu_long_form import _inputs, _long, _parts
    cfg, model, diffusion, sampler, skip = _parts("ted", "ddim")
    y = _inputs(cfg, 2, 2)
    L = int(y["audio"].shape[1])
    lengths = [int(cfg.audio_len) - 100, L]
    assert long_form.plan_lengths(lengths, cfg) == [(1, 34), (2, 64)]
    zero_tailed = y["audio"].clone()
    zero_tailed[0, lengths[0]:] = 0
    y["audio"][0, lengths[0]:] = float("nan")            # what follows a clip's valid samples is never looked at
    before = y["audio"].clone()
    torch.manual_seed(21)
    tl, frames = _long(diffusion, model, y, sampler, skip, audio_lengths=lengths)
    assert torch.equal(torch.nan_to_num(y["audio"], nan=7.0), torch.nan_to_num(before, nan=7.0))        # the caller's tensor is untouched
    assert isinstance(frames, np.ndarray) and frames.dtype == np.int32 and frames.tolist() == [f for _, f in long_form.plan_lengths(lengths, cfg)]
    assert tl.is_cuda and tuple(tl.shape) == (2, cfg.njoints, cfg.nfeats, 64) and bool(torch.isfinite(tl).all())
    assert not bool(tl[0, :, :, 34:].any())
    torch.manual_seed(21)
    want = _long(diffusion, model, dict(y, audio=zero_tailed), sampler, skip, n_windows=2)
    assert torch.equal(tl[0, :, :, :34], want[0, :, :, :34]) and torch.equal(tl[1], want[1])
    assert bool(want[0, :, :, 34:].any())                # the tail that was cut held frames
    torch.manual_seed(21)
    tl2, frames2, wins = _long(diffusion, model, y, sampler, skip, audio_lengths=lengths, return_windows=True)
    assert torch.equal(tl2, tl) and np.array_equal(frames2, frames) and tuple(wins.shape) == (2, 2, cfg.njoints, cfg.nfeats, 34)
    res = long_form.score_timeline(tl, y["audio"], frames=frames, audio_lengths=lengths)                # the pair sample_long hands over
    assert tuple(res["pose"].shape) == (2, 64, 10, 3) and not bool(res["pose"][0, 34:].any())
