"""The timeline kernels on the GPU (csrc/ls_timeline.hip: ls_ted_post_timeline, ls_beat_post_timeline, ls_beat_metrics_timeline,
ls_ted_beat_align) and the Python chain above them.

Three yardsticks.  (1) The 34-frame kernels, which are pinned to the reference (G9, G10, G21): at N = 34 and on every 34-frame slice of
a timeline the new kernels must give their bits -- no tolerance.  (2) The float64 restatement (tests/timeline_restatement.py) on the
reference-generated G22 timelines, with the tolerances the 34-frame tests use.  (3) The kernels' own outputs: a mask is an exact
function of the fp32 curve next to it, so it is recomputed from that curve in numpy and must be equal everywhere, ends included.
Synthetic timelines have N in {34, tile - 1, tile, tile + 1, 2 tile + 3} and B in {1, 3}: where tiles and halos can go wrong."""
import ctypes as C

import numpy as np
import pytest
import torch

import beat_metrics_restatement as R
import timeline_restatement as T
from livelyspeaker_amd import _lib, beat_metrics as bm, long_form, postprocess as pp
from test_gpu_beat_metrics import ALIGN_TOL

pytestmark = pytest.mark.gpu
TILE = pp.TIMELINE_TILE
SIZES = [34, TILE - 1, TILE, TILE + 1, 2 * TILE + 3]
TED_KEYS = ("aligned_motions", "pose", "angle_diff", "beat_mask")
MET_KEYS = ("success", "srgr_sum", "vel", "beat_mask", "align")


def host(v):
    return v.detach().cpu().numpy() if hasattr(v, "detach") else np.asarray(v)


def circ_deg(a, b):
    return float(np.abs((np.asarray(a, np.float64) - np.asarray(b, np.float64) + 180.0) % 360.0 - 180.0).max())


def slices(x):
    """Every 34-frame slice of [B, ..., N] as one batch [S * B, ..., 34], slice-major."""
    N = x.shape[-1]
    return np.ascontiguousarray(np.concatenate([x[..., s:s + 34] for s in range(N - 33)]))


def seeded_onsets(B, seconds, seed):
    rng = np.random.default_rng(seed)
    return [np.sort(rng.uniform(0.0, seconds, size=int(rng.integers(3, 12)))).astype(np.float32) for _ in range(B)]


def seeded_target(pred, seed):
    rng = np.random.default_rng(seed)
    target = (pred + 1.2 * rng.standard_normal(pred.shape)).astype(np.float32)        # |d| sums straddle the threshold 4
    semantic = (rng.integers(0, 11, size=pred.shape[:2]) / 10.0).astype(np.float32)
    return target, semantic


def success_fp32(pred, target, J, threshold=np.float32(4.0)):
    """k_beat_metrics's success expression in numpy fp32: exact."""
    d = np.abs(pred - target).reshape(pred.shape[0], pred.shape[1], J, 3)
    return ((d[..., 0] + d[..., 1]) + d[..., 2]) < threshold


def check_ted_against_34_frame_kernel(tl, got):
    """Bit for bit on every slice: everything a 34-frame clip can know."""
    B, N = tl.shape[0], tl.shape[3]
    old = pp.ted_postprocess(slices(tl))
    for s in range(N - 33):
        rows = slice(s * B, s * B + B)
        assert np.array_equal(old["aligned_motions"][rows], got["aligned_motions"][:, s:s + 34]), s
        assert np.array_equal(old["pose"][rows], got["pose"][:, s:s + 34]), s
        assert np.array_equal(old["angle_diff"][rows][:, 1:], got["angle_diff"][:, s + 1:s + 34]), s
        assert np.array_equal(old["beat_mask"][rows][:, 2:33], got["beat_mask"][:, s + 2:s + 33]), s


def check_beat_against_34_frame_kernels(tl, post, met, order=2):
    B, J, N = tl.shape[0], tl.shape[1], tl.shape[3]
    old = pp.beat_postprocess(slices(tl))
    oldm = bm.beat_metrics(old["pred_euler"], joints=J, order=order, want=("vel", "beat_mask"))
    for s in range(N - 33):
        rows = slice(s * B, s * B + B)
        assert np.array_equal(old["decoded_motions"][rows], post["decoded_motions"][:, s:s + 34]), s
        assert np.array_equal(old["pred_euler"][rows], post["pred_euler"][:, s:s + 34]), s
        assert np.array_equal(oldm["vel"][rows], met["vel"][:, :, s:s + 33]), s
        assert np.array_equal(oldm["beat_mask"][rows][:, :, order:33 - order], met["beat_mask"][:, :, s + order:s + 33 - order]), s


def check_masks_from_own_curves(ted, met, order=2):
    """The masks are exact functions of the fp32 curves the same call returned."""
    if ted is not None:
        assert np.array_equal(host(ted["beat_mask"]), T.ted_beat_mask(host(ted["angle_diff"]), pp.TED_BEAT_THRES))
        assert not host(ted["angle_diff"])[:, 0].any()
    if met is not None:
        vel = host(met["vel"])
        want = np.stack([R.beat_masks(v, order) for v in vel])
        assert np.array_equal(host(met["beat_mask"]).astype(bool), want)


# ---- 4. the new kernels against the 34-frame kernels, bit for bit ---------------------------------------------------------------------
def test_at_34_frames_every_output_is_the_34_frame_entry_points(golden):
    s = golden["ted"]["G5_ddpm1000_final"]
    old, new = pp.ted_postprocess(s), pp.ted_postprocess_timeline(s)
    for k in TED_KEYS:
        assert np.array_equal(old[k], new[k]), k
    assert old["motion_beat_times"] == new["motion_beat_times"] and new["beat_mask"].sum() > 0
    s = golden["beat"]["G3_ddpm50_final"]
    old, new = pp.beat_postprocess(s), pp.beat_postprocess_timeline(s)
    for k in ("decoded_motions", "pred_euler"):
        assert np.array_equal(old[k], new[k]), k
    g21 = dict(np.load(R.GOLDEN))
    onsets = np.split(g21["onset_times"], g21["onset_offsets"][1:-1])
    for order in (1, 2, 3):
        args = (g21["pred_euler"], g21["target_euler"], g21["semantic"], onsets)
        old, new = bm.beat_metrics(*args, order=order), bm.beat_metrics_timeline(*args, order=order)
        assert set(old) == set(new) == set(MET_KEYS)
        for k in MET_KEYS:
            assert old[k].dtype == new[k].dtype and np.array_equal(old[k], new[k]), (order, k)


@pytest.fixture(scope="module")
def ted_runs():
    """case -> (timeline, kernel outputs on host inputs); computed once and left unchanged."""
    return {case: (tl, pp.ted_postprocess_timeline(tl)) for case, tl in T.g22("ted").items()}


@pytest.fixture(scope="module")
def beat_runs():
    """case -> (timeline, post, onsets, target, semantic, metrics)."""
    out = {}
    for i, (case, tl) in enumerate(T.g22("beat").items()):
        post = pp.beat_postprocess_timeline(tl)
        onsets = seeded_onsets(tl.shape[0], 94 / 15.0, 40 + i)
        target, semantic = seeded_target(post["pred_euler"], 50 + i)
        out[case] = (tl, post, onsets, target, semantic, bm.beat_metrics_timeline(post["pred_euler"], target, semantic, onsets))
    return out


@pytest.mark.parametrize("case", T.CASES)
def test_every_slice_of_the_g22_timelines_is_the_34_frame_kernels(case, ted_runs, beat_runs):
    check_ted_against_34_frame_kernel(*ted_runs[case])
    tl, post, _, _, _, met = beat_runs[case]
    check_beat_against_34_frame_kernels(tl, post, met)


# ---- 5. against the restatement on the reference-generated timelines -------------------------------------------------------------------
@pytest.mark.parametrize("case", T.CASES)
def test_ted_g22_against_the_restatement(case, ted_runs):
    tl, got = ted_runs[case]
    want = T.ted_post(tl)
    assert got["aligned_motions"].shape == (2, 94, 27) and got["pose"].shape == (2, 94, 10, 3) and got["beat_mask"].dtype == bool
    assert np.array_equal(got["aligned_motions"], want["aligned"])
    dp, dd = np.abs(got["pose"] - want["pose"]).max(), np.abs(got["angle_diff"] - want["angle_diff"]).max()
    print(case, "pose max|d|", dp, "angle_diff max|d|", dd, "beats", got["beat_mask"].sum(1), "smallest decision margin",
          T.ted_beat_margin(want["angle_diff"], pp.TED_BEAT_THRES).min())
    assert dp < 1e-5 and dd < 2e-3
    assert np.array_equal(got["beat_mask"], want["beat_mask"]) and got["beat_mask"].sum(1).min() >= 20      # no frame left out
    assert got["motion_beat_times"] == [[float(t) / 15.0 for t in np.nonzero(m)[0]] for m in want["beat_mask"]]
    check_masks_from_own_curves(got, None)


@pytest.mark.parametrize("case", T.CASES)
def test_beat_g22_against_the_restatement(case, beat_runs):
    from oracle import rag_oracle as orc
    tl, post, onsets, target, semantic, got = beat_runs[case]
    o = orc.beat_post(tl)
    assert np.array_equal(post["decoded_motions"], o["decoded_motions"])
    de = circ_deg(post["pred_euler"], o["pred_euler"])
    want = T.score_batch(o["pred_euler"], None, None, onsets)
    dv = np.abs(got["vel"] - want["vel"]).max()
    margin = np.stack([[R.minima_margin(v) for v in clip] for clip in want["vel"]])
    excl = margin < R.BEAT_MARGIN
    excl[:, :, [0, -1]] = False                        # an end frame is compared with itself: never a beat, whatever the rounding
    print(case, "euler circular max|d|", de, "vel max|d|", dv, "frames left out", int(excl.sum()), "of", excl.size, "beats per series",
          want["beat_mask"].sum(2).min(), "-", want["beat_mask"].sum(2).max())
    assert de < 5e-3 and dv < R.VEL_TOL
    mask = got["beat_mask"].astype(bool)
    if case == "G22_ddim100_skip95_timeline":
        assert np.array_equal(mask, want["beat_mask"])
        clean = np.ones(2, bool)
    else:
        assert excl.sum() <= 0.01 * excl.size and np.array_equal(mask[~excl], want["beat_mask"][~excl])
        clean = ~excl[:, 2].any(1)
    da = np.abs(got["align"] - want["align"])
    print("align", got["align"], "restatement", want["align"], "compared", clean)
    assert (da[clean] < ALIGN_TOL).all()
    # SRGR on the kernel's own planes: the success bits are an exact fp32 expression, the sum a fixed tree of about 20 roundings
    ok = success_fp32(post["pred_euler"], target, 47)
    assert np.array_equal(got["success"].astype(bool), ok) and 0.05 < ok.mean() < 0.95
    ref = T.srgr_clip_sums(ok, semantic)
    assert (np.abs(got["srgr_sum"] - ref) <= 1e-5 * ref).all()
    check_masks_from_own_curves(None, got)


# ---- 6. tiles, halos, batch ----------------------------------------------------------------------------------------------------------
def synthetic(ds, B, N):
    rng = np.random.default_rng(1000 * N + B + (7 if ds == "beat" else 0))
    if ds == "ted":       # a random walk around 0: direction vectors that move like gestures, so the change curve has beats
        return np.cumsum(0.05 * rng.standard_normal((B, 9, 3, N)), axis=3).astype(np.float32)
    return (np.array([1, 0, 0, 0, 1, 0], np.float32)[None, None, :, None] + np.cumsum(0.08 * rng.standard_normal((B, 47, 6, N)), axis=3)).astype(np.float32)


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("N", SIZES)
def test_ted_tile_edges(N, B):
    tl = synthetic("ted", B, N)
    got = pp.ted_postprocess_timeline(tl)
    assert got["pose"].shape == (B, N, 10, 3)
    check_ted_against_34_frame_kernel(tl, got)
    check_masks_from_own_curves(got, None)
    assert got["beat_mask"].sum() > 0 and not got["beat_mask"][:, [0, 1, N - 1]].any()
    want = T.ted_post(tl)
    assert np.array_equal(got["aligned_motions"], want["aligned"])
    assert np.abs(got["pose"] - want["pose"]).max() < 1e-5       # the curve is tied to the 34-frame kernel above, bit for bit
    alone = pp.ted_postprocess_timeline(tl[B - 1:])
    for k in TED_KEYS:
        assert np.array_equal(alone[k], got[k][B - 1:]), k


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("N", SIZES)
def test_beat_tile_edges(N, B):
    tl = synthetic("beat", B, N)
    post = pp.beat_postprocess_timeline(tl)
    onsets = seeded_onsets(B, N / 15.0, N)
    target, semantic = seeded_target(post["pred_euler"], N + 1)
    got = bm.beat_metrics_timeline(post["pred_euler"], target, semantic, onsets)
    assert got["vel"].shape == (B, 6, N - 1) and got["success"].shape == (B, N, 47)
    check_beat_against_34_frame_kernels(tl, post, got)
    check_masks_from_own_curves(None, got)
    assert got["beat_mask"].sum() > 0
    ok = success_fp32(post["pred_euler"], target, 47)
    assert np.array_equal(got["success"].astype(bool), ok)
    ref = T.srgr_clip_sums(ok, semantic)
    assert (np.abs(got["srgr_sum"] - ref) <= 1e-5 * ref).all()
    want = np.array([R.gahr(np.nonzero(got["beat_mask"][b, 2])[0] / 15, onsets[b]) for b in range(B)])
    assert np.abs(got["align"] - want).max() < ALIGN_TOL
    alone = bm.beat_metrics_timeline(post["pred_euler"][B - 1:], target[B - 1:], semantic[B - 1:], onsets[B - 1:])
    for k in MET_KEYS:
        assert np.array_equal(alone[k], got[k][B - 1:]), k
    if N == SIZES[-1]:                                  # a wider halo than the tile's neighbours: order 40 reaches across two tiles
        for order in (1, 40):
            wide = bm.beat_metrics_timeline(post["pred_euler"], order=order, want=("vel", "beat_mask"))
            check_masks_from_own_curves(None, wide, order=order)
            assert np.array_equal(wide["vel"], got["vel"])


def test_a_prefix_of_tile_plus_one_frames_reproduces_the_full_run(ted_runs, beat_runs):
    P = TILE + 1
    for tl, full in list(ted_runs.values())[:1] + [(t, pp.ted_postprocess_timeline(t)) for t in [synthetic("ted", 3, SIZES[-1])]]:
        cut = pp.ted_postprocess_timeline(np.ascontiguousarray(tl[..., :P]))
        for k in ("aligned_motions", "pose", "angle_diff"):
            assert np.array_equal(cut[k], full[k][:, :P]), k
        assert np.array_equal(cut["beat_mask"][:, :P - 1], full["beat_mask"][:, :P - 1]) and not cut["beat_mask"][:, P - 1].any()
    tl, post, _, _, _, full = beat_runs[T.CASES[0]]
    cut_post = pp.beat_postprocess_timeline(np.ascontiguousarray(tl[..., :P]))
    for k in ("decoded_motions", "pred_euler"):
        assert np.array_equal(cut_post[k], post[k][:, :P]), k
    cut = bm.beat_metrics_timeline(cut_post["pred_euler"], want=("vel", "beat_mask"))
    assert np.array_equal(cut["vel"], full["vel"][:, :, :P - 1])
    assert np.array_equal(cut["beat_mask"][:, :, :P - 3], full["beat_mask"][:, :, :P - 3])       # order 2 away from the cut


def test_256_device_resident_clips_reproduce_the_two_clip_call(ted_runs, beat_runs):
    tile = lambda a: torch.from_numpy(np.tile(a, (128,) + (1,) * (a.ndim - 1))).cuda()        # noqa: E731
    tl, base = ted_runs[T.CASES[0]]
    got = pp.ted_postprocess_timeline(tile(tl))
    for k in TED_KEYS:
        assert got[k].is_cuda and got[k].shape[0] == 256, k
        assert np.array_equal(host(got[k][:2]), base[k]) and np.array_equal(host(got[k][254:]), base[k]), k
    assert got["motion_beat_times"][255] == base["motion_beat_times"][1]
    tl, post, onsets, target, semantic, base = beat_runs[T.CASES[0]]
    gp = pp.beat_postprocess_timeline(tile(tl))
    for k in ("decoded_motions", "pred_euler"):
        assert gp[k].is_cuda and np.array_equal(host(gp[k][:2]), post[k]) and np.array_equal(host(gp[k][254:]), post[k]), k
    got = bm.beat_metrics_timeline(gp["pred_euler"], tile(target), tile(semantic), onsets * 128)
    for k in MET_KEYS:
        assert got[k].is_cuda and got[k].shape[0] == 256, k
        assert np.array_equal(host(got[k][:2]), base[k]) and np.array_equal(host(got[k][254:]), base[k]), k


# ---- 7. the TED beat-consistency sums against BeatConsistency.push --------------------------------------------------------------------
@pytest.fixture(scope="module")
def align_case(ted_runs):
    masks = np.concatenate([got["beat_mask"] for _, got in ted_runs.values()] + [np.zeros((1, 94), bool)])      # clip 6: no beat
    counts = [12, 0, 1, 20, 7, 24, 9]                   # no onset, one onset, a full row
    slab, count = T.onset_slab(np.random.default_rng(77), 7, 24, counts, 400)        # frames to 12.8 s: past the last pose (6.3 s)
    return masks, slab, count


def test_ted_beat_align_against_the_host_accumulator(align_case):
    masks, slab, count = align_case
    times = T.slab_times(slab, count)
    beats = [[float(t) / 15.0 for t in np.nonzero(m)[0]] for m in masks]
    assert (slab[0, :12] * 512 / 16000.0).max() > 94 / 15.0
    total, n = pp.ted_beat_align(masks, slab, count)
    assert total.dtype == np.float64 and np.array_equal(n, masks.sum(1)) and n[6] == 0 and total[6] == 0.0 and total[1] == 0.0
    for b in range(7):
        one = pp.BeatConsistency()
        one.push(beats[b:b + 1], times[b:b + 1])
        print(b, "count", count[b], "beats", n[b], "device", total[b], "host", one.align_sum)
        assert abs(total[b] - one.align_sum) <= 1e-12 * max(1, count[b]), b
    dev_total, dev_n = pp.ted_beat_align(torch.from_numpy(masks).cuda(), torch.from_numpy(slab).cuda(), torch.from_numpy(count).cuda())
    assert np.array_equal(dev_total, total) and np.array_equal(dev_n, n)
    want, got = pp.BeatConsistency(), pp.BeatConsistency()
    want.push(beats, times)
    got.push_timeline(torch.from_numpy(masks).cuda(), torch.from_numpy(slab).cuda(), torch.from_numpy(count).cuda())
    assert (got.num_beats, got.motion_beats_sum) == (want.num_beats, want.motion_beats_sum) == (int(count[:6].sum()), int(masks.sum()))
    assert abs(got.score() - want.score()) <= 1e-12
    other = pp.BeatConsistency(sigma=0.25)              # sigma reaches the kernel
    other.push_timeline(masks, slab, count)
    ref = pp.BeatConsistency(sigma=0.25)
    ref.push(beats, times)
    assert abs(other.score() - ref.score()) <= 1e-12 and abs(other.score() - want.score()) > 1e-3


# ---- 8. nullable outputs, host and device inputs, end to end --------------------------------------------------------------------------
def test_host_and_device_inputs_agree_bitwise(ted_runs, beat_runs):
    tl, base = ted_runs[T.CASES[1]]
    got = pp.ted_postprocess_timeline(torch.from_numpy(tl).cuda())
    for k in TED_KEYS:
        assert got[k].is_cuda and np.array_equal(host(got[k]), base[k]), k
    assert got["motion_beat_times"] == base["motion_beat_times"]
    got = pp.ted_postprocess_timeline(torch.from_numpy(tl))              # a CPU tensor is a host input
    assert isinstance(got["pose"], np.ndarray) and np.array_equal(got["pose"], base["pose"])
    tl, post, onsets, target, semantic, base = beat_runs[T.CASES[1]]
    gp = pp.beat_postprocess_timeline(torch.from_numpy(tl).cuda())
    assert all(np.array_equal(host(gp[k]), post[k]) for k in post)
    got = bm.beat_metrics_timeline(gp["pred_euler"], torch.from_numpy(target).cuda(), torch.from_numpy(semantic).cuda(), onsets)
    for k in MET_KEYS:
        assert got[k].is_cuda and np.array_equal(host(got[k]), base[k]), k


def test_every_nullable_output_left_out_in_turn(ted_runs, beat_runs, align_case):
    lib = _lib.load_library()
    tl, base = ted_runs[T.CASES[2]]
    B, N = tl.shape[0], tl.shape[3]
    cfg = pp.ted_post_config()
    shapes = {"aligned_motions": ((B, N, 27), np.float32), "pose": ((B, N, 10, 3), np.float32), "angle_diff": ((B, N), np.float32),
              "beat_mask": ((B, N), np.uint8)}
    for left_out in TED_KEYS:
        outs = {k: np.empty(*shapes[k]) for k in TED_KEYS if k != left_out}
        ptr = [outs[k].ctypes.data_as(C.c_void_p) if k in outs else None for k in TED_KEYS]
        assert lib.ls_ted_post_timeline(0, 0, B, N, C.byref(cfg), tl.ctypes.data_as(C.c_void_p), *ptr) == 0
        for k, v in outs.items():
            assert np.array_equal(v, base[k]), (left_out, k)
    no_pose = pp.ted_postprocess_timeline(tl, want_pose=False)
    assert no_pose["pose"] is None and np.array_equal(no_pose["beat_mask"], base["beat_mask"])
    tl, post, onsets, target, semantic, base = beat_runs[T.CASES[2]]
    only_dec = pp.beat_postprocess_timeline(tl, want_euler=False)
    assert only_dec["pred_euler"] is None and np.array_equal(only_dec["decoded_motions"], post["decoded_motions"])
    eul = np.empty((2, 94, 141), np.float32)
    assert lib.ls_beat_post_timeline(0, 0, 2, 47, 94, tl.ctypes.data_as(C.c_void_p), None, eul.ctypes.data_as(C.c_void_p)) == 0
    assert np.array_equal(eul, post["pred_euler"])
    p = post["pred_euler"]
    for name in MET_KEYS:
        got = bm.beat_metrics_timeline(p, target, semantic, onsets, want=(name,))
        assert set(got) == {name} and np.array_equal(got[name], base[name]), name
        rest = tuple(n for n in MET_KEYS if n != name)
        got = bm.beat_metrics_timeline(p, target, semantic, onsets, want=rest)
        assert set(got) == set(rest) and all(np.array_equal(got[n], base[n]) for n in rest), name
    got = bm.beat_metrics_timeline(torch.from_numpy(p).cuda(), torch.from_numpy(target).cuda(), None, onsets, want=("srgr_sum", "align"))
    assert np.array_equal(host(got["align"]), base["align"])           # device inputs, both masks left out: temporaries hold them
    want = base["success"].reshape(2, -1).sum(1) * R.SRGR_SCALE
    assert (np.abs(host(got["srgr_sum"]) - want) <= 1e-5 * want).all()
    masks, slab, count = align_case
    total, n = pp.ted_beat_align(masks, slab, count)
    a = _lib.LsTedAlignArgs()
    a.batch, a.n_frames, a.on_device, a.onset_cols, a.hop, a.fps, a.sigma, a.sr = 7, 94, 0, 24, 512, 15.0, pp.TED_BEAT_SIGMA, 16000.0
    m8 = np.ascontiguousarray(masks, np.uint8)
    a.beat_mask, a.onset_frames, a.onset_count = m8.ctypes.data, slab.ctypes.data, count.ctypes.data
    t2, n2 = np.empty(7, np.float64), np.empty(7, np.int32)
    a.align_sum = t2.ctypes.data
    assert lib.ls_ted_beat_align(0, C.byref(a)) == 0 and np.array_equal(t2, total)
    a.align_sum, a.n_beats = None, n2.ctypes.data
    assert lib.ls_ted_beat_align(0, C.byref(a)) == 0 and np.array_equal(n2, n)


def test_score_timeline_end_to_end_on_a_sampled_timeline():
    from test_gpu_long_form import _inputs, _long, _parts
    cfg, model, diffusion, sampler, skip = _parts("ted", "ddim")
    y = _inputs(cfg, 2, 3)
    rng = np.random.default_rng(9)
    audio = 0.01 * rng.standard_normal(tuple(y["audio"].shape)).astype(np.float32)
    audio[:, ::6400] += 0.9                              # a click every 0.4 s, so that onsets exist
    y["audio"] = torch.from_numpy(audio).cuda()
    torch.manual_seed(5)
    tl = _long(diffusion, model, y, sampler, skip, n_windows=3)
    assert tl.is_cuda and tuple(tl.shape) == (2, 9, 3, 94)
    res = long_form.score_timeline(tl, y["audio"])
    assert set(res) == {"pose", "beat_mask", "motion_beat_times", "bc"} and tuple(res["pose"].shape) == (2, 94, 10, 3) and res["pose"].is_cuda
    post = pp.ted_postprocess_timeline(tl)
    assert res["motion_beat_times"] == post["motion_beat_times"] and torch.equal(res["beat_mask"], post["beat_mask"])
    want = pp.BeatConsistency()
    want.push(post["motion_beat_times"], audio=y["audio"])
    print("bc", res["bc"], "host", want.score(), "onsets", want.num_beats, "motion beats", want.motion_beats_sum)
    assert want.num_beats >= 10 and want.motion_beats_sum > 0
    assert abs(res["bc"] - want.score()) <= 1e-12
    host_res = long_form.score_timeline(host(tl), audio)                   # numpy inputs: the same bits
    assert host_res["bc"] == res["bc"] and np.array_equal(host_res["pose"], host(res["pose"]))
    # BEAT: the chain on a reference-generated timeline, against its pieces
    btl = T.g22("beat")[T.CASES[0]]
    baudio = np.ascontiguousarray(audio[:, :96000])
    got = long_form.score_timeline(btl, baudio, dataset="beat")
    assert set(got) == {"pred_euler", "beat_mask", "align"} and got["align"].shape == (2,) and np.isfinite(got["align"]).all()
    target, semantic = seeded_target(got["pred_euler"], 3)
    got2 = long_form.score_timeline(btl, baudio, dataset="beat", target_euler=target, semantic=semantic)
    assert np.array_equal(got2["align"], got["align"])
    ok = success_fp32(got["pred_euler"], target, 47)
    want_rate = T.srgr_clip_sums(ok, semantic).sum() / (2 * 94 * 47)
    assert abs(got2["srgr"] - want_rate) <= 1e-5 * want_rate
