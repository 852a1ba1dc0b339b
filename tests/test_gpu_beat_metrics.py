"""ls_beat_metrics / ls_beat_ldiv and BeatEvaluator on the GPU: fixture G21 (the reference's own numbers, tests/golden/
make_golden_beat_metrics.py) through the kernels and through the whole chain from the rot6d tensors, then the shapes at which the
kernels can go wrong against the float64 restatement (tests/beat_metrics_restatement.py, pinned to G21 by test_beat_metrics_host.py).

Tolerances.  Masks are compared outside the fixture's exclusion masks (comparisons closer than the Euler / velocity tolerance, which
fp32 rounding may flip).  vel: 0.0175 degrees (sqrt(3) * 1e-2).  srgr_sum: 1e-5 relative (about 20 fp32 roundings in a fixed tree) plus
what the clip's excluded entries can weigh.  align: 2e-5 absolute (the exponent reaches about 27, so its fp32 relative error is about
5e-6, plus expf).  Against the restatement on the SAME fp32 planes only the kernel's own rounding separates the two: a velocity is off
by at most ~1.2e-4 (2e-7 relative of values up to 600) and a summed difference by ~1e-4, so comparisons closer than 1e-3 are left out."""
import numpy as np
import pytest

import beat_metrics_restatement as R

pytestmark = pytest.mark.gpu

SAME_PLANE_MARGIN = 1e-3
ALIGN_TOL = 2e-5


@pytest.fixture(scope="module")
def g21():
    return dict(np.load(R.GOLDEN))


@pytest.fixture(scope="module")
def onsets(g21):
    return np.split(g21["onset_times"], g21["onset_offsets"][1:-1])


@pytest.fixture(scope="module")
def base(g21, onsets):
    """The 4-clip host call every test compares with; computed once and left unchanged."""
    from livelyspeaker_amd import beat_metrics as bm
    return bm.beat_metrics(g21["pred_euler"], g21["target_euler"], g21["semantic"], onsets)


def host(v):
    return v.detach().cpu().numpy() if hasattr(v, "detach") else np.asarray(v)


def check_against_g21(got, g21, clips=slice(None)):
    keep = ~g21["srgr_excluded"][clips]
    assert np.array_equal(host(got["success"]).astype(bool)[keep], g21["success"][clips][keep])
    dv = np.abs(host(got["vel"]) - g21["vel"][clips]).max()
    print("vel max|d| (deg)", dv)
    assert dv < R.VEL_TOL
    keep = ~g21["beat_excluded"][clips]
    assert np.array_equal(host(got["beat_mask"]).astype(bool)[keep], g21["beat_mask"][clips][keep])
    sem = g21["semantic"][clips]
    ref = R.srgr_clip_sums(g21["success"][clips], sem)
    slack = g21["srgr_excluded"][clips].reshape(len(ref), -1).sum(1) * sem.max() * R.SRGR_SCALE
    ds = np.abs(host(got["srgr_sum"]) - ref)
    print("srgr_sum", host(got["srgr_sum"]), "reference", ref, "slack", slack)
    assert (ds <= 1e-5 * np.abs(ref) + slack).all()
    clean = ~g21["beat_excluded"][clips][:, 2].any(1)
    da = np.abs(host(got["align"]) - g21["align"][clips])
    print("align", host(got["align"]), "reference", g21["align"][clips], "compared", clean)
    assert clean.sum() >= min(3, len(clean)) and (da[clean] < ALIGN_TOL).all()


def check_against_restatement(got, want, threshold=R.SRGR_THRESHOLD, order=R.ORDER, align_series=2, semantic_max=1.0):
    if "success" in want:
        excl = np.abs(want["diff"] - threshold) < SAME_PLANE_MARGIN
        assert np.array_equal(host(got["success"]).astype(bool)[~excl], want["success"][~excl])
        slack = excl.reshape(len(excl), -1).sum(1) * semantic_max * R.SRGR_SCALE
        assert (np.abs(host(got["srgr_sum"]) - want["srgr_sum"]) <= 1e-5 * np.abs(want["srgr_sum"]) + slack).all()
    assert np.abs(host(got["vel"]) - want["vel"]).max() < SAME_PLANE_MARGIN
    excl = np.stack([[R.minima_margin(v, order) for v in clip] for clip in want["vel"]]) < SAME_PLANE_MARGIN
    excl[:, :, [0, -1]] = False
    assert np.array_equal(host(got["beat_mask"]).astype(bool)[~excl], want["beat_mask"][~excl])
    if "align" in got:
        clean = ~excl[:, align_series].any(1)
        assert clean.any() and (np.abs(host(got["align"]) - want["align"])[clean] < ALIGN_TOL).all()


def test_g21_through_ls_beat_metrics(base, g21):
    assert base["success"].dtype == np.uint8 and base["success"].shape == (4, 34, 47) and base["beat_mask"].shape == (4, 6, 33)
    assert set(np.unique(base["success"])) <= {0, 1} and set(np.unique(base["beat_mask"])) <= {0, 1}
    assert not base["beat_mask"][:, :, [0, 32]].any()
    check_against_g21(base, g21)


def test_g21_through_the_evaluator_from_rot6d(g21, onsets, golden):
    import torch
    from livelyspeaker_amd import beat_metrics as bm
    from livelyspeaker_amd.postprocess import beat_postprocess
    sample = torch.from_numpy(golden["beat"]["G3_ddpm50_final"]).cuda()
    tar_pose = torch.from_numpy(g21["tar_pose"]).cuda()
    semantic = torch.from_numpy(g21["semantic"]).cuda()
    # the kernels on the planes ls_beat_post makes of the rot6d tensors, entry by entry
    pred = beat_postprocess(sample)["pred_euler"]
    target = beat_postprocess(tar_pose.reshape(4, 34, 47, 6).permute(0, 2, 3, 1))["pred_euler"]
    assert np.abs(host(target) - g21["target_euler"]).max() < 5e-3
    check_against_g21(bm.beat_metrics(pred, target, semantic, onsets), g21)
    # and the evaluator's accumulation of them
    ev = bm.BeatEvaluator()
    res = ev.push(sample, tar_pose, semantic, onsets)
    sc = ev.scores()
    rows = 4 * 34
    ref_sum = R.srgr_clip_sums(g21["success"], g21["semantic"]).sum()
    slack = g21["srgr_excluded"].sum() * g21["semantic"].max() * R.SRGR_SCALE
    print("srgr", sc["srgr"], "reference", float(g21["srgr_rate"]), "align", sc["align"], "reference", g21["align"].mean(), "l1div", sc["l1div"],
          "reference", float(g21["l1div_avg"]))
    assert abs(sc["srgr"] - g21["srgr_rate"]) <= (1e-5 * ref_sum + slack) / (rows * 47) and sc["srgr"] == res["srgr_rate"]
    assert not g21["beat_excluded"][:, 2].any()
    assert np.abs(res["align"] - g21["align"]).max() < ALIGN_TOL and abs(sc["align"] - g21["align"].sum() / 4) < ALIGN_TOL
    # on the planes ls_beat_post made, only ls_beat_ldiv's own rounding separates the evaluator from the restatement (1e-6, test_l1div)
    same = R.l1div_sum(host(pred).reshape(rows, 141)) / rows
    assert abs(sc["l1div"] - same) <= 1e-6 * same
    # against the reference: every angle within 5e-3 degrees of the reference's, and so is every column mean, so an element's
    # |x - mean| moves by at most 1e-2; these are rounding differences of either sign, so the sum over 136 * 141 elements is a
    # random walk with sigma <= 1e-2 * sqrt(136 * 141) = 1.38, bounded at five sigma and divided by the 136 rows: 0.051
    assert abs(sc["l1div"] - g21["l1div_avg"]) < 5 * 1e-2 * np.sqrt(rows * 141) / rows
    assert sc["fid"] is None and sc["diversity"] is None and ev.total_length == 4
    ev.push(sample[:2], tar_pose[:2], semantic[:2], onsets[:2])             # a second batch: SRGR.avg() over both
    slack2 = (g21["srgr_excluded"].sum() + g21["srgr_excluded"][:2].sum()) * g21["semantic"].max() * R.SRGR_SCALE
    ref_sum2 = ref_sum + R.srgr_clip_sums(g21["success"][:2], g21["semantic"][:2]).sum()
    assert abs(ev.scores()["srgr"] - g21["srgr_avg"]) <= (1e-5 * ref_sum2 + slack2) / (6 * 34 * 47)
    assert ev.total_length == 6 and ev.srgr_calculator.counter == 6 * 34
    with pytest.raises(ValueError, match="clip 1"):
        ev.push(sample[:2], tar_pose[:2], semantic[:2], [onsets[0], []])
    assert ev.total_length == 6


def test_evaluator_features_fid_and_diversity(g21, golden):
    import torch
    from types import SimpleNamespace
    from livelyspeaker_amd import beat_metrics as bm, synth
    from livelyspeaker_amd.embedding_net import HalfEmbeddingNet
    from oracle import eval_oracle as evo
    sd = synth.make_embedding_net_state_dict(282, 48, seed=synth.SEED_WEIGHTS + 202, hidden=(4, 2))
    net = HalfEmbeddingNet(SimpleNamespace(pose_length=34, pose_dims=282, vae_length=48))
    net.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()})
    net = net.cuda().eval()
    sample = torch.from_numpy(golden["beat"]["G3_ddpm50_final"]).cuda()
    tar_pose = torch.from_numpy(g21["tar_pose"]).cuda()
    ev = bm.BeatEvaluator(eval_model=net)
    ev.push(sample, tar_pose)
    ev.push(sample[:3], tar_pose[:3])
    decoded = golden["beat"]["G3_ddpm50_final"].transpose(0, 3, 1, 2).reshape(4, 34, 282)
    want_out, want_ori = evo.pose_encoder(sd, decoded), evo.pose_encoder(sd, g21["tar_pose"])
    scale = float(np.abs(want_out).max())
    assert np.abs(ev.latent_out_all[0] - want_out).max() < 1e-4 * scale and np.abs(ev.latent_ori_all[0] - want_ori).max() < 1e-4 * scale
    assert ev.latent_out_all[1].shape == (3, 48) and np.abs(ev.latent_out_all[1] - want_out[:3]).max() < 1e-4 * scale
    torch.manual_seed(4)
    sc = ev.scores()
    torch.manual_seed(4)
    assert sc["diversity"] == bm.FIDCalculator.get_diversity(ev.latent_out_all)
    out, ori = np.concatenate(ev.latent_out_all), np.concatenate(ev.latent_ori_all)
    fid = bm.FIDCalculator.frechet_distance(out, ori)
    # 7 clips in 48 dimensions: both covariances have rank 6, so most eigenvalues of S1^(1/2) S2 S1^(1/2) are zeros computed to within
    # eps * tr(S1) * tr(S2), and the square root of such a zero is what the batch-merged and the one-pass moments may differ by:
    # 48 eigenvalues, the factor 2 of -2 Tr(.), two computations
    bound = 4 * 48 * np.sqrt(np.finfo(np.float64).eps * np.trace(np.cov(out, rowvar=False)) * np.trace(np.cov(ori, rowvar=False)))
    print("fid", sc["fid"], "one pass", fid, "bound", bound)
    assert abs(sc["fid"] - fid) <= bound and np.isfinite(fid) and bound < 1e-3 * fid
    assert sc["srgr"] == 0 and sc["align"] == 0.0 and ev.total_length == 7


def test_single_clip_and_single_onset(base, g21, onsets):
    from livelyspeaker_amd import beat_metrics as bm
    got = bm.beat_metrics(g21["pred_euler"][1:2], g21["target_euler"][1:2], g21["semantic"][1:2], onsets[1:2])
    for k, v in got.items():
        assert np.array_equal(v, base[k][1:2]), k
    one = bm.beat_metrics(g21["pred_euler"][:1], onset_times=[[0.7]], want=("align", "beat_mask"))
    assert set(one) == {"align", "beat_mask"} and np.array_equal(one["beat_mask"], base["beat_mask"][:1])
    times = np.nonzero(one["beat_mask"][0, 2])[0] / 15
    assert abs(one["align"][0] - R.gahr(times, [np.float32(0.7)])) < ALIGN_TOL


def test_constant_clip_scores_zero_and_succeeds_everywhere(base, g21, onsets):
    from livelyspeaker_amd import beat_metrics as bm
    const = np.full((1, 34, 141), 12.5, np.float32)
    pred = np.concatenate([g21["pred_euler"], const])
    target = np.concatenate([g21["target_euler"], const])
    semantic = np.concatenate([g21["semantic"], np.full((1, 34), 0.5, np.float32)])
    on = onsets + [np.array([0.2, 1.1], np.float32)]
    got = bm.beat_metrics(pred, target, semantic, on)
    for k, v in got.items():
        assert np.array_equal(v[:4], base[k]), k
    assert got["success"][4].all() and not got["beat_mask"][4].any() and not got["vel"][4].any() and got["align"][4] == 0.0
    assert abs(got["srgr_sum"][4] - 34 * 47 * 0.5 * R.SRGR_SCALE) <= 1e-5 * 34 * 47 * 0.5 * R.SRGR_SCALE
    check_against_restatement(got, R.score_batch(pred, target, semantic, on))


def test_256_device_resident_clips_reproduce_the_4_clip_call(base, g21, onsets):
    import torch
    from livelyspeaker_amd import beat_metrics as bm
    tile = lambda a: torch.from_numpy(np.tile(a, (64,) + (1,) * (a.ndim - 1))).cuda()        # noqa: E731
    got = bm.beat_metrics(tile(g21["pred_euler"]), tile(g21["target_euler"]), tile(g21["semantic"]), onsets * 64)
    assert set(got) == set(base)
    for k, v in got.items():
        assert v.is_cuda and v.shape[0] == 256, k
        assert np.array_equal(host(v[252:]), base[k]), k             # bit for bit: a clip's sums do not depend on the batch
        assert np.array_equal(host(v[:4]), base[k]), k


def test_host_and_device_inputs_agree_bitwise(base, g21, onsets):
    import torch
    from livelyspeaker_amd import beat_metrics as bm
    got = bm.beat_metrics(torch.from_numpy(g21["pred_euler"]).cuda(), torch.from_numpy(g21["target_euler"]).cuda(),
                          torch.from_numpy(g21["semantic"]).cuda(), onsets)
    for k, v in got.items():
        assert v.is_cuda and np.array_equal(host(v), base[k]), k


def test_every_nullable_argument_left_out_in_turn(base, g21, onsets):
    from livelyspeaker_amd import beat_metrics as bm
    p, t, s = g21["pred_euler"], g21["target_euler"], g21["semantic"]
    for name in ("success", "srgr_sum", "vel", "beat_mask", "align"):
        got = bm.beat_metrics(p, t, s, onsets, want=(name,))                   # one output alone
        assert set(got) == {name} and np.array_equal(got[name], base[name]), name
        rest = tuple(n for n in base if n != name)
        got = bm.beat_metrics(p, t, s, onsets, want=rest)                      # every output but one
        assert set(got) == set(rest) and all(np.array_equal(got[n], base[n]) for n in rest), name
    got = bm.beat_metrics(p, None, None, onsets)                               # no target: no SRGR
    assert set(got) == {"vel", "beat_mask", "align"} and all(np.array_equal(got[n], base[n]) for n in got)
    got = bm.beat_metrics(p, t, s, None)                                       # no onsets: no alignment
    assert set(got) == {"success", "srgr_sum", "vel", "beat_mask"} and all(np.array_equal(got[n], base[n]) for n in got)
    got = bm.beat_metrics(p, t, None, onsets)                                  # no semantic: every frame weighs 1
    assert np.array_equal(got["success"], base["success"])
    want = base["success"].reshape(4, -1).sum(1) * R.SRGR_SCALE
    assert (np.abs(got["srgr_sum"] - want) <= 1e-5 * want).all()


def test_a_clip_without_an_onset_is_refused(g21, onsets):
    from livelyspeaker_amd import beat_metrics as bm
    with pytest.raises(ValueError, match="clip 2"):
        bm.beat_metrics(g21["pred_euler"], onset_times=[onsets[0], onsets[1], np.zeros(0, np.float32), onsets[3]])
    with pytest.raises(ValueError, match="per clip"):
        bm.beat_metrics(g21["pred_euler"], onset_times=onsets[:3])


def test_six_joints_are_their_own_series(g21, onsets):
    from livelyspeaker_amd import beat_metrics as bm
    pred = np.ascontiguousarray(g21["pred_euler"][:, :, :18])
    target = np.ascontiguousarray(g21["target_euler"][:, :, :18])
    kw = dict(joints=6, series_joints=(0, 1, 2, 3, 4, 5), align_series=4)
    got = bm.beat_metrics(pred, target, g21["semantic"], onsets, **kw)
    assert got["success"].shape == (4, 34, 6)
    check_against_restatement(got, R.score_batch(pred, target, g21["semantic"], onsets, joints=6, series=(0, 1, 2, 3, 4, 5), align_series=4),
                              align_series=4)
    with pytest.raises(Exception, match="ls_beat_metrics"):
        bm.beat_metrics(pred, joints=6)                                        # the BEAT series need joint 27


@pytest.mark.parametrize("order", [1, 3])
def test_other_orders(order, g21, onsets):
    from livelyspeaker_amd import beat_metrics as bm
    got = bm.beat_metrics(g21["pred_euler"], None, None, onsets, order=order)
    want = R.score_batch(g21["pred_euler"], None, None, onsets, order=order)
    assert want["beat_mask"].sum() != R.score_batch(g21["pred_euler"], None, None, onsets)["beat_mask"].sum()
    check_against_restatement(got, want, order=order)


def test_l1div(g21):
    import torch
    from livelyspeaker_amd import beat_metrics as bm
    rows = g21["pred_euler"].reshape(136, 141)
    keep = rows.copy()
    l1 = bm.L1div()
    l1.run(rows)
    print("l1div sum", l1.sum, "reference", float(g21["l1div_sum"]))
    assert np.array_equal(rows, keep) and l1.counter == 136              # the caller's rows are only read
    assert abs(l1.sum - g21["l1div_sum"]) <= 1e-6 * g21["l1div_sum"] and abs(l1.avg() - g21["l1div_avg"]) <= 1e-6 * g21["l1div_avg"]
    assert bm.l1div_sum(rows[:1]) == 0.0                                 # one row is its own mean
    big = torch.from_numpy(np.tile(rows, (64, 1))).cuda()                # 8704 rows, device-resident
    before = big.clone()
    got = bm.l1div_sum(big)
    want = R.l1div_sum(np.tile(rows, (64, 1)))
    assert abs(got - want) <= 1e-6 * want and torch.equal(big, before)
    l1.run(big)
    assert l1.counter == 136 + 8704 and abs(l1.avg() - (g21["l1div_sum"] + want) / (136 + 8704)) <= 1e-6 * l1.avg()
    odd = rows[:67, :13]                                                 # a partial row block, non-contiguous input
    want = R.l1div_sum(odd)
    assert abs(bm.l1div_sum(odd) - want) <= 1e-6 * want


def test_load_pose_and_srgr_drop_ins(base, g21):
    from livelyspeaker_amd import beat_metrics as bm
    al = bm.alignment(0.3, 2)
    beats = al.load_pose(g21["pred_euler"][0], 0, 500, 15, True)
    assert len(beats) == 6 and all(isinstance(b, tuple) and len(b) == 1 for b in beats)
    for s in range(6):
        assert np.array_equal(beats[s][0], np.nonzero(base["beat_mask"][0, s])[0])
    srgr = bm.SRGR(4, 47)
    rate = srgr.run(g21["pred_euler"].reshape(-1, 141), g21["target_euler"].reshape(-1, 141), g21["semantic"].flatten())
    assert rate == float(base["srgr_sum"].astype(np.float64).sum()) / (136 * 47) and srgr.avg() == rate
