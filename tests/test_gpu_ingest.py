"""The dataset ingest on the device (ls_ted_ingest, ls_beat_ingest) against fixture G23, which tests/golden/make_golden_ingest.py recorded
from the reference's own DataPreprocessor / MotionPreprocessor / data_utils (TED) and rot_utils (BEAT): every window of the batch is
compared, none is skipped.  Each recording has at most 100 raw frames.

Measured on an MI355X (profiles/r18_ingest.md has the run): see the figures each test prints before it asserts."""
import os

import numpy as np
import pytest

import ingest_restatement as R
from conftest import GOLDEN
from livelyspeaker_amd import ingest, postprocess as pp

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -24


@pytest.fixture(scope="module")
def g23():
    return np.load(os.path.join(GOLDEN, "ingest_golden.npz"))


def recordings(g):
    off = np.concatenate([[0], np.cumsum(g["n_raw"])])
    B = len(g["n_raw"])
    words = [[("w", s, e) for s, e in g["word_times"][g["word_offsets"][b]:g["word_offsets"][b + 1]]] for b in range(B)]
    return ([g["raw"][off[b]:off[b + 1]] for b in range(B)], [R.fixture_audio(b, int(g["audio_len"][b])) for b in range(B)],
            g["start_time"].tolist(), g["end_time"].tolist(), words)


def run_ted(g, rows=None, cuda=False, **kw):
    sk, au, s, e, words = recordings(g)
    rows = range(len(sk)) if rows is None else rows
    pick = lambda v: [v[b] for b in rows]                                   # noqa: E731
    sk, au = pick(sk), pick(au)
    if cuda:
        import torch
        sk, au = [torch.from_numpy(v).cuda() for v in sk], [torch.from_numpy(v).cuda() for v in au]
    out = ingest.ted_ingest(sk, au, pick(s), pick(e), g["mean_pose"], g["mean_dir_vec"], words=pick(words), **kw)
    return {k: (v.cpu().numpy() if hasattr(v, "detach") else v) for k, v in out.items()}


@pytest.fixture(scope="module")
def ted_all(g23):
    """every window that has its words, filtered or not: what the fixture's data rows hold"""
    return run_ted(g23, disable_filtering=True)


@pytest.fixture(scope="module")
def ted_kept(g23):
    return run_ted(g23)


def ted_bound(g):
    """32 * 2^-24 * max|coordinate| / min non-zero bone length, from the fixture's own inputs: the float32 rounding of interpolation,
    subtraction and normalisation, amplified by the cancellation in a short bone"""
    raw = g["raw"].astype(np.float64)
    bones = np.stack([np.linalg.norm(raw[:, b] - raw[:, a], axis=1) for a, b, _ in R.DIR_VEC_PAIRS], 1)
    return 32 * EPS * np.abs(raw).max() / bones[bones > 0].min()


def test_ted_tolerance(g23, ted_all):
    g, got = g23, ted_all
    bound = ted_bound(g)
    assert got["pose_seq"].shape == g["pose_seq"].shape == (len(g["data_rows"]), 34, 30) and got["vec_seq"].shape == g["vec_seq"].shape
    d_pose = np.abs(got["pose_seq"].astype(np.float64) - g["pose_seq"]).max()
    d_vec = np.abs(got["vec_seq"].astype(np.float64) - g["vec_seq"]).max()
    want_x = g["vec_seq"].reshape(-1, 34, 9, 3).transpose(0, 2, 3, 1)
    d_x = np.abs(got["x"].astype(np.float64) - want_x).max()
    print(f"G23 TED: bound {bound:.3e}; max |pose_seq - ref| {d_pose:.3e}, |vec_seq - ref| {d_vec:.3e}, |x - ref| {d_x:.3e}")
    assert d_pose <= bound and d_vec <= bound and d_x <= bound
    assert np.array_equal(got["x"], got["vec_seq"].reshape(-1, 34, 9, 3).transpose(0, 2, 3, 1))       # x is vec_seq in the model's layout
    s = np.abs(got["stats"].astype(np.float64) - g["stats"]) / R.THRESHOLDS
    print(f"G23 TED: max |statistic - float64| / threshold {s.max():.3e} (every statistic lies >= 1e-2 from its threshold)")
    assert s.max() < 1e-3


def test_verdicts_keep_and_order(g23, ted_all, ted_kept):
    g = g23
    for got in (ted_all, ted_kept):
        assert np.array_equal(got["verdict"], g["verdict"]) and np.array_equal(got["clip"], g["win_clip"])
        assert np.array_equal(got["start_frame"], g["win_start"])
    assert np.array_equal(ted_kept["keep"], g["verdict"] == 0) and np.array_equal(np.nonzero(ted_kept["keep"])[0], g["kept_rows"])
    assert np.array_equal(np.nonzero(ted_all["keep"])[0], g["data_rows"])
    at = [g["data_rows"].tolist().index(r) for r in g["kept_rows"]]             # the kept windows among the data rows, in the reference's order
    for k in ("x", "vec_seq", "pose_seq", "audio"):
        assert len(ted_kept[k]) == len(g["kept_rows"]) and np.array_equal(ted_kept[k], ted_all[k][at]), k
    assert np.array_equal(ted_kept["stats"], ted_all["stats"])


def test_audio_windows_are_bitwise(g23, ted_all):
    want = R.decode_audio(g23["audio_first"], g23["audio_delta"])
    assert ted_all["audio"].dtype == np.float32 and np.array_equal(ted_all["audio"], want)
    assert (np.diff(want, axis=1) == -1).any()                                  # a reflected stretch was read


def test_ragged_batch_equals_each_recording_alone(g23, ted_all):
    g = g23
    for b in range(len(g["n_raw"])):
        alone = run_ted(g, rows=[b], disable_filtering=True)
        rows = g["win_clip"] == b
        data = np.isin(g["data_rows"], np.nonzero(rows)[0])
        assert len(alone["verdict"]) == rows.sum()
        assert np.array_equal(alone["verdict"], ted_all["verdict"][rows]) and np.array_equal(alone["stats"], ted_all["stats"][rows])
        for k in ("x", "vec_seq", "pose_seq", "audio"):
            assert np.array_equal(alone[k], ted_all[k][data]), (b, k)


def test_zero_length_bone_gives_zeros(g23, ted_all):
    g = g23
    mean = g["mean_dir_vec"].reshape(9, 3)
    zero = np.abs(g["vec_seq"].reshape(-1, 34, 9, 3) + mean).max(-1) == 0          # where the reference's direction is zero
    assert zero.any() and zero[..., 2].sum() == zero.sum()                          # the bone (2, 3)
    got = ted_all["vec_seq"].reshape(-1, 34, 9, 3)
    assert np.array_equal(got[zero], np.broadcast_to(np.float32(0) - mean, got.shape)[zero])
    raw = g["raw"][:20]
    d = ingest.convert_pose_seq_to_dir_vec(raw)
    assert d.shape == (20, 9, 3) and not np.isnan(d).any() and (d[:13, 2] == 0).all() and (np.abs(np.linalg.norm(d[13:], axis=-1) - 1) < 1e-6).all()


def beat_inputs(g):
    return ([g["beat_tar_pose_0"], g["beat_tar_pose_1"]], [R.fixture_audio(b, int(g["beat_audio_len"][b])) for b in range(2)])


def test_beat_tolerance(g23):
    g = g23
    poses, audio = beat_inputs(g)
    got = ingest.beat_ingest(poses, audio, g["beat_mean"], g["beat_std"])
    want, want_audio, gap = [], [], 0.0
    for b in range(2):
        ref = g[f"beat_rot6d_{b}"]
        gap = max(gap, np.abs(ref - R.beat_rot6d(poses[b], g["beat_mean"], g["beat_std"])).max())
        for s, a0 in R.beat_windows(len(poses[b]), len(audio[b])):
            want.append(ref[s:s + 34])
            want_audio.append(R.symmetric_window(audio[b], a0, 36266))
    want = np.array(want)
    tol = 2 * gap                 # the float32 reference against float64, doubled: the device's sin and cos are not torch's
    d = np.abs(got["rot6d"].astype(np.float64) - want).max()
    print(f"G23 BEAT: float32 reference against float64 {gap:.3e}, tolerance {tol:.3e}; max |rot6d - ref| {d:.3e}")
    assert got["rot6d"].shape == want.shape == (8, 34, 282) and d <= tol
    assert np.array_equal(got["x"], got["rot6d"].reshape(-1, 34, 47, 6).transpose(0, 2, 3, 1))
    assert np.array_equal(got["audio"], np.array(want_audio)) and got["keep"].all() and (got["verdict"] == 0).all()
    assert got["clip"].tolist() == [0] * 5 + [1] * 3 and got["start_frame"].tolist() == [0, 10, 20, 30, 40, 0, 10, 20]
    keep = np.array([1, 0, 1, 1, 0, 1, 1, 0], np.uint8)                         # the caller's word / sem rules
    part = ingest.beat_ingest(poses, audio, g["beat_mean"], g["beat_std"], keep_windows=keep)
    assert part["verdict"].tolist() == [0, 4, 0, 0, 4, 0, 0, 4] and np.array_equal(part["keep"], keep != 0)
    for k in ("x", "rot6d", "audio"):
        assert np.array_equal(part[k], got[k][keep != 0]), k
    alone = ingest.beat_ingest(poses[1:], audio[1:], g["beat_mean"], g["beat_std"])                 # ragged against alone
    for k in ("x", "rot6d", "audio"):
        assert np.array_equal(alone[k], got[k][5:]), k


def test_ted_round_trip():
    """convert_pose_seq_to_dir_vec(ted_postprocess(sample)['pose']) is the unit direction of sample + mean_dir_vec.  The pose is a
    float32 chain of at most 4 bones (coordinates below 1.5) and a direction its difference over a bone of at least 0.14: the same
    32 * 2^-24 * max|coordinate| / min bone length as on the fixture."""
    rng = np.random.Generator(np.random.PCG64(1810))
    sample = (0.3 * rng.standard_normal((3, 9, 3, 34))).astype(np.float32)
    pose = pp.ted_postprocess(sample)["pose"]
    got = ingest.convert_pose_seq_to_dir_vec(pose)
    v = sample.transpose(0, 3, 1, 2).astype(np.float64) + pp.TED_MEAN_DIR_VEC.reshape(9, 3)
    want = v / np.linalg.norm(v, axis=-1, keepdims=True)
    bound = 32 * EPS * np.abs(pose).max() / min(ln for _, _, ln in pp.TED_DIR_VEC_PAIRS)
    d = np.abs(got - want).max()
    print(f"TED round trip: max |direction - unit(sample + mean)| {d:.3e}, bound {bound:.3e}")
    assert got.shape == (3, 34, 9, 3) and got.dtype == np.float64 and d <= bound
    assert np.array_equal(ingest.convert_pose_seq_to_dir_vec(pose[0]), got[0])                        # 3-D input
    assert np.array_equal(ingest.convert_pose_seq_to_dir_vec(pose.reshape(3, 34, 30)), got)           # flattened joints


def test_beat_round_trip():
    """beat_postprocess(beat_ingest(.)['x']) returns the Euler angles that went in, away from gimbal lock (|Y| < 80 degrees).  A
    rot6d entry carries a few float32 roundings (16 * 2^-24 allows for degrees -> radians at |angle| <= pi, sin / cos, products, sum
    and the inverse's normalisation); atan2 / asin amplify them by at most 1 / cos(80 degrees) = 5.76, in degrees by 57.3; the input
    itself is rounded at `* std + mean` (4 * 2^-24 * 180)."""
    rng = np.random.Generator(np.random.PCG64(1811))
    euler = rng.uniform(-170, 170, (45, 47, 3))
    euler[:, :, 1] = rng.uniform(-80, 80, (45, 47))
    mean, std = rng.uniform(-30, 30, 141), rng.uniform(5, 40, 141)
    tar = ((euler.reshape(45, 141) - mean) / std).astype(np.float32)
    out = ingest.beat_ingest([tar], [np.zeros(48000, np.float32)], mean, std)
    back = pp.beat_postprocess(out["x"])["pred_euler"]
    tol = 57.3 * 5.76 * 16 * EPS + 4 * 180 * EPS
    d = max(np.abs(back[w].astype(np.float64) - euler.reshape(45, 141)[s:s + 34]).max() for w, s in enumerate((0, 10)))
    print(f"BEAT round trip: max |Euler back - Euler in| {d:.3e} degrees, tolerance {tol:.3e}")
    assert back.shape == (2, 34, 141) and d <= tol


def test_device_pointers_equal_host_pointers(g23, ted_all):
    import torch
    dev = run_ted(g23, cuda=True, disable_filtering=True)
    for k, v in ted_all.items():
        assert np.array_equal(dev[k], v), k
    poses, audio = beat_inputs(g23)
    host = ingest.beat_ingest(poses, audio, g23["beat_mean"], g23["beat_std"])
    out = ingest.beat_ingest([torch.from_numpy(p).cuda() for p in poses], [torch.from_numpy(a).cuda() for a in audio], g23["beat_mean"],
                             g23["beat_std"])
    assert out["x"].is_cuda and out["keep"].is_cuda
    for k, v in host.items():
        assert np.array_equal(out[k].cpu().numpy() if hasattr(out[k], "detach") else out[k], v), k


def test_drop_ins(g23):
    g = g23
    sk, au, s, e, _ = recordings(g)
    bound = ted_bound(g)
    for b in (0, 1, 3):                                                          # down-sampling, up-sampling with its tail, a short one
        want = R.resample_pose_seq(sk[b], e[b] - s[b], 15)
        got = ingest.resample_pose_seq(sk[b], e[b] - s[b], 15)
        assert got.shape == want.shape == (g["resampled_len"][b], 10, 3) and got.dtype == np.float32
        assert np.abs(got.astype(np.float64) - want).max() <= bound
    a = au[0][:1000]
    for n in (1, 999, 1000, 1001, 1700, 2000):
        want = np.pad(a, (0, max(0, n - 1000)), mode="symmetric")[:n]
        assert np.array_equal(ingest.make_audio_fixed_length(a, n), want), n
    for r in range(len(g["verdict"])):                                           # every window through MotionPreprocessor.get
        b, f = int(g["win_clip"][r]), int(g["win_start"][r])
        win = R.resample_pose_seq(sk[b], e[b] - s[b], 15)[f:f + 42]
        mp = ingest.MotionPreprocessor(win, g["mean_pose"])
        kept, message = mp.get()
        want = R.VERDICTS[R.motion_verdict(g["stats"][r])]
        assert message == want and (kept == win.tolist() if want == "PASS" else kept == []), (r, message, want)
        assert np.abs(mp.stats - g["stats"][r]).max() / R.THRESHOLDS.min() < 1
