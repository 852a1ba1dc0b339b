"""The BEAT evaluation metrics, host side: the float64 restatement (tests/beat_metrics_restatement.py) against the reference's own
numbers (fixture G21, tests/golden/make_golden_beat_metrics.py) and against scipy, the fixture's usability conditions, and the
C-ABI / Python surface of ls_beat_metrics and ls_beat_ldiv.  Nothing here needs a GPU."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
from scipy.signal import argrelextrema

import beat_metrics_restatement as R
from livelyspeaker_amd import _lib, beat_metrics as bm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def g21():
    return dict(np.load(R.GOLDEN))


def rel(a, b):
    return abs(float(a) - float(b)) / max(abs(float(b)), 1e-300)


def test_fixture_inputs_are_the_seeded_ones(g21, golden):
    target, semantic, onsets = R.fixture_inputs(golden["beat"]["G3_ddpm50_final"])
    assert np.array_equal(target.transpose(0, 3, 1, 2).reshape(4, 34, 282), g21["tar_pose"])
    assert np.array_equal(semantic, g21["semantic"]) and set(np.round(semantic * 10).astype(int).ravel()) <= set(range(11))
    assert np.array_equal(np.concatenate(onsets), g21["onset_times"])
    assert np.array_equal(np.cumsum([0] + [len(o) for o in onsets]), g21["onset_offsets"])
    assert all(3 <= len(o) <= 8 and o.min() >= 0 and o.max() <= 2.2 for o in onsets)


def test_restatement_srgr_against_the_reference(g21):
    success, diff = R.srgr_success(g21["pred_euler"], g21["target_euler"])
    keep = ~g21["srgr_excluded"].reshape(-1, 47)
    assert np.array_equal(success[keep], g21["success"].reshape(-1, 47)[keep])
    # the rates are sums over the whole mask: taken from the reference's own mask so that an excluded entry cannot move them
    ref = g21["success"].reshape(-1, 47)
    assert rel(R.srgr_rate(ref, g21["semantic"]), g21["srgr_rate"]) < 1e-9
    assert rel(R.srgr_rate(ref[:2 * 34], g21["semantic"][:2]), g21["srgr_rate2"]) < 1e-9
    rows = (4 * 34, 2 * 34)
    avg = (g21["srgr_rate"] * rows[0] + g21["srgr_rate2"] * rows[1]) / sum(rows)
    assert rel(avg, g21["srgr_avg"]) < 1e-9
    assert rel(R.srgr_clip_sums(ref, g21["semantic"]).sum() / (4 * 34 * 47), g21["srgr_rate"]) < 1e-9


def test_restatement_l1div_against_the_reference(g21):
    # L1div.run on the fixture's rows as float64; the scripts hand it the fp32 planes, and that fp32 (pairwise) sum is what
    # l1div_sum holds for the GPU test, whose 1e-6 covers its rounding
    rows = g21["pred_euler"].reshape(-1, 141)
    assert rel(R.l1div_sum(rows), g21["l1div_sum_f64"]) < 1e-9
    assert rel(R.l1div_sum(rows) / 136, g21["l1div_avg_f64"]) < 1e-9
    # fp32 against float64: one rounding each for the mean and the difference, log2(n) levels of numpy's pairwise sum, half an ulp each
    assert rel(g21["l1div_sum"], g21["l1div_sum_f64"]) < (np.log2(136 * 141) + 2) * 2.0 ** -24 < 1e-6
    assert rel(g21["l1div_sum"] / 136, g21["l1div_avg"]) < 2.0 ** -23        # the reference's sum and quotient are fp32 numbers


def test_restatement_beats_and_align_against_the_reference(g21):
    onsets = np.split(g21["onset_times"], g21["onset_offsets"][1:-1])
    got = R.score_batch(g21["pred_euler"], None, None, onsets)
    assert np.abs(got["vel"] - g21["vel"]).max() < 1e-3          # the reference differences and norms in fp32 (values up to ~600)
    keep = ~g21["beat_excluded"]
    assert np.array_equal(got["beat_mask"][keep], g21["beat_mask"][keep])
    for b in range(4):
        times = np.nonzero(g21["beat_mask"][b, 2])[0] / 15
        assert rel(R.gahr(times, onsets[b]), g21["align"][b]) < 1e-9
        if not g21["beat_excluded"][b, 2].any():
            assert rel(got["align"][b], g21["align"][b]) < 1e-9


def test_fixture_usability_conditions(g21):
    ex, bx = g21["srgr_excluded"], g21["beat_excluded"]
    assert ex.mean() <= 0.02 and ex.reshape(4, -1).mean(1).max() <= 0.02
    assert bx.mean() <= 0.02
    assert (~bx[:, 2].any(1)).sum() >= 3
    assert 0.2 <= g21["success"].mean() <= 0.8
    diff = R.srgr_success(g21["pred_euler"], g21["target_euler"])[1].reshape(4, 34, 47)
    assert np.array_equal(ex, np.abs(diff - 4.0) < R.SRGR_MARGIN)
    margin = np.stack([[R.minima_margin(v, 2) for v in clip] for clip in g21["vel"]]) < R.BEAT_MARGIN
    margin[:, :, [0, 32]] = False
    assert np.array_equal(bx, margin)


@pytest.mark.parametrize("order", [1, 2, 3])
def test_minima_are_scipys(order):
    rng = np.random.default_rng(31 + order)
    series = [rng.uniform(0, 50, 33) for _ in range(8)]
    series += [np.round(rng.uniform(0, 4, 33)) for _ in range(8)]                    # plateaus: equal neighbours give no beat
    series += [rng.uniform(0, 1, n) for n in (1, 2, 3, 2 * order, 2 * order + 1)]    # shorter than 2 * order + 1
    series += [np.zeros(33), np.r_[3.0, 1.0, 1.0, 3.0, 0.5, 2.0], np.r_[2.0, 1.0, 2.0]]
    for x in series:
        assert np.array_equal(R.minima(x, order), argrelextrema(x, np.less, order=order)[0]), x
        ends = {0, len(x) - 1}
        assert not ends & set(R.minima(x, order).tolist())
    assert R.minima(np.r_[3.0, 1.0, 1.0, 3.0], 1).size == 0


def test_frames_to_time(g21):
    assert np.array_equal(bm.frames_to_time(g21["frames"]), g21["frames_time"])
    assert bm.frames_to_time(np.array([43]))[0] == 43 * 512 / 22050
    assert bm.frames_to_time(np.array([10]), sr=16000, hop_length=256)[0] == 10 * 256 / 16000


def test_fid_and_diversity_against_the_reference(g21):
    import torch
    feat = np.load(os.path.join(ROOT, "tests", "golden", "eval_beat_golden.npz"))["beat_feat"]
    assert rel(bm.FIDCalculator.frechet_distance(feat[:48], feat[48:]), g21["fid"]) < 1e-6
    torch.manual_seed(4)
    assert rel(bm.FIDCalculator.get_diversity([feat[i:i + 16] for i in range(0, 96, 16)]), g21["diversity"]) < 1e-6


def test_host_side_of_the_drop_ins(g21):
    al = bm.alignment(0.3, 2)
    with pytest.raises(NotImplementedError):
        al.load_pose(g21["pred_euler"][0], 1, 500, 15, True)
    with pytest.raises(NotImplementedError):
        al.load_pose(g21["pred_euler"][0], 0, 1, 15, True)
    with pytest.raises(NotImplementedError, match="librosa"):
        al.load_audio(np.zeros(16000), 0, 500, True)
    onsets = np.split(g21["onset_times"], g21["onset_offsets"][1:-1])
    beats = [(np.nonzero(g21["beat_mask"][0, s])[0],) for s in range(6)]
    assert rel(al.calculate_align(None, None, onsets[0], *beats, 15), g21["align"][0]) < 1e-9
    assert al.GAHR(np.array([]), onsets[0], 0.3) == 0.0
    with pytest.raises(ValueError, match="clip 1"):
        bm._ragged([[0.5], [], [1.0]], 3)
    s = bm.SRGR(4, 47)
    assert s.avg() == 0 and (s.threshold, s.joints, s.pose_dimes) == (4, 47, 3)
    ref = R.srgr_clip_sums(g21["success"], g21["semantic"])
    assert rel(s.add(ref, 4 * 34), g21["srgr_rate"]) < 1e-9
    s.add(ref[:2], 2 * 34)
    assert rel(s.avg(), g21["srgr_avg"]) < 1e-9 and s.counter == 6 * 34
    assert bm.BEAT_SERIES_JOINTS == R.SERIES_JOINTS and bm.SRGR_SCALE == 1 / 0.165


def test_abi_mirror_of_the_beat_metrics_arguments(tmp_path):
    """LsBeatMetricsArgs against what a C compiler makes of include/ls_hip.h; both entry points declared, exported and listed."""
    fields = [n for n, _ in _lib.LsBeatMetricsArgs._fields_]
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ls_hip.h"\nint main(void) {\n'
                   '    printf("%zu", sizeof(ls_beat_metrics_args));\n' +
                   "".join(f'    printf(" %zu", offsetof(ls_beat_metrics_args, {n}));\n' for n in fields) +
                   '    printf(" %d\\n", LS_ABI_VERSION);\n    return 0;\n}\n')
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    A = _lib.LsBeatMetricsArgs
    assert got == [ctypes.sizeof(A)] + [getattr(A, n).offset for n in fields] + [5]
    hdr = open(os.path.join(ROOT, "include", "ls_hip.h")).read()
    lib = ctypes.CDLL(_lib.library_path())
    for name in ("ls_beat_metrics", "ls_beat_ldiv"):
        assert name in _lib.EXPORTS and re.search(rf"\bint {name}\s*\(", hdr) and hasattr(lib, name), name


def test_invalid_arguments_are_refused_without_a_launch():
    """Every LS_EINVAL exit sits in front of hipSetDevice: no GPU is needed to be refused."""
    lib = _lib.load_library()
    x = np.zeros((1, 34, 141), np.float32)
    vel = np.zeros((1, 6, 33), np.float32)
    al = np.zeros(1, np.float32)
    on = np.array([0.5], np.float32)

    def args(**kw):
        a = _lib.LsBeatMetricsArgs()
        a.batch, a.njoints, a.order, a.align_series = 1, 47, 2, 2
        for s, j in enumerate(bm.BEAT_SERIES_JOINTS):
            a.series_joint[s] = j
        a.threshold, a.scale, a.sigma, a.fps = 4.0, 1 / 0.165, 0.3, 15.0
        a.pred, a.vel = x.ctypes.data, vel.ctypes.data
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    def offsets(*v):
        o = np.array(v, np.int64)
        return dict(onset_offsets=o.ctypes.data, onset_times=on.ctypes.data, align=al.ctypes.data), o

    assert lib.ls_beat_metrics(0, None) == -1
    assert lib.ls_beat_metrics(0, ctypes.byref(args(pred=None))) == -1
    assert lib.ls_beat_metrics(0, ctypes.byref(args(batch=0))) == -1
    assert lib.ls_beat_metrics(0, ctypes.byref(args(order=0))) == -1
    assert lib.ls_beat_metrics(0, ctypes.byref(args(njoints=27))) == -1            # series joint 27 is outside [0, 27)
    a = args()
    a.series_joint[3] = -1
    assert lib.ls_beat_metrics(0, ctypes.byref(a)) == -1
    assert lib.ls_beat_metrics(0, ctypes.byref(args(align_series=6))) == -1
    assert lib.ls_beat_metrics(0, ctypes.byref(args(srgr_sum=al.ctypes.data))) == -1     # SRGR without a target
    assert lib.ls_beat_metrics(0, ctypes.byref(args(align=al.ctypes.data))) == -1        # alignment without onsets
    for bad in ((0, 0), (1, 2), (0, -1)):                                           # no onset, not from 0, decreasing
        kw, keep = offsets(*bad)
        assert lib.ls_beat_metrics(0, ctypes.byref(args(**kw))) == -1, bad
    keep = offsets(0, 1, 0)                                                         # offsets not non-decreasing
    b2 = args(batch=2, **keep[0])
    assert lib.ls_beat_metrics(0, ctypes.byref(b2)) == -1
    total = ctypes.c_double()
    assert lib.ls_beat_ldiv(0, 0, 0, 141, x.ctypes.data, ctypes.byref(total)) == -1
    assert lib.ls_beat_ldiv(0, 0, 34, 0, x.ctypes.data, ctypes.byref(total)) == -1
    assert lib.ls_beat_ldiv(0, 0, 34, 141, None, ctypes.byref(total)) == -1
    assert lib.ls_beat_ldiv(0, 0, 34, 141, x.ctypes.data, None) == -1
