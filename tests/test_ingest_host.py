"""Dataset ingest, host side: ls_ingest_plan against numpy (and scipy's interp1d where it is installed), its refusals, the C-ABI
mirrors of the three argument structs, what ls_ted_ingest / ls_beat_ingest refuse before they touch a device, and the float64
restatement (tests/ingest_restatement.py) against fixture G23 (tests/golden/make_golden_ingest.py).  Nothing here needs a GPU."""
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest

import ingest_restatement as R
from livelyspeaker_amd import _lib, ingest
from livelyspeaker_amd.postprocess import ted_post_config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "ingest_golden.npz")
N_EXT, STRIDE = 42, 10


def sweep(fps):
    """(n, duration) with n in 2..120: expected frame counts m = duration * fps for which n / step = m lands on whole numbers (m
    itself, as duration = m / fps usually makes it) and just beside them (the duration nudged by a few units in the last place and by
    1e-9), among them the TED rates 25 -> 15 and 10 -> 15, m = n_ext and m around it"""
    cases = []
    for n in range(2, 121):
        for m in sorted({n, 2 * n, max(2, n // 2), max(2, round(n * 15 / 25)), round(n * 1.5), N_EXT, N_EXT + 1, N_EXT - 1, 7, 63}):
            d = m / fps
            for dur in (d, np.nextafter(d, 0), np.nextafter(d, 1e9), d * (1 - 1e-9), d * (1 + 1e-9), d + 1 / (3 * fps)):
                cases.append((n, float(dur)))
    return cases


@pytest.mark.parametrize("fps", [10, 15, 25])
def test_plan_against_numpy(fps):
    cases = sweep(fps)
    rng = np.random.Generator(np.random.PCG64(1800 + fps))
    n_raw = [c[0] for c in cases]
    start = rng.uniform(0, 5, len(cases))
    end = start + np.array([c[1] for c in cases])
    dur = end - start                                     # what the plan forms: the sweep's durations up to the rounding of start + d - start
    # audio lengths: mostly as long as the motion, some shorter so that the last windows are padded (never below the window itself)
    L = np.maximum((dur * 16000 * rng.choice([1.0, 0.97, 0.8], len(cases))).astype(np.int64), int(N_EXT / fps * 16000))
    words = [[("w", s + 0.37 * k, s + 0.37 * k + rng.uniform(0.05, 0.3)) for k in range(int(rng.integers(0, 12)))] for s in start]
    p = ingest.ingest_plan(n_raw, start, end, L, words=words, fps=fps)
    assert p["frame_offsets"][0] == 0 and p["frame_offsets"][-1] == p["n_frames"] and p["window_offsets"][-1] == p["n_windows"]
    audio_window = int(N_EXT / fps * 16000)
    on_integer = beside = tails = empty = padded = 0
    for b, n in enumerate(n_raw):
        x_new, lo, frac = R.resample_table(n, dur[b], fps)
        f0, f1 = p["frame_offsets"][b], p["frame_offsets"][b + 1]
        assert f1 - f0 == len(x_new) == math.ceil(n / (n / (dur[b] * fps))), (n, dur[b])
        assert np.array_equal(p["frame_lo"][f0:f1], lo) and np.array_equal(p["frame_hi"][f0:f1], lo + 1) and (p["frame_clip"][f0:f1] == b).all()
        assert np.array_equal(p["frame_frac"][f0:f1], frac.astype(np.float32))           # equal after one rounding to float
        assert lo.min() >= 0 and lo.max() <= n - 2
        on_integer += int((frac[1:] == 1).any())
        tails += int((frac > 1).any())
        beside += int(len(x_new) != round(dur[b] * fps))
        rows = R.ted_windows(len(x_new), int(L[b]), start[b], words[b], N_EXT, STRIDE, fps)
        w0, w1 = p["window_offsets"][b], p["window_offsets"][b + 1]
        assert w1 - w0 == len(rows) == max(0, math.floor((len(x_new) - N_EXT) / STRIDE) + 1)
        empty += int(not rows)
        for w, (s, a0, n_pad, has) in zip(range(w0, w1), rows):
            got = (p["win_clip"][w], p["win_first"][w], p["win_audio_start"][w], p["win_n_pad"][w], bool(p["win_has_words"][w]))
            assert got == (b, s, a0, n_pad, has), (b, w, got, (s, a0, n_pad, has))
            assert a0 == math.floor(s / len(x_new) * int(L[b])) and n_pad == max(0, a0 + audio_window - int(L[b]))
            padded += int(n_pad > 0)
    assert min(on_integer, beside, tails, empty, padded) > 20, (on_integer, beside, tails, empty, padded)      # the sweep reaches every case
    assert {0, 1} == set(p["win_has_words"].tolist())
    no_words = ingest.ingest_plan(n_raw, start, end, L, fps=fps)
    assert no_words["win_has_words"].all() and np.array_equal(no_words["win_audio_start"], p["win_audio_start"])


def test_plan_frames_are_interp1d():
    """The table's (lo, frac) reproduce scipy's interp1d(kind='linear', fill_value='extrapolate') on random data."""
    interp1d = pytest.importorskip("scipy.interpolate").interp1d
    rng = np.random.Generator(np.random.PCG64(1801))
    for n, dur, fps in [(2, 1.0, 15), (40, 4.0, 15), (100, 4.0, 15), (75, 3.0, 10), (120, 2.8, 25), (7, 3.1, 15)]:
        y = rng.standard_normal((n, 5))
        x_new = np.arange(0, n, n / (dur * fps))
        want = interp1d(np.arange(0, n), y, axis=0, kind="linear", fill_value="extrapolate")(x_new)
        p = ingest.ingest_plan([n], [0.0], [dur], [1 << 30], fps=fps)
        lo, hi = p["frame_lo"], p["frame_hi"]
        frac = x_new - lo
        assert np.array_equal(p["frame_frac"], frac.astype(np.float32))
        assert np.abs(y[lo] + (y[hi] - y[lo]) * frac[:, None] - want).max() < 1e-12


def test_beat_plan_against_the_restatement():
    n_raw, L = [75, 60, 33, 100, 510], [5 * 16000 + 123, 4 * 16000, 3 * 16000, 4 * 16000 + 15999, 34 * 16000]
    for first, final in ((0, 0), (1, 1)):
        seconds = [min(n // 15, l // 16000) for n, l in zip(n_raw, L)]
        p = ingest.ingest_plan(n_raw, [first] * 5, [s - final for s in seconds], L, beat=True)
        assert p["n_frames"] == 0 and p["n_ext"] == 34
        for b in range(5):
            rows = R.beat_windows(n_raw[b], L[b], clean_first=first, clean_final=final)
            w0, w1 = p["window_offsets"][b], p["window_offsets"][b + 1]
            assert [(int(p["win_first"][w]), int(p["win_audio_start"][w])) for w in range(w0, w1)] == rows, (b, first)
            for w in range(w0, w1):
                end = int(p["win_audio_start"][w]) + 36266
                assert p["win_n_pad"][w] == max(0, end - 16000 * (seconds[b] - final))
    # floor(34 / 15 * 16000) samples from floor(start * 16000 / 15) end before the clip's last whole second does: BEAT never pads
    assert p["n_windows"] > 0 and (p["win_n_pad"] == 0).all()


def test_plan_refusals():
    ok = dict(n_raw=[100], start_times=[0.0], end_times=[4.0], audio_len=[64000])
    assert ingest.ingest_plan(**ok)["n_windows"] == 2
    for bad in (dict(audio_len=[0]),                                 # empty audio
                dict(audio_len=[20000]),                             # the second window's padding is longer than the audio itself
                dict(n_raw=[1]), dict(n_raw=[0]),
                dict(n_poses=43, n_ext=42), dict(n_poses=0), dict(n_poses=65, n_ext=70), dict(n_ext=129),
                dict(stride=0), dict(fps=0), dict(sr=0), dict(end_times=[0.0])):
        with pytest.raises(_lib.EngineError):
            ingest.ingest_plan(**{**ok, **bad})
    assert ingest.ingest_plan(**{**ok, "audio_len": [33000]})["win_n_pad"].tolist() == [11800, 17300]       # <= 33000: legal
    assert ingest.ingest_plan([50], [0.0], [2.0], [32000])["n_windows"] == 0                                  # shorter than n_ext: legal
    lib = _lib.load_library()
    assert lib.ls_ingest_plan(None) == -1
    a = _lib.LsIngestPlanArgs()
    assert lib.ls_ingest_plan(ctypes.byref(a)) == -1
    with pytest.raises(_lib.EngineError):                            # BEAT: the clip ends beyond the recording
        ingest.ingest_plan([75], [0], [6], [6 * 16000], beat=True)


def test_abi_mirrors_of_the_ingest_arguments(tmp_path):
    """The three ctypes structs against what a C compiler makes of include/ls_hip.h; the entries declared, exported and listed."""
    pairs = [("ls_ingest_plan_args", _lib.LsIngestPlanArgs), ("ls_ted_ingest_args", _lib.LsTedIngestArgs),
             ("ls_beat_ingest_args", _lib.LsBeatIngestArgs)]
    body = ""
    for cname, S in pairs:
        body += f'    printf(" %zu", sizeof({cname}));\n' + "".join(f'    printf(" %zu", offsetof({cname}, {n}));\n' for n, _ in S._fields_)
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ls_hip.h"\nint main(void) {\n' + body +
                   '    printf(" %d %d %d %d %d %d\\n", LS_ABI_VERSION, LS_INGEST_WORDS, LS_INGEST_MAX_POSES, LS_INGEST_MAX_EXT, LS_INGEST_N_STATS,'
                   ' LS_INGEST_MOTION);\n    return 0;\n}\n')
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    want = []
    for _, S in pairs:
        want += [ctypes.sizeof(S)] + [getattr(S, n).offset for n, _ in S._fields_]
    assert got == want + [5, ingest.VERDICTS.index("words"), ingest.MAX_POSES, ingest.MAX_EXT, len(ingest.STATS), ingest.VERDICTS.index("motion")]
    hdr = open(os.path.join(ROOT, "include", "ls_hip.h")).read()
    lib = ctypes.CDLL(_lib.library_path())
    for name in ("ls_ingest_plan", "ls_ted_ingest", "ls_beat_ingest"):
        assert name in _lib.EXPORTS and re.search(rf"\bint {name}\s*\(", hdr) and hasattr(lib, name), name
    lib.ls_abi_version.restype = ctypes.c_int
    assert lib.ls_abi_version() == 5


def test_entries_refuse_a_table_that_leaves_its_recording():
    """Every LS_EINVAL exit sits in front of hipSetDevice: a frame row, a window or an audio window outside its recording never
    reaches a kernel, and no GPU is needed to be refused."""
    lib = _lib.load_library()
    plan = ingest.ingest_plan([100], [0.0], [4.0], [64000])
    raw, wav, mean = np.zeros((100, 30), np.float32), np.zeros(64000, np.float32), np.zeros(30, np.float32)
    cfg = ted_post_config()

    def ted(**kw):
        p = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in plan.items()}
        scalars = dict(n_poses=34, n_ext=42, audio_out_len=36267, batch=1)
        for k, v in kw.items():
            if k in scalars:
                scalars[k] = v
            elif isinstance(v, tuple):
                p[k][v[0]] = v[1]
            else:
                p[k] = v
        a = _lib.LsTedIngestArgs()
        a.batch, a.n_poses, a.n_ext, a.audio_out_len = scalars["batch"], scalars["n_poses"], scalars["n_ext"], scalars["audio_out_len"]
        a.n_frames, a.n_windows, a.cfg = p["n_frames"], p["n_windows"], ctypes.pointer(cfg)
        a.mean_pose, a.raw_poses, a.audio = mean.ctypes.data, raw.ctypes.data, wav.ctypes.data
        for k in ("n_raw", "audio_len", "frame_offsets", "frame_clip", "frame_lo", "frame_hi", "frame_frac", "win_clip", "win_first",
                  "win_audio_start", "win_has_words"):
            setattr(a, k, p[k].ctypes.data)
        ted.keep = p
        return lib.ls_ted_ingest(0, ctypes.byref(a))

    assert lib.ls_ted_ingest(0, None) == -1
    for bad in (dict(frame_hi=(59, 100)), dict(frame_lo=(0, -1)), dict(frame_clip=(3, 1)), dict(win_first=(1, 19)), dict(win_first=(0, -1)),
                dict(win_clip=(0, 1)), dict(win_audio_start=(1, 2 * 64000 - 36267 + 1)), dict(win_audio_start=(0, -1)),
                dict(audio_len=np.array([18133], np.int64)), dict(n_ext=51), dict(n_poses=43), dict(n_poses=65, n_ext=65), dict(audio_out_len=0),
                dict(frame_offsets=np.array([0, 59], np.int32)), dict(batch=0), dict(n_raw=np.array([59], np.int32))):
        assert ted(**bad) == -1, bad
    cfg.njoints = 8
    assert ted() == -1
    cfg.njoints, cfg.bone_child[2] = 9, 10
    assert ted() == -1

    bp = ingest.ingest_plan([75], [0], [5], [80000], beat=True)
    poses, one = np.zeros((75, 141), np.float32), np.ones(141, np.float32)

    def beat(**kw):
        p = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in bp.items()}
        scalars = dict(n_poses=34, njoints=47, audio_out_len=36266)
        for k, v in kw.items():
            if k in scalars:
                scalars[k] = v
            else:
                p[k][v[0]] = v[1]
        a = _lib.LsBeatIngestArgs()
        a.batch, a.n_poses, a.njoints, a.n_windows, a.audio_out_len = 1, scalars["n_poses"], scalars["njoints"], p["n_windows"], scalars["audio_out_len"]
        a.mean_pose, a.std_pose, a.poses, a.audio = one.ctypes.data, one.ctypes.data, poses.ctypes.data, wav.ctypes.data
        for k in ("n_raw", "audio_len", "win_clip", "win_first", "win_audio_start"):
            setattr(a, k, p[k].ctypes.data)
        beat.keep = p
        return lib.ls_beat_ingest(0, ctypes.byref(a))

    assert bp["n_windows"] == 5 and lib.ls_beat_ingest(0, None) == -1
    for bad in (dict(win_first=(4, 42)), dict(win_first=(0, -1)), dict(win_clip=(2, 1)), dict(win_audio_start=(4, 2 * 80000 - 36265)),
                dict(n_poses=35), dict(njoints=48), dict(njoints=0), dict(audio_out_len=0), dict(n_raw=(0, 73))):
        assert beat(**bad) == -1, bad


def test_python_surface_refuses_before_the_library_call():
    with pytest.raises(ValueError, match="symmetric"):
        ingest.make_audio_fixed_length(np.zeros(10, np.float32), 21)
    with pytest.raises(ValueError, match="expected"):
        ingest.convert_pose_seq_to_dir_vec(np.zeros((4, 9, 3), np.float32))
    with pytest.raises(ValueError, match="one skeleton"):
        ingest.ted_ingest([np.zeros((50, 10, 3))], [], [0], [2], np.zeros(30), np.zeros(27))
    with pytest.raises(ValueError, match="frames"):
        ingest.MotionPreprocessor(np.zeros((200, 10, 3), np.float32), np.zeros(30)).get()
    with pytest.raises(ValueError, match="47 joints"):
        ingest.beat_ingest([np.zeros((75, 140), np.float32)], [np.zeros(80000, np.float32)], np.zeros(140), np.ones(140))
    assert ingest.MotionPreprocessor([], np.zeros(30)).get() == ([], "PASS")
    assert ingest.dir_vec_pairs == R.DIR_VEC_PAIRS and ingest.VERDICTS == R.VERDICTS


# ---- the float64 restatement against fixture G23 ----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def g23():
    return np.load(GOLDEN)


def clips_of(g):
    raw_off = np.concatenate([[0], np.cumsum(g["n_raw"])])
    for b in range(len(g["n_raw"])):
        w0, w1 = g["word_offsets"][b], g["word_offsets"][b + 1]
        yield b, g["raw"][raw_off[b]:raw_off[b + 1]], R.fixture_audio(b, int(g["audio_len"][b])), g["word_times"][w0:w1]


def test_restatement_against_the_fixture(g23):
    g = g23
    rows = []
    for b, raw, audio, words in clips_of(g):
        wins = R.ted_ingest(raw, audio, float(g["start_time"][b]), float(g["end_time"][b]), g["mean_pose"], g["mean_dir_vec"], words=words)
        rows += [(b, w) for w in wins]
    assert [b for b, _ in rows] == g["win_clip"].tolist() and [w["start_frame"] for _, w in rows] == g["win_start"].tolist()
    assert [w["verdict"] for _, w in rows] == g["verdict"].tolist()                                  # ALL windows
    assert [i for i, (_, w) in enumerate(rows) if w["verdict"] == 0] == g["kept_rows"].tolist()     # and the kept order
    assert np.abs(np.array([w["stats"] for _, w in rows]) - g["stats"]).max() < 1e-12
    want_audio = R.decode_audio(g["audio_first"], g["audio_delta"])
    assert want_audio.shape == (len(g["data_rows"]), 36267)
    for k, r in enumerate(g["data_rows"]):
        w = rows[r][1]
        assert np.abs(w["pose_seq"].astype(np.float64) - g["pose_seq"][k]).max() <= R.POSE_TOL
        assert np.abs(w["vec_seq"] - g["vec_seq"][k]).max() <= R.VEC_TOL
        assert np.array_equal(w["audio"], want_audio[k])
    assert set(g["verdict"].tolist()) == {0, 1, 2, 3, 4} and len(g["data_rows"]) == len(g["verdict"]) - 1


def test_beat_restatement_against_the_fixture(g23):
    for i in range(2):
        want = g23[f"beat_rot6d_{i}"]
        got = R.beat_rot6d(g23[f"beat_tar_pose_{i}"], g23["beat_mean"], g23["beat_std"])
        assert want.dtype == np.float32 and got.shape == want.shape and np.abs(got - want).max() <= R.ROT_TOL
