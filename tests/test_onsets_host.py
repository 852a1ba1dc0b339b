"""Audio onsets, host side: the float64 restatement (tests/onsets_restatement.py) against what librosa documents, the tables
ls_onsets_tables builds against the restatement's, and the C-ABI / Python surface of ls_onsets.  Nothing here needs a GPU."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import onsets_restatement as R
from livelyspeaker_amd import _lib, audio_onsets as ao, beat_metrics as bm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# librosa.mel_frequencies(n_mels=40), as its documentation prints it
MEL_40 = [0., 85.317, 170.635, 255.952, 341.269, 426.586, 511.904, 597.221, 682.538, 767.855, 853.173, 938.49, 1024.856, 1119.114,
          1222.042, 1334.436, 1457.167, 1591.187, 1737.532, 1897.337, 2071.84, 2262.393, 2470.47, 2697.686, 2945.799, 3216.731,
          3512.582, 3835.643, 4188.417, 4573.636, 4994.285, 5453.621, 5955.205, 6502.92, 7101.009, 7754.107, 8467.272, 9246.028,
          10096.408, 11025.]


def ulps(a, b):
    """Distance in float32 units in the last place, entry by entry (both non-negative; adding 0 turns librosa's -0 into 0)."""
    a, b = a.astype(np.float32) + np.float32(0), b.astype(np.float32) + np.float32(0)
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


def test_mel_scale_is_the_documented_one():
    assert np.abs(R.mel_frequencies(40) - np.array(MEL_40)).max() < 1e-3
    assert abs(R.hz_to_mel(1000.0) - 15.0) < 1e-12 and abs(R.mel_to_hz(R.hz_to_mel(4000.0)) - 4000.0) < 1e-9


def test_pick_parameters():
    assert R.pick_parameters(16000) == (0, 1, 3, 4, 0)
    assert R.pick_parameters(22050) == (1, 1, 4, 5, 1)


@pytest.mark.parametrize("sr,fmax,empty", [(16000, 11025.0, 11), (16000, 8000.0, 0), (22050, 11025.0, 0)])
def test_tables_match_the_restatement(sr, fmax, empty):
    t = ao.onset_tables(sr, fmax=fmax)
    win = R.hann_window().astype(np.float32)
    assert t["window"].dtype == np.float32 and ulps(t["window"][1:], win[1:]).max() <= 1 and t["window"][0] == 0 == win[0]
    assert t["window"][1024] == 1.0
    n = np.arange(2048)
    tw = np.stack([np.cos(2 * np.pi * n / 2048), -np.sin(2 * np.pi * n / 2048)], 1)
    assert np.abs(t["twiddle"] - tw).max() <= 2.0 ** -24
    want = R.mel_filterbank(sr, fmax=fmax)
    got = ao.mel_filterbank(sr, fmax=fmax)
    assert want.dtype == np.float32 and got.shape == want.shape == (128, 1025)
    assert np.array_equal(got != 0, want != 0)                         # the same sparsity pattern
    assert int((~(want != 0).any(1)).sum()) == empty and int((~(got != 0).any(1)).sum()) == empty
    assert ulps(got, want).max() <= 1
    ptr, col = t["mel_ptr"], t["mel_col"]
    assert ptr[0] == 0 and ptr[-1] == col.size == t["mel_w"].size and (np.diff(ptr) >= 0).all() and (t["mel_w"] != 0).all()
    for i in range(128):
        assert (np.diff(col[ptr[i]:ptr[i + 1]]) > 0).all() and (col[ptr[i]:ptr[i + 1]] <= 1024).all()


def test_tables_refuse_bad_arguments():
    lib = _lib.load_library()
    nnz = ctypes.c_int32()

    def call(sr=16000.0, n_fft=2048, n_mels=128, fmin=0.0, fmax=11025.0, col=None, cap=0):
        return lib.ls_onsets_tables(sr, n_fft, n_mels, fmin, fmax, None, None, None, col, None, cap, ctypes.byref(nnz))

    assert call() == 0 and nnz.value == int((R.mel_filterbank(16000) != 0).sum())
    col = np.empty(nnz.value, np.int32)
    assert call(col=col.ctypes.data, cap=nnz.value) == 0 and call(col=col.ctypes.data, cap=nnz.value - 1) == -1
    for bad in (dict(sr=0.0), dict(n_fft=2047), dict(n_fft=0), dict(n_mels=0), dict(fmin=-1.0), dict(fmax=0.0), dict(fmin=5000.0, fmax=4000.0),
                dict(cap=-1)):
        assert call(**bad) == -1, bad


def test_abi_mirror_of_the_onsets_arguments(tmp_path):
    """LsOnsetsArgs against what a C compiler makes of include/ls_hip.h; both entry points declared, exported and listed."""
    fields = [n for n, _ in _lib.LsOnsetsArgs._fields_]
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ls_hip.h"\nint main(void) {\n'
                   '    printf("%zu", sizeof(ls_onsets_args));\n' +
                   "".join(f'    printf(" %zu", offsetof(ls_onsets_args, {n}));\n' for n in fields) +
                   '    printf(" %d %d %d %d\\n", LS_ABI_VERSION, LS_ONSETS_PAD_CONSTANT, LS_ONSETS_PAD_REFLECT, LS_ONSETS_MAX_FRAMES);\n'
                   '    return 0;\n}\n')
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    A = _lib.LsOnsetsArgs
    assert got == [ctypes.sizeof(A)] + [getattr(A, n).offset for n in fields] + [5, ao.PAD_MODES["constant"], ao.PAD_MODES["reflect"],
                                                                                 ao.MAX_FRAMES]
    hdr = open(os.path.join(ROOT, "include", "ls_hip.h")).read()
    lib = ctypes.CDLL(_lib.library_path())
    for name in ("ls_onsets", "ls_onsets_tables"):
        assert name in _lib.EXPORTS and re.search(rf"\bint {name}\s*\(", hdr) and hasattr(lib, name), name
        assert re.fullmatch(r"[a-z_]+", name)


def test_invalid_arguments_are_refused_without_a_launch():
    """Every LS_EINVAL exit sits in front of hipSetDevice: no GPU is needed to be refused."""
    lib = _lib.load_library()
    y = np.zeros((1, 2048), np.float32)
    env = np.zeros((1, 5), np.float32)
    out = np.zeros((1, 5), np.float32)

    def args(**kw):
        a = _lib.LsOnsetsArgs()
        a.batch, a.length, a.pad_mode, a.sr, a.sr_pick, a.fmax, a.delta = 1, 2048, 0, 16000.0, 16000.0, 11025.0, 0.07
        a.audio, a.oenv = y.ctypes.data, out.ctypes.data
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    assert lib.ls_onsets(0, None) == -1
    assert lib.ls_onsets(0, ctypes.byref(args(audio=None))) == -1                              # no input
    assert lib.ls_onsets(0, ctypes.byref(args(envelope=env.ctypes.data))) == -1               # both inputs
    assert lib.ls_onsets(0, ctypes.byref(args(batch=0))) == -1
    assert lib.ls_onsets(0, ctypes.byref(args(length=0))) == -1
    assert lib.ls_onsets(0, ctypes.byref(args(pad_mode=1, length=1024))) == -1                # reflect needs L > 1024
    assert lib.ls_onsets(0, ctypes.byref(args(length=512 * 4096))) == -1                      # 4097 frames
    assert lib.ls_onsets(0, ctypes.byref(args(pad_mode=2))) == -1
    assert lib.ls_onsets(0, ctypes.byref(args(pad_mode=-1))) == -1
    assert lib.ls_onsets(0, ctypes.byref(args(fmax=0.0))) == -1
    assert lib.ls_onsets(0, ctypes.byref(args(fmax=-8000.0))) == -1
    assert lib.ls_onsets(0, ctypes.byref(args(sr=0.0))) == -1
    assert lib.ls_onsets(0, ctypes.byref(args(sr_pick=0.0))) == -1
    given = dict(audio=None, envelope=env.ctypes.data, length=5)
    assert lib.ls_onsets(0, ctypes.byref(args(length=4097, audio=None, envelope=env.ctypes.data))) == -1
    for name in ("mel_db", "rms", "onset_bt_rms"):                                            # a given envelope has no spectrum
        assert lib.ls_onsets(0, ctypes.byref(args(**given, **{name: out.ctypes.data}))) == -1, name


def test_python_surface_refuses_before_the_library_call():
    y = np.zeros((2, 1024), np.float32)
    with pytest.raises(ValueError, match="reflect"):
        ao.audio_onsets(y, pad_mode="reflect")
    with pytest.raises(ValueError, match="pad_mode"):
        ao.audio_onsets(y, pad_mode="edge")
    with pytest.raises(ValueError, match="either"):
        ao.audio_onsets(y, onset_envelope=y)
    with pytest.raises(ValueError, match="either"):
        ao.audio_onsets()
    with pytest.raises(ValueError, match="unknown"):
        ao.audio_onsets(y, want=("onsets",))
    with pytest.raises(ValueError, match="frames"):
        ao.audio_onsets(np.zeros((1, 512 * 4096), np.float32))
    with pytest.raises(ValueError):
        ao.audio_onsets(np.zeros(2048, np.float32))
    with pytest.raises(ValueError, match="units"):
        ao.onset_detect(y[0], units="samples")


def test_host_side_of_the_drop_ins():
    al = ao.alignment(0.3, 2)
    assert isinstance(al, bm.alignment) and (al.sigma, al.order, al.pad_mode, al.fmax) == (0.3, 2, "constant", 11025.0)
    with pytest.raises(NotImplementedError, match="without_file"):
        al.load_audio("speech.wav", 0, 2)
    with pytest.raises(NotImplementedError, match="librosa"):                 # the parent keeps raising
        bm.alignment(0.3, 2).load_audio(np.zeros(16000), 0, 500, True)
    beats = tuple((np.array([3, 9, 17, 25]),) for _ in range(6))
    frames = np.array([4, 20, 31])
    want = bm.alignment.GAHR(np.array([3, 9, 17, 25]) / 15, frames * 512 / 22050, 0.3)
    assert al.calculate_align(None, None, frames, *beats, 15) == want
    # onset_backtrack: the restatement's, duplicates kept, and empty in, empty out
    rng = np.random.default_rng(5)
    for _ in range(8):
        e = np.round(rng.uniform(0, 4, 40), 1)
        ev = np.sort(rng.choice(40, 6, replace=False))
        assert np.array_equal(ao.onset_backtrack(ev, e), R.onset_backtrack(ev, e))
    assert np.array_equal(ao.onset_backtrack([5, 6], [3, 2, 1, 2, 3, 4, 5, 6.0]), [2, 2])
    assert ao.onset_backtrack([], np.ones(8)).size == 0


def test_restatement_edges():
    """What the chain's definition fixes without a spectrum: frame counts, the padding, the truncated windows, the backtrack."""
    assert [R.n_frames(L) for L in (36267, 1025, 2048, 512 * 40, 100000)] == [71, 3, 5, 41, 196]
    y = np.arange(1, 1026, dtype=np.float64)
    fr = R.frames(y, "reflect")
    assert fr.shape == (3, 2048) and fr[0, 0] == 1025 and fr[0, 1023] == 2 and fr[0, 1024] == 1 and fr[2, -1] == 2
    assert not R.frames(y, "constant")[0, :1024].any()
    with pytest.raises(ValueError):
        R.frames(y[:1024], "reflect")
    x = np.array([0, 0, 1, 1, 0, 0, 0, 0.5, 0, 0, 0, 0.0])
    mx, avg = R.moving_max_and_mean(x, 1, 1, 4, 5)
    assert np.array_equal(mx, [0, 0, 1, 1, 1, 0, 0, 0.5, 0.5, 0, 0, 0])
    assert np.allclose(avg, [np.mean(x[max(0, n - 4): n + 5]) for n in range(12)], rtol=0, atol=1e-15)
    assert list(R.onset_detect_envelope(x, 16000)) == [2, 3, 7] and list(R.onset_detect_envelope(x, 22050)) == [2, 7]
    assert R.onset_detect_envelope(np.zeros(12)).size == 0 and R.onset_detect_envelope(np.full(12, 0.5)).size == 0
    assert list(R.minima([2, 1, 3, 0.5, 0.5, 4, 1, 1, 0.25, 5, 0, 6])) == [0, 1, 4, 8, 10]
    y32 = R.test_clip(7, 36267)
    assert y32.dtype == np.float32 and R.onset_strength(y32, 16000, dtype=np.float32).dtype == np.float32
    o64, o32 = R.onset_strength(y32, 16000), R.onset_strength(y32, 16000, dtype=np.float32)
    assert np.abs(R.normalise(o32.astype(np.float64)) - R.normalise(o64)).max() < 1e-5
    assert np.array_equal(R.onset_detect_envelope(o64, 16000), R.onset_detect_envelope(o32, 16000))


def test_restatement_against_librosa_where_it_is_installed():
    """Skipped without librosa; 0.9.2 is what the reference pins and what the defaults follow."""
    librosa = pytest.importorskip("librosa")
    old = tuple(int(v) for v in librosa.__version__.split(".")[:2]) < (0, 10)
    for seed in range(3):
        y = R.test_clip(seed, 36267)
        fmax = R.FMAX_092 if old else 8000.0
        oenv = librosa.onset.onset_strength(y=y, sr=16000)
        assert np.abs(R.normalise(np.float64(oenv)) - R.normalise(R.onset_strength(y, 16000, fmax=fmax))).max() < 1e-4
        want = librosa.onset.onset_detect(onset_envelope=oenv, sr=16000)
        assert np.array_equal(R.onset_detect_envelope(np.float64(oenv), 16000), want)
        assert np.array_equal(R.onset_backtrack(want, oenv), librosa.onset.onset_backtrack(want, oenv))
        S = np.abs(librosa.stft(y=y, pad_mode="constant"))
        e = librosa.feature.rms(S=S)[0]
        assert np.abs(e - R.rms(y)).max() < 1e-5 * e.max()
        assert np.array_equal(R.mel_filterbank(16000, fmax=fmax), librosa.filters.mel(sr=16000, n_fft=2048, fmax=fmax))
