"""The audio front end, host side: the restatement (tests/resample_restatement.py) against scipy, the library's taps against numpy, the
plan of the outputs a push emits against its definition, the plan's unit under the host sanitizers (tests/resample_plan_main.cpp, a
stand-alone program), the ABI of the two new structs, every refusal of the ls_resample* entries with no device present, the Python
surface's argument errors and the WAV reader.  No GPU."""
import ctypes
import os
import re
import subprocess
import wave

import numpy as np
import pytest

import resample_restatement as rr
from livelyspeaker_amd import _lib, audio_io, build, long_form
from test_long_form_host import _no_engine, _parts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RATES = (48000, 44100, 22050, 8000, 16000)


@pytest.mark.parametrize("sr", RATES)
def test_restatement_is_resample_poly(sr):
    """Both are double sums of at most 2 half + 1 terms of order 1: agreement to 1e-12 max|y|."""
    ss = pytest.importorskip("scipy.signal")
    x = np.random.default_rng(sr).standard_normal(1000)
    up, down, half = rr.ratio(sr, 16000, 4)
    h = rr.design(up, down, 4)
    y, _ = rr.resample_sr(x, sr, 16000, 4, h)
    z = ss.resample_poly(x, up, down, window=h / up)
    assert y.shape == z.shape
    err = np.abs(y - z).max()
    print(f"{sr}: {2 * half + 1} taps, max error {err:.3g}")
    assert err <= 1e-12 * np.abs(y).max()


@pytest.mark.parametrize("zeros", [4, 32])
@pytest.mark.parametrize("sr", RATES)
def test_taps_are_the_definition(sr, zeros):
    """h64 against np.sinc / np.kaiser to 1e-12 max|h| (double rounding of a sine below about 100 rad and of an I0 series: 1e-14
    relative), and h32 its rounding wherever h64 is not within 1e-12 |h64| of a rounding tie."""
    h64, h32, r = audio_io.resample_taps(sr, 16000, zeros)
    up, down, half = rr.ratio(sr, 16000, zeros)
    assert (r["up"], r["down"], r["half"], r["n_taps"]) == (up, down, half, 2 * half + 1)
    assert r["taps_per_output"] == 2 * half // up + 1 and r["carry_len"] == -((-(2 * half + down)) // up) + 1
    want = rr.design(up, down, zeros)
    assert h64.shape == want.shape == h32.shape and h32.dtype == np.float32
    err = np.abs(h64 - want).max()
    print(f"{sr} Hz, {zeros} zeros: {h64.size} taps, max error {err:.3g} of {np.abs(want).max():.3g}")
    assert err <= 1e-12 * np.abs(want).max()
    lo = np.nextafter(h64.astype(np.float32), np.float32(-np.inf)).astype(np.float64)
    hi = np.nextafter(h64.astype(np.float32), np.float32(np.inf)).astype(np.float64)
    near = h64.astype(np.float32).astype(np.float64)
    tie = np.minimum(np.abs(h64 - (lo + near) / 2), np.abs(h64 - (hi + near) / 2)) <= 1e-12 * np.abs(h64)
    assert (h32 == h64.astype(np.float32))[~tie].all()
    if zeros == 32:                                                        # the DC gain at the defaults
        print(f"DC gain - 1 = {h64.sum() / up - 1:.3g}")
        assert abs(h64.sum() / up - 1) <= 1e-6


@pytest.mark.parametrize("zeros", [1, 4, 32])
@pytest.mark.parametrize("sr", [48000, 44100, 8000, 11025, 16000])
def test_plan_tiles_the_outputs_once_and_in_order(sr, zeros):
    up, down, half = rr.ratio(sr, 16000, zeros)
    rng = np.random.default_rng(sr + zeros)
    for L in (1, 2, 97, 3000):
        for trial in range(4):
            cuts = np.sort(rng.integers(0, L + 1, size=int(rng.integers(0, 12))))
            if trial == 3:                                                  # empty pushes among them
                cuts = np.sort(np.concatenate([cuts, cuts[:3]]))
            edges = np.concatenate([[0], cuts, [L]])
            n = nxt = 0
            for a, b in zip(edges[:-1], edges[1:]):
                first, count = _lib.resample_ratio_plan(up, down, half, n, int(b - a))
                assert first == nxt and count >= 0
                n, nxt = int(b), nxt + count
                assert nxt == rr.decided(n, up, down, half) <= -((-n * up) // down)          # D by its definition, and below the finish
                assert nxt == 0 or ((nxt - 1) * down + half) // up <= n - 1                    # every sample of an emitted output is there
            first, count = _lib.resample_ratio_plan(up, down, half, L, 0, True)
            assert first == nxt and first + count == -((-L * up) // down)
    d = [_lib.resample_ratio_plan(up, down, half, 0, n)[1] for n in range(0, 400)]
    assert all(a <= b for a, b in zip(d[:-1], d[1:]))                       # D is monotone
    assert audio_io.resample_plan(sr, 16000, 0, 3000, True, zeros) == (0, -((-3000 * up) // down))
    if sr == 16000:                                                         # the pass-through emits every sample at once
        assert audio_io.resample_plan(sr, 16000, 5, 7, False, zeros) == (5, 7)


def test_plan_ratio_and_taps_refusals():
    lib = _lib.load_library()
    a, b = ctypes.c_int64(), ctypes.c_int64()

    def plan(up, down, half, before, new, fin, f=a, c=b):
        return lib.ls_resample_plan(up, down, half, before, new, fin, ctypes.byref(f) if f is not None else None, ctypes.byref(c) if c is not None else None)

    assert plan(1, 3, 96, 0, 97, 0) == 0 and (a.value, b.value) == (0, 1)
    assert plan(1, 3, 96, 0, 5, 0, f=None) == -1 and plan(1, 3, 96, 0, 5, 0, c=None) == -1
    assert plan(0, 3, 96, 0, 5, 0) == -1 and plan(1, 0, 96, 0, 5, 0) == -1 and plan(1, 3, -1, 0, 5, 0) == -1
    assert plan(1, 3, 96, -1, 5, 0) == -1 and plan(1, 3, 96, 5, -1, 0) == -1
    assert plan(1, 3, 96, 0, 0, 1) == -1 and plan(1, 3, 96, 0, 1, 1) == 0                     # a finish needs a sample
    assert plan(1, 3, 96, 2 ** 62, 0, 0) == 0 and plan(1, 3, 96, 2 ** 62, 1, 0) == -1 and plan(1, 3, 96, 2 ** 62 + 1, 0, 0) == -1
    assert plan(160, 441, 14112, 2 ** 62 // 160 + 1, 0, 0) == -1 and plan(2 ** 62 + 1, 1, 0, 0, 0, 0) == -1
    v = [ctypes.c_int64() for _ in range(6)]
    ratio = lambda i, o, z, holes=(): lib.ls_resample_ratio(i, o, z, *[None if k in holes else ctypes.byref(x) for k, x in enumerate(v)])      # noqa: E731
    assert ratio(48000, 16000, 32) == 0 and [x.value for x in v] == [1, 3, 96, 193, 196, 193]
    assert ratio(0, 16000, 32) == -1 and ratio(48000, 0, 32) == -1 and ratio(48000, 16000, 0) == -1 and ratio(-5, 16000, 32) == -1
    assert all(ratio(48000, 16000, 32, holes=(k,)) == -1 for k in range(6))
    assert ratio(65535, 1, 32) == 0 and ratio(65536, 1, 32) == -5 and ratio(1, 65536, 32) == -5       # n_taps above 2^22: LS_EUNSUPPORTED
    h64, h32 = np.zeros(9), np.zeros(9, np.float32)
    p64, p32 = h64.ctypes.data_as(_lib.c_f64p), h32.ctypes.data_as(_lib.c_f32p)
    taps = lib.ls_resample_taps
    assert taps(1, 1, 4, 12.0, 0.95, p64, p32) == 0 and taps(1, 1, 4, 12.0, 0.95, None, None) == -1
    assert taps(1, 1, 4, 12.0, 0.95, p64, None) == 0 and taps(1, 1, 4, 12.0, 0.95, None, p32) == 0
    assert taps(0, 1, 4, 12.0, 0.95, p64, p32) == -1 and taps(1, 0, 4, 12.0, 0.95, p64, p32) == -1 and taps(1, 1, 0, 12.0, 0.95, p64, p32) == -1
    assert taps(1, 1, 4, -0.5, 0.95, p64, p32) == -1 and taps(1, 1, 4, 12.0, 0.0, p64, p32) == -1 and taps(1, 1, 4, 12.0, 1.01, p64, p32) == -1
    assert taps(1, 1, 4, float("nan"), 0.95, p64, p32) == -1 and taps(1, 65536, 32, 12.0, 0.95, p64, p32) == -5
    with pytest.raises(ValueError):
        _lib.resample_ratio_plan(1, 3, 96, 0, 0, True)
    with pytest.raises(ValueError):
        _lib.resample_ratio(48000.5, 16000)
    with pytest.raises(_lib.EngineError, match="2\\^22"):
        _lib.resample_ratio(65536, 1)
    with pytest.raises(ValueError):
        _lib.resample_taps(1, 3, rolloff=0.0)


def test_plan_on_its_edges_under_asan_and_ubsan(tmp_path):
    """tests/resample_plan_main.cpp with the plan's unit, as plain C++ with the host sanitizers linked statically: a child process of its
    own, nothing preloaded, nothing inside Python, no GPU."""
    exe = str(tmp_path / "resample_plan")
    made = subprocess.run([build.hipcc_path(), "-x", "c++", "-std=c++17", "-O1", "-g", "-fno-gpu-sanitize", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "resample_plan_main.cpp"),
                           os.path.join(ROOT, "livelyspeaker_amd", "csrc", "ls_resample_plan.cpp"), "-o", exe], capture_output=True, text=True)
    assert made.returncode == 0, made.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr
    assert run.stderr == "", run.stderr


STRUCTS = (("ls_resample_args", _lib.LsResampleArgs), ("ls_resample_stream_push_args", _lib.LsResampleStreamPushArgs))
NEW_EXPORTS = ("ls_resample_ratio", "ls_resample_plan", "ls_resample_taps", "ls_resample", "ls_resample_stream_open", "ls_resample_stream_push",
               "ls_resample_stream_reset", "ls_resample_stream_info", "ls_resample_stream_close", "ls_resample_stream_last_error")


def test_abi_mirrors(tmp_path):
    lines = []
    for cname, cls in STRUCTS:
        lines.append(f'    printf("%zu", sizeof({cname}));\n')
        lines += [f'    printf(" %zu", offsetof({cname}, {n}));\n' for n, _ in cls._fields_]
        lines.append('    printf("\\n");\n')
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ls_hip.h"\nint main(void) {\n' + "".join(lines) +
                   '    printf("%d %d %d %d\\n", LS_ABI_VERSION, LS_RESAMPLE_F32, LS_RESAMPLE_I16, LS_RESAMPLE_MAX_CHANNELS);\n    return 0;\n}\n')
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [[int(v) for v in line.split()] for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()]
    for row, (cname, cls) in zip(got, STRUCTS):
        assert row == [ctypes.sizeof(cls)] + [getattr(cls, n).offset for n, _ in cls._fields_], cname
    assert got[2] == [5, _lib.RESAMPLE_DTYPES["float32"], _lib.RESAMPLE_DTYPES["int16"], _lib.RESAMPLE_MAX_CHANNELS]
    hdr = open(os.path.join(ROOT, "include", "ls_hip.h")).read()
    lib = ctypes.CDLL(_lib.library_path())
    for name in NEW_EXPORTS:
        assert name in _lib.EXPORTS and re.search(rf"\b{name}\s*\(", hdr) and hasattr(lib, name), name
    for src_name in ("ls_resample.hip", "ls_resample_api.cpp", "ls_resample_plan.cpp"):
        assert src_name in build.SOURCES


def _args(**over):
    """ls_resample_args for one clip of 100 mono float32 frames at 48 kHz on the host, with ``over`` on top; keeps its arrays alive."""
    x, lens, out, got = np.zeros(100, np.float32), np.array([100], np.int64), np.zeros(40, np.float32), np.zeros(1, np.int64)
    a = _lib.LsResampleArgs()
    a.batch, a.on_device, a.dtype, a.channels, a.row_stride = 1, 0, 0, 1, 100
    a.audio, a.lengths = x.ctypes.data, lens.ctypes.data_as(_lib.c_i64p)
    a.in_sr, a.out_sr, a.zeros, a.beta, a.rolloff = 48000, 16000, 32, 12.0, 0.95
    a.out, a.out_stride, a.out_lengths = out.ctypes.data, 40, got.ctypes.data_as(_lib.c_i64p)
    a._keep = (x, lens, out, got)
    for k, v in over.items():
        if k == "length":
            lens[0] = v
        else:
            setattr(a, k, v)
    return a


def test_one_shot_refuses_ahead_of_any_device_call():
    lib = _lib.load_library()
    msg = lambda: lib.ls_resample_stream_last_error(None).decode()      # noqa: E731
    assert lib.ls_resample(0, None) == -1
    for bad in (dict(audio=None), dict(lengths=None), dict(out=None), dict(batch=0), dict(batch=65536), dict(dtype=2), dict(dtype=-1), dict(channels=0),
                dict(channels=9), dict(in_sr=0), dict(out_sr=0), dict(zeros=0), dict(beta=-1.0), dict(rolloff=0.0), dict(rolloff=1.5), dict(row_stride=0),
                dict(out_stride=0), dict(length=0), dict(length=101), dict(length=2 ** 31), dict(out_stride=33), dict(channels=2, length=51)):
        assert lib.ls_resample(0, ctypes.byref(_args(**bad))) == -1, bad
        assert msg().startswith("ls_resample"), bad
    assert lib.ls_resample(0, ctypes.byref(_args(in_sr=65536, out_sr=1))) == -5 and "4194304" in msg()      # LS_EUNSUPPORTED, the count named
    good = _args()
    rc = lib.ls_resample(0, ctypes.byref(good))                             # every check passed: the device, or the lack of one
    assert rc in (0, -3) and good._keep[3][0] == 34


def test_stream_refuses_ahead_of_any_device_call():
    lib = _lib.load_library()
    h = ctypes.c_void_p()

    def rc(capacity=2, in_sr=48000, out_sr=16000, channels=1, dtype=0, zeros=32, beta=12.0, rolloff=0.95, max_chunk=4096, out=h):
        return lib.ls_resample_stream_open(0, capacity, in_sr, out_sr, channels, dtype, zeros, beta, rolloff, max_chunk, ctypes.byref(out) if out is not None else None)

    assert rc(out=None) == -1
    for bad in (dict(capacity=0), dict(in_sr=0), dict(out_sr=-1), dict(channels=0), dict(channels=9), dict(dtype=2), dict(zeros=0), dict(beta=-0.1),
                dict(rolloff=0.0), dict(rolloff=2.0), dict(max_chunk=0)):
        assert rc(**bad) == -1, bad
        assert lib.ls_resample_stream_last_error(None).decode().startswith("ls_resample_stream_open")
    assert rc(in_sr=65536, out_sr=1) == -5 and "above 2^22" in lib.ls_resample_stream_last_error(None).decode()
    assert not h.value
    assert lib.ls_resample_stream_push(None, None) == -1 and lib.ls_resample_stream_reset(None, 0) == -1
    assert lib.ls_resample_stream_info(None, None, None, None) == -1
    lib.ls_resample_stream_close(None)


def test_every_refusal_sits_in_front_of_the_device():
    """In the three entries no line that returns LS_EINVAL or LS_ESTATE follows a HIP call: the device work lives in helpers (run,
    allocate, push) that the entries call once every check has passed."""
    src = open(os.path.join(ROOT, "livelyspeaker_amd", "csrc", "ls_resample_api.cpp")).read()
    for entry, helper in (("int ls_resample(", "no_device(\"ls_resample\""), ("int ls_resample_stream_open(", "no_device(\"ls_resample_stream_open\""),
                          ("int ls_resample_stream_push(", "push(h, a,")):
        body = src[src.index(entry):]
        body = body[:body.index("\n}\n")]
        head, tail = body[:body.index(helper)], body[body.index(helper):]
        assert "LS_EINVAL" not in tail and "LS_ESTATE" not in tail, entry
        assert not re.findall(r"\bhip[A-Z]\w+", head), entry
    for helper in ("int run(", "int allocate(H* h)", "int push(H* h"):
        body = src[src.index(helper):]
        body = body[:body.index("\n}\n")]
        assert "LS_EINVAL" not in body and "LS_ESTATE" not in body, helper
    body = src[src.index("int ls_resample_stream_reset("):]
    assert not re.findall(r"\bhip[A-Z]\w+", body[:body.index("\n}\n")])


def test_python_surface_refuses_before_a_device_is_touched(monkeypatch):
    monkeypatch.setattr(_lib, "ResampleStreamEngine", lambda *a, **k: (_ for _ in ()).throw(AssertionError("an engine was opened")))
    x = np.zeros((2, 100), np.float32)
    for bad in (x.astype(np.float64), x.astype(np.int32), x[0], np.zeros((2, 100, 2, 1), np.float32), np.zeros((2, 100, 9), np.float32),
                np.zeros((2, 0), np.float32), [[0.0] * 4] * 2):
        with pytest.raises(ValueError):
            audio_io.resample(bad, 48000)
    for kw in (dict(in_sr=0), dict(in_sr=48000.5), dict(in_sr=48000, out_sr=0), dict(in_sr=48000, zeros=0), dict(in_sr=48000, beta=-1.0),
               dict(in_sr=48000, rolloff=0.0), dict(in_sr=48000, lengths=[100]), dict(in_sr=48000, lengths=[100, 101]), dict(in_sr=48000, lengths=[0, 5])):
        with pytest.raises(ValueError):
            audio_io.resample(x, **kw)
    with pytest.raises(_lib.EngineError, match="2\\^22"):
        audio_io.resample(x, 65536, 1)
    for kw in (dict(capacity=0), dict(in_sr=0), dict(channels=0), dict(channels=9), dict(channels=True), dict(dtype="float64"), dict(max_chunk=0),
               dict(zeros=0), dict(rolloff=1.5), dict(beta=-2.0)):
        full = dict(capacity=2, in_sr=48000)
        full.update(kw)
        with pytest.raises(ValueError):
            audio_io.open_resample_stream(**full)
    rs = audio_io.open_resample_stream(2, 48000, channels=2, dtype="int16", max_chunk=512)
    assert rs.samples_in.tolist() == [0, 0] and rs.outputs_done.tolist() == [0, 0] and rs.ratio["carry_len"] == 196
    stereo = np.zeros((2, 100, 2), np.int16)
    for bad in (stereo.astype(np.float32), stereo[:, :, 0], stereo[:1], np.zeros((2, 513, 2), np.int16)):
        with pytest.raises(ValueError):
            rs.push(bad)
    with pytest.raises(ValueError, match="lengths"):
        rs.push(stereo, lengths=[100, 101])
    with pytest.raises(ValueError, match="lengths"):
        rs.push(lengths=[1, 0])
    with pytest.raises(ValueError, match="finish"):
        rs.push(stereo, finish=[True])
    with pytest.raises(ValueError, match="no sample"):
        rs.push(stereo, lengths=[0, 5], finish=[True, False])
    with pytest.raises(ValueError, match="no sample"):
        rs.finish(0)
    with pytest.raises(ValueError):
        rs.reset(2)
    rs.reset(1)                                                             # an empty slot: a no-op, and no engine
    got = rs.push(stereo, lengths=[0, 0])                                   # an empty push: nothing runs
    assert got["audio"].shape == (2, 0) and got["out_count"].tolist() == [0, 0] and rs._eng is None
    rs.close()
    with pytest.raises(RuntimeError):
        rs.push(stereo)


@pytest.mark.parametrize("ds", ["ted", "beat"])
def test_sessions_refuse_input_sr_arguments(ds, monkeypatch):
    _no_engine(monkeypatch)
    monkeypatch.setattr(_lib, "ResampleStreamEngine", lambda *a, **k: (_ for _ in ()).throw(AssertionError("an engine was opened")))
    cfg, model, diffusion = _parts(ds)
    from livelyspeaker_amd import synth
    y = synth.make_long_cond(cfg, 2, 2)
    emo = None if y.get("emo") is None else y["emo"][:, 0]
    args = (diffusion, model, y["seed_poses"], y["vid_indices"], y["scale"])
    for bad in (dict(input_sr=0), dict(input_sr=44100.5), dict(input_sr=48000, input_channels=0), dict(input_sr=48000, input_channels=9),
                dict(input_channels=2), dict(resample={"zeros": 4}), dict(input_sr=48000, resample={"zeros": 0}),
                dict(input_sr=48000, resample={"window": "hann"}), dict(input_sr=48000, resample={"max_chunk": 0})):
        with pytest.raises(ValueError):
            long_form.open_stream(*args, emo=emo, **bad)
        with pytest.raises(ValueError):
            long_form.open_pool(diffusion, model, 2, **bad)
    diffusion.noise_source = "torch_device"                                 # refused as the session already refuses it
    with pytest.raises(NotImplementedError):
        long_form.open_stream(*args, emo=emo, input_sr=48000)
    with pytest.raises(NotImplementedError):
        long_form.open_pool(diffusion, model, 2, input_sr=48000)
    diffusion.noise_source = "torch_cpu"
    st = long_form.open_stream(*args, emo=emo, input_sr=48000, input_channels=2, resample={"zeros": 16})
    assert st._in.capacity == 2 and st._in.channels == 2 and st._in.ratio["half"] == 48 and st.input_samples_in == 0
    assert long_form.open_stream(*args, emo=emo)._in is None
    pool = long_form.open_pool(diffusion, model, 3, input_sr=44100)
    assert pool._in.capacity == 3 and pool.slots["input_samples_in"].tolist() == [0, 0, 0]
    assert "input_samples_in" not in long_form.open_pool(diffusion, model, 3).slots


@pytest.mark.parametrize("ds", ["ted", "beat"])
def test_a_refused_push_leaves_the_resampler_as_it_was(ds, monkeypatch):
    """The session's own refusals come before its resampler is fed: the chunk is checked and its 16 kHz count planned on the host,
    and the samples go in only once nothing can refuse the call.  (What needs a running series: tests/test_gpu_long_stream_sr.py.)"""
    _no_engine(monkeypatch)
    monkeypatch.setattr(_lib, "ResampleStreamEngine", lambda *a, **k: (_ for _ in ()).throw(AssertionError("an engine was opened")))
    cfg, model, diffusion = _parts(ds)
    from livelyspeaker_amd import synth
    y = synth.make_long_cond(cfg, 2, 2)
    args = (diffusion, model, y["seed_poses"], y["vid_indices"], y["scale"])
    n = 3 * cfg.audio_len + 400                                             # enough at 48 kHz for window 0
    chunk = np.zeros((2, n, 2), np.int16)
    st = long_form.open_stream(*args, input_sr=48000, input_channels=2, resample={"max_chunk": n})
    pool = long_form.open_pool(diffusion, model, 2, input_sr=48000, input_channels=2, resample={"max_chunk": n})
    assert audio_io.resample_plan(48000, 16000, 0, n)[1] >= cfg.audio_len
    bad = [dict(text_features=np.zeros((2, 512), np.float32)),              # no sag
           dict(emo=np.zeros(3, np.int64))]                                 # TED: no emo at all; BEAT: one id per clip
    if ds == "beat":
        bad.append({})                                                      # the first window needs an emotion id
    for kw in bad:
        with pytest.raises(ValueError):
            st.push(chunk, **kw)
        assert st.input_samples_in == 0 and st.samples_in == 0 and st._in.samples_in.tolist() == [0, 0] and st._in.dtype is None
    with pytest.raises(ValueError):
        st.push(chunk[:, :, :1])                                            # the resampler's own refusal: one channel, opened for two
    with pytest.raises(ValueError, match="not open"):
        pool.push(chunk, [n, 0])
    assert pool._in.samples_in.tolist() == [0, 0] and pool._in.dtype is None and st._in.samples_in.tolist() == [0, 0]


def _write_wav(path, data, sr, width=2):
    with wave.open(str(path), "wb") as w:
        w.setnchannels(data.shape[1])
        w.setsampwidth(width)
        w.setframerate(sr)
        w.writeframes(data.tobytes())


def test_read_wav_and_load(tmp_path, monkeypatch):
    rng = np.random.default_rng(3)
    mono = rng.integers(-32768, 32768, size=(1234, 1)).astype("<i2")
    stereo = rng.integers(-32768, 32768, size=(777, 2)).astype("<i2")
    _write_wav(tmp_path / "mono.wav", mono, 44100)
    _write_wav(tmp_path / "stereo.wav", stereo, 48000)
    _write_wav(tmp_path / "bytes.wav", rng.integers(0, 256, size=(50, 1)).astype(np.uint8), 8000, width=1)
    (tmp_path / "text.wav").write_bytes(b"not a wave file at all")
    got, sr = audio_io.read_wav(tmp_path / "mono.wav")
    assert sr == 44100 and got.dtype == np.int16 and (got == mono).all()
    got, sr = audio_io.read_wav(str(tmp_path / "stereo.wav"))
    assert sr == 48000 and got.shape == (777, 2) and (got == stereo).all()
    with pytest.raises(ValueError, match="8-bit"):
        audio_io.read_wav(tmp_path / "bytes.wav")
    with pytest.raises(ValueError, match="16-bit PCM"):
        audio_io.read_wav(tmp_path / "text.wav")
    seen = {}

    def fake(audio, in_sr, out_sr=16000, device=0, **kw):
        seen.update(audio=audio, in_sr=in_sr, out_sr=out_sr, device=device)
        return np.arange(12, dtype=np.float32)[None], np.array([10])

    monkeypatch.setattr(audio_io, "resample", fake)
    y = audio_io.load(tmp_path / "stereo.wav", sr=22050, device=1)
    assert y.dtype == np.float32 and (y == np.arange(10)).all()
    assert seen["audio"].shape == (1, 777, 2) and seen["audio"].dtype == np.int16 and (seen["audio"][0] == stereo).all()
    assert (seen["in_sr"], seen["out_sr"], seen["device"]) == (48000, 22050, 1)
    assert "NOT its bits" in audio_io.load.__doc__
