"""The resampler on the GPU (audio_io.resample -> ls_resample, audio_io.open_resample_stream -> ls_resample_stream_*; csrc/ls_resample.hip).

One-shot: every output against the float64 restatement (tests/resample_restatement.py) fed the library's own float32 taps and the float32
mixdown, within the bound a chain of T fused multiply-adds obeys whatever its order -- |y - y64| <= (T + 2) 2^-24 sum_k |h_k| |x_k|, T
= taps_per_output -- which is derived, not measured.  B = 3 clips of 1, 997 and 3000 frames: half exceeds the first, and at 32 zeros the
taps of one output span tiles.  The four rates take the kernel's three forms: taps in LDS (48 kHz, 8 kHz), taps from global memory
(44.1 kHz, 22.05 kHz), and, at 600 zeros, a tile whose samples do not fit the LDS stage.
Stream: bit for bit the one-shot call under any chunking, per slot."""
import functools

import numpy as np
import pytest
import torch

import resample_restatement as rr
from livelyspeaker_amd import _lib, audio_io

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LENGTHS = (1, 997, 3000)
N = 3000
FORMATS = {"f32": (np.float32, 1), "f32x2": (np.float32, 2), "i16": (np.int16, 1), "i16x3": (np.int16, 3)}
U = 2.0 ** -24


@functools.lru_cache(maxsize=None)
def _audio(fmt, rows=3, seed=0):
    """[rows, N] or [rows, N, C]; left unchanged by every test."""
    dtype, C = FORMATS[fmt]
    rng = np.random.default_rng(seed + 17 * C)
    shape = (rows, N) if C == 1 else (rows, N, C)
    x = rng.uniform(-1, 1, size=shape).astype(np.float32) if dtype == np.float32 else rng.integers(-32768, 32768, size=shape).astype(np.int16)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def _reference(fmt, sr, zeros):
    """Per clip ``(y64, mag)`` of the restatement on the float32 mixdown with the library's float32 taps, and the ratio."""
    _, h32, r = audio_io.resample_taps(sr, 16000, zeros)
    mono = rr.mixdown(_audio(fmt))
    return [rr.resample_sr(mono[b, :n], sr, 16000, zeros, h32.astype(np.float64)) for b, n in enumerate(LENGTHS)], r


def _poisoned(fmt):
    """The audio with what lies behind each clip's length made unmistakable: NaN (float32) or full scale (int16)."""
    x = _audio(fmt).copy()
    for b, n in enumerate(LENGTHS):
        x[b, n:] = np.nan if x.dtype == np.float32 else 32767
    return x


def _check_against_restatement(y, n_out, fmt, sr, zeros):
    ref, r = _reference(fmt, sr, zeros)
    T = r["taps_per_output"]
    y = y.cpu().numpy() if torch.is_tensor(y) else y
    worst = 0.0
    for b, (y64, mag) in enumerate(ref):
        assert n_out[b] == y64.size == _lib.resample_ratio_plan(r["up"], r["down"], r["half"], 0, LENGTHS[b], True)[1]
        got = y[b, :y64.size].astype(np.float64)
        assert np.isfinite(got).all() and (y[b, y64.size:] == 0).all()          # exactly 0 behind a clip's outputs
        bound = (T + 2) * U * mag
        worst = max(worst, float(np.max(np.abs(got - y64) / np.maximum(bound, 1e-300))))
        assert (np.abs(got - y64) <= bound).all(), (b, float(np.abs(got - y64).max()))
    return worst, T


@pytest.mark.parametrize("fmt", list(FORMATS))
@pytest.mark.parametrize("zeros", [4, 32])
@pytest.mark.parametrize("sr", [48000, 44100, 8000, 22050])
def test_one_shot_against_the_restatement(sr, zeros, fmt):
    x = torch.from_numpy(_poisoned(fmt)).to(DEV)
    y, n_out = audio_io.resample(x, sr, lengths=LENGTHS, zeros=zeros)
    assert y.is_cuda and y.dtype == torch.float32 and y.shape == (3, int(n_out.max()))
    worst, T = _check_against_restatement(y, n_out, fmt, sr, zeros)
    print(f"{sr} Hz, {zeros} zeros, {fmt}: T = {T}, worst error / bound = {worst:.3f}")


def test_a_tile_that_does_not_fit_the_stage():
    """48 kHz at 600 zeros: 3601 taps per output, so the samples of a 256-output tile (765 + 3604) pass the 4096 the stage holds and
    the kernel reads through the fetch; same bound, and the stream gives the same bits."""
    x = torch.from_numpy(_poisoned("f32x2")).to(DEV)
    y, n_out = audio_io.resample(x, 48000, lengths=LENGTHS, zeros=600)
    worst, T = _check_against_restatement(y, n_out, "f32x2", 48000, 600)
    assert T == 3601
    print(f"48000 Hz, 600 zeros: worst error / bound = {worst:.3f}")
    with audio_io.open_resample_stream(1, 48000, channels=2, zeros=600, max_chunk=4096) as rs:
        clip = torch.from_numpy(_audio("f32x2")[2:3].copy()).to(DEV)
        a = rs.push(clip[:, :1801])
        b = rs.push(clip[:, 1801:], finish=[True])
        got = torch.cat([a["audio"][0, :a["out_count"][0]], b["audio"][0, :b["out_count"][0]]])
        assert int(a["out_count"][0]) > 0 and torch.equal(got, y[2, :n_out[2]])


@pytest.mark.parametrize("sr", [48000, 44100, 8000, 22050])
def test_a_clip_alone_and_a_host_input_give_the_same_bits(sr):
    for fmt in ("f32x2", "i16x3"):
        x = _poisoned(fmt)
        y, n_out = audio_io.resample(torch.from_numpy(x).to(DEV), sr, lengths=LENGTHS)
        host, n_host = audio_io.resample(x, sr, lengths=LENGTHS)
        assert isinstance(host, np.ndarray) and (n_host == n_out).all() and np.array_equal(host, y.cpu().numpy())
        for b, n in enumerate(LENGTHS):
            alone, n_alone = audio_io.resample(torch.from_numpy(_audio(fmt)[b:b + 1, :n].copy()).to(DEV), sr)
            assert n_alone[0] == n_out[b] and torch.equal(alone[0], y[b, :n_out[b]]), (fmt, b)


@pytest.mark.parametrize("fmt", list(FORMATS))
def test_pass_through_is_the_mixdown(fmt):
    x = _poisoned(fmt)
    y, n_out = audio_io.resample(torch.from_numpy(x).to(DEV), 16000, lengths=LENGTHS)
    want = rr.mixdown(_audio(fmt))
    assert n_out.tolist() == list(LENGTHS) and y.shape == (3, N)
    for b, n in enumerate(LENGTHS):
        assert np.array_equal(y[b, :n].cpu().numpy(), want[b, :n]) and bool((y[b, n:] == 0).all())
    with audio_io.open_resample_stream(3, 16000, channels=FORMATS[fmt][1], dtype=None) as rs:      # the stream's pass-through: every sample at once
        got = rs.push(x[:, :700], lengths=[1, 700, 700])
        assert got["out_count"].tolist() == [1, 700, 700] and np.array_equal(got["audio"][1], want[1, :700])


def _one_shot(series, sr):
    y, n = audio_io.resample(torch.from_numpy(np.array(series[None])).to(DEV), sr)
    return y[0, :n[0]].cpu().numpy()


@pytest.mark.parametrize("sr,fmt,on_device", [(48000, "i16x3", True), (44100, "f32", False), (48000, "f32x2", False), (44100, "i16", True)])
def test_stream_is_bitwise_the_one_shot_call_under_any_chunking(sr, fmt, on_device):
    series = _audio(fmt)[2]                                                   # one series of 3000 frames for every slot
    r = _lib.resample_ratio(sr, 16000)
    whole, head = _one_shot(series, sr), _one_shot(series[:1200], sr)
    cuts = [0, 1, 2, 700, 701, 1500, 2999, N]
    # per slot: (frames, finish) per push.  Slot 0: single samples for the first 50; slot 1: the cuts; slot 2: a first series of 1200
    # frames that finishes mid-way, empty pushes, then the whole series in one push and a finish without a sample
    script = [[(1, False)] * 50 + [(N - 50, True)],
              [(b - a, b == N) for a, b in zip(cuts[:-1], cuts[1:])],
              [(1200, False), (0, True), (0, False), (0, False), (N, False), (0, False), (0, True)]]
    rs = audio_io.open_resample_stream(3, sr, channels=FORMATS[fmt][1], dtype=None, max_chunk=4096)
    fed, done, pos = np.zeros(3, np.int64), np.zeros(3, np.int64), np.zeros(3, np.int64)
    series_out, outs, bytes_seen = [[[]], [[]], [[]]], None, set()
    for step in range(max(len(s) for s in script)):
        lens = np.array([s[step][0] if step < len(s) else 0 for s in script])
        fin = np.array([s[step][1] if step < len(s) else False for s in script])
        chunk = np.zeros((3, int(lens.max())) + series.shape[1:], series.dtype)
        for s in range(3):
            chunk[s, :lens[s]] = series[pos[s]:pos[s] + lens[s]]
        outs = rs.push(torch.from_numpy(chunk).to(DEV) if on_device else chunk, lens, fin)
        assert (_lib._is_cuda(outs["audio"]) == on_device) or not lens.any()
        audio = outs["audio"].cpu().numpy() if torch.is_tensor(outs["audio"]) else outs["audio"]
        for s in range(3):
            first, count = (done[s], 0) if not lens[s] and not fin[s] else _lib.resample_ratio_plan(r["up"], r["down"], r["half"], fed[s], lens[s], fin[s])
            assert (outs["out_first"][s], outs["out_count"][s]) == (first, count), (step, s)
            assert (audio[s, count:] == 0).all()
            series_out[s][-1].append(audio[s, :count].copy())
            fed[s], done[s], pos[s] = fed[s] + lens[s], first + count, pos[s] + lens[s]
            if fin[s]:
                fed[s] = done[s] = pos[s] = 0
                series_out[s].append([])
        assert rs.samples_in.tolist() == fed.tolist() and rs.outputs_done.tolist() == done.tolist()
        if rs._eng is not None:
            info = rs.info()
            assert info["samples_in"].tolist() == fed.tolist() and info["outputs_done"].tolist() == done.tolist()
            bytes_seen.add(info["device_bytes"])
    cat = lambda parts: np.concatenate(parts) if parts else np.zeros(0, np.float32)      # noqa: E731
    assert np.array_equal(cat(series_out[0][0]), whole) and np.array_equal(cat(series_out[1][0]), whole)
    assert np.array_equal(cat(series_out[2][0]), head)                          # the series that finished mid-way
    assert np.array_equal(cat(series_out[2][1]), whole)                         # ... and the one after it does not see it
    assert len(bytes_seen) == 1 and min(bytes_seen) > 0                         # nothing grows after the open
    # a slot that is reset mid-series emits nothing that was pending, and its next series is the one-shot call on it
    x = series[None].repeat(3, axis=0)
    put = (lambda a: torch.from_numpy(np.array(a)).to(DEV)) if on_device else np.ascontiguousarray
    first = rs.push(put(x[:, :500]), [0, 500, 0])
    assert first["out_count"][1] == _lib.resample_ratio_plan(r["up"], r["down"], r["half"], 0, 500)[1] < len(_one_shot(series[:500], sr))
    rs.reset(1)
    rs.reset(1)                                                                 # idempotent
    rs.reset(0)                                                                 # an empty slot: a no-op
    assert rs.samples_in.tolist() == [0, 0, 0] and rs.info()["samples_in"].tolist() == [0, 0, 0]
    a = rs.push(put(x[:, :1700]), [0, 1700, 0])
    b = rs.push(put(x[:, 1700:]), [0, N - 1700, 0], [False, True, False])
    assert a["out_first"][1] == 0 and (a["out_count"][[0, 2]] == 0).all()
    got = [np.asarray(o["audio"].cpu() if torch.is_tensor(o["audio"]) else o["audio"])[1, :o["out_count"][1]] for o in (a, b)]
    assert np.array_equal(np.concatenate(got), whole)
    assert rs.info()["device_bytes"] in bytes_seen
    with pytest.raises(ValueError, match="no sample"):
        rs.finish(1)
    tail = rs.push(put(x[:, :100]), [100, 0, 0])
    assert np.array_equal(np.concatenate([np.asarray(tail["audio"].cpu() if on_device else tail["audio"])[0, :tail["out_count"][0]],
                                          np.asarray(rs.finish(0, device_out=False))]), _one_shot(series[:100], sr))
    rs.close()


def test_the_engine_refuses_a_push_ahead_of_any_launch_and_stays_as_it_was():
    """ls_resample_stream_push's own refusals, behind the Python checks that keep them from ever being reached through
    ``ResampleStream``: LS_EINVAL with the message, and the handle's counts and bytes as before."""
    rs = audio_io.open_resample_stream(2, 48000, max_chunk=1000)
    x = np.ascontiguousarray(_audio("f32")[:2, :1000])
    rs.push(x, [1000, 0])                                                   # slot 0: 1000 frames in, 302 outputs; slot 1 empty
    eng = rs._engine()
    before = eng.info()
    assert before["samples_in"].tolist() == [1000, 0] and before["outputs_done"].tolist() == [302, 0]
    out, first, count = np.full((2, 400), 7.0, np.float32), np.full(2, -1, np.int64), np.full(2, -1, np.int64)

    def args(lens, n_max=1000, fin=None, audio=x, cap=400, dst=out):
        a = _lib.LsResampleStreamPushArgs()
        a._keep = (np.asarray(lens, np.int32), None if fin is None else np.asarray(fin, np.int32))
        a.on_device, a.n_max, a.out_capacity = 0, n_max, cap
        a.audio = None if audio is None else audio.ctypes.data
        a.lengths = a._keep[0].ctypes.data_as(_lib.c_i32p)
        a.finish = None if fin is None else a._keep[1].ctypes.data_as(_lib.c_i32p)
        a.out = None if dst is None else dst.ctypes.data
        a.out_first, a.out_count = first.ctypes.data_as(_lib.c_i64p), count.ctypes.data_as(_lib.c_i64p)
        return a

    for bad, message in ((args([10, 0], n_max=1001), r"n_max 1001 outside \[0, 1000\]"),
                         (args([10, 0], n_max=-1), r"n_max -1 outside"),
                         (args([1001, 0]), r"lengths\[0\] = 1001 outside \[0, 1000\]"),
                         (args([0, -1]), r"lengths\[1\] = -1 outside"),
                         (args([0, 0], fin=[0, 1]), r"no plan for slot 1 .*finished must hold a sample"),      # the plan refuses it
                         (args([900, 0], cap=299), r"slot 0 emits 300 outputs, out_capacity is 299"),
                         (args([900, 0], audio=None), r"lengths without audio"),
                         (args([900, 0], dst=None), r"outputs without out")):
        with pytest.raises(ValueError, match=r"\(-1\).*" + message):
            eng.push(bad)
    a = args([10, 0])
    a.lengths = None
    with pytest.raises(ValueError, match=r"\(-1\).*null argument"):
        eng.push(a)
    assert eng.lib.ls_resample_stream_push(eng.h, None) == -1
    for slot in (2, -1):                                                    # reset: a slot outside [0, capacity)
        assert eng.lib.ls_resample_stream_reset(eng.h, slot) == -1
        assert f"slot {slot} outside [0, 2)" in eng.lib.ls_resample_stream_last_error(eng.h).decode()
        with pytest.raises(ValueError, match="outside"):
            eng.reset(slot)
    after = eng.info()
    assert str(after) == str(before) and (out == 7.0).all()                 # nothing ran, nothing moved
    rest = rs.push(x[:, :900], [900, 0], [True, False])                     # and the series goes on as if nothing had been tried
    whole = _one_shot(np.concatenate([x[0], x[0, :900]]), 48000)
    assert rest["out_first"][0] == 302 and np.array_equal(rest["audio"][0, :rest["out_count"][0]], whole[302:])
    rs.close()
