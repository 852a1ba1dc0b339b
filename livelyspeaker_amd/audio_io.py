"""The audio front end: waveforms at any integer sample rate, mono or interleaved, float32 or int16, to the mono float32 16 kHz every
other entry point takes -- resampled on the device (csrc/ls_resample.hip), in one call or as a stream that carries its filter state
across chunks and gives bit for bit the whole-series call under any chunking.

    y, n_out = resample(audio, in_sr)                    # [B, n] or [B, n, C]  ->  [B, max(n_out)], int64 [B]
    rs = open_resample_stream(capacity, in_sr, channels=2, dtype='int16')
    got = rs.push(chunk, lengths)                        # {'audio' [S, K], 'out_first' [S], 'out_count' [S]}
    tail = rs.finish(slot)                               # what the end of the series still owes; the slot is free
    x = load('talk.wav')                                 # 16-bit PCM WAV -> mono float32 at 16 kHz

The filter (one definition, ``include/ls_hip.h``): a Kaiser-windowed sinc of ``zeros`` zero crossings per side at the lower of the two
rates, applied polyphase; ``resample_plan`` says which outputs a push decides, ``resample_taps`` gives the taps.  Not built: formats
other than 16-bit PCM WAV, non-integer and time-varying rates, device-resident lengths."""
from __future__ import annotations

import ctypes as C
import wave

import numpy as np

from . import _lib

OUT_SR = 16000
MAX_CHANNELS = _lib.RESAMPLE_MAX_CHANNELS


def resample_plan(in_sr, out_sr, n_before, n_new, finishing=False, zeros=32):
    """``(out_first, out_count)``: the outputs a push of ``n_new`` samples at ``in_sr`` decides on a series that holds ``n_before``
    (``ls_resample_plan``; no GPU).  ``in_sr == out_sr`` is a pass-through and emits every sample at once."""
    r = _lib.resample_ratio(in_sr, out_sr, zeros)
    return _lib.resample_ratio_plan(r["up"], r["down"], 0 if int(in_sr) == int(out_sr) else r["half"], n_before, n_new, finishing)


def resample_taps(in_sr, out_sr=OUT_SR, zeros=32, beta=12.0, rolloff=0.95):
    """``(h64, h32, ratio)``: the taps of a rate pair in double and as the kernels read them, with ``_lib.resample_ratio``'s dict."""
    r = _lib.resample_ratio(in_sr, out_sr, zeros)
    h64, h32 = _lib.resample_taps(r["up"], r["down"], zeros, beta, rolloff)
    return h64, h32, r


def _check_filter(in_sr, out_sr, zeros, beta, rolloff):
    r = _lib.resample_ratio(in_sr, out_sr, zeros)
    if not float(beta) >= 0 or not 0 < float(rolloff) <= 1:
        raise ValueError(f"beta must be >= 0 and rolloff in (0, 1], got {beta}, {rolloff}")
    return r


def _is_torch(a):
    return hasattr(a, "detach")


def _dtype_name(a):
    name = str(a.dtype).replace("torch.", "")
    if name not in _lib.RESAMPLE_DTYPES:
        raise ValueError(f"audio must be float32 or int16, got {name}")
    return name


def _check_audio(audio, rows, channels, who):
    """``(dtype name, frames per row, channels)`` of ``audio`` [rows, n] or [rows, n, C]; ``rows`` / ``channels`` None: any."""
    if not hasattr(audio, "shape") or not hasattr(audio, "dtype"):
        raise ValueError(f"{who}: audio must be a numpy array or a torch tensor, got {type(audio).__name__}")
    name = _dtype_name(audio)
    shape = tuple(int(v) for v in audio.shape)
    if len(shape) not in (2, 3) or (rows is not None and shape[0] != rows) or shape[0] < 1:
        raise ValueError(f"{who}: audio must be [{'B' if rows is None else rows}, n] or [.., n, C], got {list(shape)}")
    ch = shape[2] if len(shape) == 3 else 1
    if not 1 <= ch <= MAX_CHANNELS:
        raise ValueError(f"{who}: {ch} channels outside [1, {MAX_CHANNELS}]")
    if channels is not None and ch != channels:
        raise ValueError(f"{who}: audio has {ch} channels, the stream was opened for {channels}")
    return name, shape[1], ch


def _pointer(audio, device):
    """``(on_device, pointer, keep-alive)`` of a contiguous view of ``audio`` in its own dtype."""
    if _lib._is_cuda(audio):
        import torch
        t = audio.detach().to(torch.device("cuda", device)).contiguous()
        return True, C.c_void_p(t.data_ptr()), t
    n = np.ascontiguousarray(audio.detach().numpy() if _is_torch(audio) else audio)
    return False, n.ctypes.data_as(C.c_void_p), n


def _output(shape, like, device, on_device):
    """A zeroed float32 output on the side of the input: ``(object, pointer)``."""
    if on_device:
        import torch
        t = torch.zeros(shape, dtype=torch.float32, device=torch.device("cuda", device))
        return t, C.c_void_p(t.data_ptr())
    n = np.zeros(shape, np.float32)
    if like is not None and _is_torch(like):
        import torch
        return torch.from_numpy(n), n.ctypes.data_as(C.c_void_p)
    return n, n.ctypes.data_as(C.c_void_p)


def resample(audio, in_sr, out_sr=OUT_SR, lengths=None, zeros=32, beta=12.0, rolloff=0.95, device=0):
    """``audio`` [B, n] or interleaved [B, n, C] (numpy, CPU or CUDA tensor; float32 or int16; C <= 8) at ``in_sr`` Hz to mono float32 at
    ``out_sr``: ``(y [B, max(n_out)], n_out int64 [B])`` on the side the input is on.  ``lengths`` [B] (host): clip b's valid frames,
    default n; clip b gets ``n_out[b] = ceil(lengths[b] * out_sr / in_sr)`` outputs and 0 behind them, and nothing beyond its own
    frames is read, so a clip alone gives the bits it gives inside the batch.  int16 is scaled by 1 / 32768.  ``in_sr == out_sr``:
    the mixdown alone."""
    name, n, ch = _check_audio(audio, None, None, "resample")
    r = _check_filter(in_sr, out_sr, zeros, beta, rolloff)
    B = int(audio.shape[0])
    if n < 1:
        raise ValueError("resample: audio holds no frame")
    lens = np.full(B, n, np.int64) if lengths is None else _lib.host_lengths(lengths, B, 1, n, "lengths").astype(np.int64)
    half = 0 if int(in_sr) == int(out_sr) else r["half"]
    n_out = np.array([_lib.resample_ratio_plan(r["up"], r["down"], half, 0, int(v), True)[1] for v in lens], np.int64)
    cols = int(n_out.max())
    on_device, ptr, keep = _pointer(audio, device)
    out, out_ptr = _output((B, cols), audio, device, on_device)
    got = np.zeros(B, np.int64)
    a = _lib.LsResampleArgs()
    a.batch, a.on_device, a.dtype, a.channels = B, int(on_device), _lib.RESAMPLE_DTYPES[name], ch
    a.row_stride, a.audio, a.lengths = n * ch, ptr, lens.ctypes.data_as(_lib.c_i64p)
    a.in_sr, a.out_sr, a.zeros, a.beta, a.rolloff = int(in_sr), int(out_sr), int(zeros), float(beta), float(rolloff)
    a.out, a.out_stride, a.out_lengths = out_ptr, cols, got.ctypes.data_as(_lib.c_i64p)
    lib = _lib.load_library()
    if on_device:
        _lib._order_after_torch(int(device), None)       # the kernels run on the null stream: torch's work so far comes first
    rc = lib.ls_resample(int(device), C.byref(a))
    if rc != 0:
        msg = lib.ls_resample_stream_last_error(None).decode()
        raise (ValueError if rc == -1 else _lib.EngineError)(f"ls_resample failed ({rc}): {msg}")
    assert (got == n_out).all()
    del keep
    return out, n_out


class ResampleStream:
    """A running ``open_resample_stream``; see there.  ``samples_in``: the input frames of each slot's series, ``outputs_done`` the
    outputs emitted for it (host int64 [S])."""

    def __init__(self, capacity, in_sr, out_sr=OUT_SR, channels=1, dtype="float32", zeros=32, beta=12.0, rolloff=0.95, max_chunk=65536, device=0):
        S = int(capacity)
        if S < 1:
            raise ValueError(f"capacity must be >= 1, got {capacity}")
        if dtype is not None and dtype not in _lib.RESAMPLE_DTYPES:
            raise ValueError(f"dtype must be 'float32', 'int16' or None (that of the first push), got {dtype!r}")
        if isinstance(channels, bool) or int(channels) != channels or not 1 <= int(channels) <= MAX_CHANNELS:
            raise ValueError(f"channels must lie in [1, {MAX_CHANNELS}], got {channels!r}")
        if int(max_chunk) < 1:
            raise ValueError(f"max_chunk must be >= 1, got {max_chunk}")
        r = _check_filter(in_sr, out_sr, zeros, beta, rolloff)
        self.capacity, self.in_sr, self.out_sr, self.channels, self.dtype = S, int(in_sr), int(out_sr), int(channels), dtype
        self.max_chunk, self.device, self.ratio = int(max_chunk), int(device), r
        self._filter = (int(zeros), float(beta), float(rolloff))
        self._half = 0 if self.in_sr == self.out_sr else r["half"]
        self._samples = np.zeros(S, np.int64)
        self._outputs = np.zeros(S, np.int64)
        self._eng = None
        self._closed = False

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    @property
    def samples_in(self):
        return self._samples.copy()

    @property
    def outputs_done(self):
        return self._outputs.copy()

    def _engine(self):
        if self._eng is None:         # bound at the first call that needs it: every refusal comes before a device is touched
            self.dtype = self.dtype or "float32"
            self._eng = _lib.ResampleStreamEngine(self.capacity, self.in_sr, self.out_sr, self.channels, self.dtype, *self._filter, self.max_chunk,
                                                  self.device)
        return self._eng

    def plan(self, lengths, finish=None):
        """``(out_first, out_count)`` int64 [S] of a push of ``lengths`` frames with the flags ``finish``, from host counts alone."""
        S = self.capacity
        first, count = self._outputs.copy(), np.zeros(S, np.int64)
        for s in range(S):
            if lengths[s] or (finish is not None and finish[s]):
                first[s], count[s] = _lib.resample_ratio_plan(self.ratio["up"], self.ratio["down"], self._half, self._samples[s], lengths[s],
                                                        finish is not None and bool(finish[s]))
        return first, count

    def push(self, audio=None, lengths=None, finish=None, device_out=None):
        """``audio`` [S, n] or [S, n, C] (numpy, CPU or CUDA tensor of the stream's dtype; n <= max_chunk): slot s's new frames in
        ``audio[s, :lengths[s]]`` (``lengths=None``: n for every slot).  ``finish`` (bool [S]): the slots whose series ends with this
        push -- they emit what is pending and are empty afterwards.  Returns ``{'audio': [S, K] float32, 'out_first', 'out_count'}``:
        slot s's new outputs in ``audio[s, :out_count[s]]``, zero behind them, K = max(out_count); they continue the series at
        ``out_first[s]``.  The outputs are on the side of ``audio`` (``device_out`` overrides it; a call without audio: host).
        What the engine would refuse raises ``ValueError`` before anything runs, and the stream stays as it was."""
        name, n_max, lens, fin, first, count = self.check(audio, lengths, finish)
        S, self.dtype = self.capacity, self.dtype or name
        K = int(count.max())
        on_device = _lib._is_cuda(audio) if device_out is None else bool(device_out)
        out, out_ptr = _output((S, K), audio, self.device, on_device)
        return self._run(audio, n_max, lens, fin, first, count, on_device, out, out_ptr)

    def check(self, audio=None, lengths=None, finish=None):
        """Everything ``push`` refuses, and what it would emit, from host counts alone; the stream stays as it is.  Returns ``(dtype name
        or None, n_max, lengths int64 [S], finish int32 [S], out_first, out_count int64 [S])``."""
        if self._closed:
            raise RuntimeError("the resample stream is closed")
        S, name = self.capacity, None
        if audio is None:
            if lengths is not None and np.asarray(lengths).any():
                raise ValueError("lengths are the valid frames of audio: pass audio")
            n_max, lens = 0, np.zeros(S, np.int64)
        else:
            name, n_max, _ = _check_audio(audio, S, self.channels, "push")
            if name != (self.dtype or name):
                raise ValueError(f"push: the stream was opened for {self.dtype}, audio is {name}")
            if n_max > self.max_chunk:
                raise ValueError(f"a push takes at most max_chunk = {self.max_chunk} frames per slot, got {n_max}")
            lens = np.full(S, n_max, np.int64) if lengths is None else _lib.host_lengths(lengths, S, 0, n_max, "lengths").astype(np.int64)
        fin = np.zeros(S, np.int32)
        if finish is not None:
            fin = np.asarray(finish.detach().cpu().numpy() if _is_torch(finish) else finish).reshape(-1).astype(bool).astype(np.int32)
            if fin.shape != (S,):
                raise ValueError(f"finish must hold one flag per slot, got {fin.size} for {S} slots")
        for s in range(S):
            if fin[s] and self._samples[s] + lens[s] < 1:
                raise ValueError(f"finish on slot {s}, which holds no sample")
        first, count = self.plan(lens, fin)
        return name, n_max, lens, fin, first, count

    def _run(self, audio, n_max, lens, fin, first, count, on_device, out, out_ptr):
        S, K = self.capacity, int(count.max())
        if not lens.any() and not K:                      # nothing to compute: a finish at an output boundary still frees its slots
            if fin.any():
                self._samples[fin.astype(bool)] = 0
                self._outputs[fin.astype(bool)] = 0
                if self._eng is not None:
                    for s in np.nonzero(fin)[0]:
                        self._eng.reset(int(s))
            return {"audio": out, "out_first": first, "out_count": count}
        a = _lib.LsResampleStreamPushArgs()
        keep = None
        if audio is not None and lens.any():
            if _lib._is_cuda(audio) != on_device:         # device_out against the audio's side: the audio follows the outputs
                import torch
                audio = torch.as_tensor(audio).to(torch.device("cuda", self.device)) if on_device else audio.detach().cpu()
            _, a.audio, keep = _pointer(audio, self.device)
        lens32, got_first, got_count = lens.astype(np.int32), np.zeros(S, np.int64), np.zeros(S, np.int64)
        a.on_device, a.n_max, a.out_capacity = int(on_device), n_max, K
        a.lengths, a.finish = lens32.ctypes.data_as(_lib.c_i32p), fin.ctypes.data_as(_lib.c_i32p)
        a.out, a.out_first, a.out_count = out_ptr, got_first.ctypes.data_as(_lib.c_i64p), got_count.ctypes.data_as(_lib.c_i64p)
        eng = self._engine()
        if on_device:
            _lib._order_after_torch(self.device, None)
        eng.push(a)
        assert (got_count == count).all() and (got_first[count > 0] == first[count > 0]).all()
        self._samples += lens
        self._outputs = first + count
        self._samples[fin.astype(bool)] = 0
        self._outputs[fin.astype(bool)] = 0
        del keep
        return {"audio": out, "out_first": first, "out_count": count}

    def finish(self, slot, device_out=None):
        """End slot ``slot``'s series: the outputs ``[k]`` the end still owes (``ceil(samples_in * out_sr / in_sr)`` in all).  The slot is
        empty afterwards: its next frames start a new series."""
        slot = int(slot)
        if not 0 <= slot < self.capacity or self._samples[slot] < 1:
            raise ValueError(f"slot {slot} holds no sample")
        fin = np.zeros(self.capacity, bool)
        fin[slot] = True
        got = self.push(finish=fin, device_out=device_out)
        return got["audio"][slot, :int(got["out_count"][slot])]

    def reset(self, slot):
        """Drop slot ``slot``'s series without emitting what is pending (``ls_resample_stream_reset``): no samples in, no carry.  A slot
        that is already empty stays so."""
        slot = int(slot)
        if not 0 <= slot < self.capacity:
            raise ValueError(f"slot {slot} outside [0, {self.capacity})")
        if self._closed:
            raise RuntimeError("the resample stream is closed")
        self._samples[slot] = self._outputs[slot] = 0
        if self._eng is not None:
            self._eng.reset(slot)

    def info(self) -> dict:
        """``samples_in``, ``outputs_done`` [S] and ``device_bytes`` (``ls_resample_stream_info``); the bytes are constant after the open."""
        return self._engine().info()

    def close(self):
        self._closed = True
        if self._eng is not None:
            self._eng.close()
            self._eng = None


def open_resample_stream(capacity, in_sr, out_sr=OUT_SR, channels=1, dtype="float32", zeros=32, beta=12.0, rolloff=0.95, max_chunk=65536,
                         device=0) -> ResampleStream:
    """The streaming form of ``resample``: ``capacity`` slots, each a series of its own that is fed chunks of any size (up to
    ``max_chunk`` frames) of ``channels`` interleaved ``dtype`` samples (``None``: the dtype of the first push) at ``in_sr``.  Per slot, the outputs of all pushes and the finish,
    concatenated, are bit for bit ``resample`` on the whole series (tests/test_gpu_resample.py): the handle keeps the last
    ``ratio['carry_len']`` mono samples of every slot on the device, and an output's sum runs in the same order in both forms.  The
    engine's handle is opened lazily, by the first push that has work for the device (so every argument error comes before a device is
    touched); ``ls_resample_stream_open`` allocates everything for ``capacity`` and ``max_chunk`` there, and nothing grows afterwards."""
    return ResampleStream(capacity, in_sr, out_sr, channels, dtype, zeros, beta, rolloff, max_chunk, device)


def read_wav(path):
    """``(int16 [n, C], sr)`` of a 16-bit PCM WAV file (the stdlib ``wave`` module).  Any other sample width or an encoding ``wave`` does
    not read raises ``ValueError`` that names it."""
    try:
        with wave.open(str(path), "rb") as w:
            width, ch, sr, n = w.getsampwidth(), w.getnchannels(), w.getframerate(), w.getnframes()
            if width != 2 or w.getcomptype() != "NONE":
                raise ValueError(f"{path}: {8 * width}-bit samples ({w.getcomptype()}); only 16-bit PCM WAV is read")
            raw = w.readframes(n)
    except wave.Error as e:
        raise ValueError(f"{path}: not a PCM WAV file the wave module reads ({e}); only 16-bit PCM WAV is read") from e
    data = np.frombuffer(raw, dtype="<i2").astype(np.int16, copy=False)
    return data[:len(data) // ch * ch].reshape(-1, ch), int(sr)


def load(path, sr=OUT_SR, device=0):
    """A 16-bit PCM WAV file as mono float32 at ``sr`` Hz, numpy [n]: ``read_wav``, then ``resample`` on ``device``.  This has the SHAPE
    and SCALE of ``librosa.load(path, sr=sr)`` -- mono, float32 in [-1, 1), ``ceil(n * sr / file_sr)`` samples -- and NOT its bits: the
    filter here is this module's Kaiser-windowed sinc, not resampy's or soxr's."""
    data, file_sr = read_wav(path)
    if data.shape[0] < 1:
        raise ValueError(f"{path}: no frames")
    y, n_out = resample(data[None], file_sr, sr, device=device)
    return np.asarray(y)[0, :int(n_out[0])]
