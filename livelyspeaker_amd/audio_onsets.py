"""Audio onsets for the beat-alignment scores, on the gfx950 engine (``ls_onsets``): what the reference's evaluation loops take from
librosa 0.9.2 -- ``librosa.onset.onset_detect(y=audio, sr=16000, units='time')`` per TED clip (scripts/test_RAG_ted.py:113) and
``alignment.load_audio`` per BEAT clip (scripts_beat/utils/metric.py:60-74) -- as two HIP kernels over a whole batch: STFT (n_fft
2048, hop 512, periodic Hann, centred), 128 Slaney mel filters, dB, spectral flux, peak picking, backtracking.

``from utils.metric import alignment`` becomes ``from livelyspeaker_amd.audio_onsets import alignment``; ``audio_onsets`` is the
batched form, whose results stay on the device.

Two defaults depend on the librosa version and follow 0.9.2: ``pad_mode='constant'`` (zeros; ``'reflect'`` is the other value) and
``fmax=11025.0`` (0.9.x hard-codes it in ``onset_strength_multi``; pass ``fmax=sr / 2`` for what 0.10 and later compute).  The chain
is restated in float64 in tests/onsets_restatement.py; librosa itself was not available to compare with.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib, beat_metrics

N_FFT, HOP, N_MELS = 2048, 512, 128
MAX_FRAMES = 4096
SCORE_TILE = 256            # LS_SCORE_TILE: the frames per tile of the any-length pick (ls_onsets_long)
MAX_LENGTH_LONG = 2 ** 31 - N_FFT
PAD_MODES = {"constant": 0, "reflect": 1}
OUTPUTS = ("mel_db", "rms", "oenv", "count", "onset_raw", "onset_bt", "onset_bt_rms")


def onset_tables(sr=16000, n_fft=N_FFT, n_mels=N_MELS, fmin=0.0, fmax=11025.0):
    """``ls_onsets_tables``: the float32 tables the kernels compute with -- window [n_fft], twiddle [n_fft, 2] and the Slaney mel
    filterbank in CSR form (mel_ptr, mel_col, mel_w) -- built on the host; no GPU is needed."""
    lib = _lib.load_library()
    nnz = C.c_int32()
    if lib.ls_onsets_tables(sr, n_fft, n_mels, fmin, fmax, None, None, None, None, None, 0, C.byref(nnz)) != 0:
        raise _lib.EngineError("ls_onsets_tables refused its arguments")
    window, twiddle = np.empty(n_fft, np.float32), np.empty((n_fft, 2), np.float32)
    ptr, col, w = np.empty(n_mels + 1, np.int32), np.empty(nnz.value, np.int32), np.empty(nnz.value, np.float32)
    rc = lib.ls_onsets_tables(sr, n_fft, n_mels, fmin, fmax, window.ctypes.data, twiddle.ctypes.data, ptr.ctypes.data,
                              col.ctypes.data, w.ctypes.data, nnz.value, C.byref(nnz))
    if rc != 0:
        raise _lib.EngineError(f"ls_onsets_tables failed ({rc})")
    return {"window": window, "twiddle": twiddle, "mel_ptr": ptr, "mel_col": col, "mel_w": w}


def mel_filterbank(sr=16000, n_fft=N_FFT, n_mels=N_MELS, fmin=0.0, fmax=11025.0):
    """The CSR table of ``onset_tables`` as the dense [n_mels, 1 + n_fft // 2] array of ``librosa.filters.mel``."""
    t = onset_tables(sr, n_fft, n_mels, fmin, fmax)
    W = np.zeros((n_mels, 1 + n_fft // 2), np.float32)
    for i in range(n_mels):
        s = slice(t["mel_ptr"][i], t["mel_ptr"][i + 1])
        W[i, t["mel_col"][s]] = t["mel_w"][s]
    return W


def audio_onsets(audio=None, sr=16000, sr_pick=None, *, onset_envelope=None, pad_mode="constant", fmax=11025.0, delta=0.07,
                 device=0, want=("oenv", "count", "onset_raw", "onset_bt", "onset_bt_rms"), timing=None, lengths=None):
    """``ls_onsets`` on a batch of clips: audio [B, L] (numpy, or a CUDA tensor: then the outputs stay on the device), or
    ``onset_envelope`` [B, F] for the pick alone.  ``sr_pick`` is the rate onset_detect's picking windows are sized by: ``sr`` when
    the caller passes it to onset_detect (TED), 22050 when it does not (BEAT's load_audio).  Returns a dict of the outputs named in
    ``want``: mel_db [B, F, 128], rms [B, F], oenv [B, F], count [B] and the int32 slabs onset_raw, onset_bt, onset_bt_rms [B, F] of
    which the first count[b] entries of row b are valid; with ``count`` wanted, ``counts`` is its host copy (the one host wait).
    ``timing``: a list that receives the two kernel times in ms.

    ``lengths`` (a host sequence [B]): clips of different lengths in one call (``ls_onsets_ragged``).  Clip b holds ``lengths[b]`` valid
    samples (frames, with ``onset_envelope``) of its row; what follows them is never read.  The outputs keep their [B, F] shapes; on
    clip b's own ``1 + lengths[b] // 512`` frames they are bit for bit those of the clip alone at its own length, beyond them 0 (floats)
    and -1 (the slabs).  ``None`` is the equal-length call."""
    return _onsets(MAX_FRAMES, audio, sr, sr_pick, onset_envelope, pad_mode, fmax, delta, device, want, timing, lengths)


def audio_onsets_long(audio=None, sr=16000, sr_pick=None, *, onset_envelope=None, pad_mode="constant", fmax=11025.0, delta=0.07,
                      device=0, want=("oenv", "count", "onset_raw", "onset_bt", "onset_bt_rms"), timing=None):
    """``audio_onsets`` for an equal-length batch of clips of ANY length (``ls_onsets_long``): the same arguments and the same dict,
    without the limit of ``MAX_FRAMES`` frames (131 s of audio) -- a quarter of an hour of speech is 28 126 frames.  The spectrum is
    the same kernel; the pick runs tiled over ``SCORE_TILE`` frames with nothing on chip sized by the clip, and every float is a
    per-frame expression or an exact reduction, so up to ``MAX_FRAMES`` frames every output equals ``audio_onsets``' bit for bit.
    ``timing`` receives the spectrum's time and that of all launches of the pick.  Not built: ``lengths=`` (the ragged form)."""
    return _onsets(None, audio, sr, sr_pick, onset_envelope, pad_mode, fmax, delta, device, want, timing, None)


def _onsets(max_frames, audio, sr, sr_pick, onset_envelope, pad_mode, fmax, delta, device, want, timing, lengths):
    """Both entries: ``max_frames`` None is the any-length one."""
    if (audio is None) == (onset_envelope is None):
        raise ValueError("pass either audio or onset_envelope")
    if pad_mode not in PAD_MODES:
        raise ValueError(f"pad_mode must be 'constant' or 'reflect', got {pad_mode!r}")
    unknown = set(want) - set(OUTPUTS)
    if unknown:
        raise ValueError(f"unknown outputs {sorted(unknown)}")
    given = audio is None
    src = onset_envelope if given else audio
    if len(src.shape) != 2:
        raise ValueError(f"expected [B, {'F' if given else 'L'}], got {list(src.shape)}")
    B, L = int(src.shape[0]), int(src.shape[1])
    F = L if given else 1 + L // HOP
    if given and {"mel_db", "rms", "onset_bt_rms"} & set(want):
        want = tuple(w for w in want if w not in ("mel_db", "rms", "onset_bt_rms"))
    if B < 1 or L < 1 or (max_frames is not None and F > max_frames):
        raise ValueError(f"need at least one clip and one sample, and at most {MAX_FRAMES} frames: got B={B}, length {L}")
    if max_frames is None and (L > MAX_LENGTH_LONG or -(-B * F // 4) > 2 ** 31 - 1):
        raise ValueError(f"at most {MAX_LENGTH_LONG} samples per clip and 2^33 - 4 frames per call: got B={B}, length {L}")
    if not given and pad_mode == "reflect" and L <= N_FFT // 2:
        raise ValueError(f"reflect padding needs more than {N_FFT // 2} samples, got {L}")
    lens = None
    if lengths is not None:
        lens = _lib.host_lengths(lengths, B, 1, L, "lengths")
        if not given and pad_mode == "reflect" and int(lens.min()) <= N_FFT // 2:
            raise ValueError(f"reflect padding needs more than {N_FFT // 2} samples in every clip, got {int(lens.min())}")
    m = _lib._Marshal(device, src)
    a = _lib.LsOnsetsArgs()
    a.batch, a.length, a.on_device, a.pad_mode = B, L, int(m.on_device), PAD_MODES[pad_mode]
    a.sr, a.sr_pick, a.fmax, a.delta = float(sr), float(sr if sr_pick is None else sr_pick), float(fmax), float(delta)
    if given:
        a.envelope = m.f32(src, (B, L))
    else:
        a.audio = m.f32(src, (B, L))
    out = {}
    shapes = {"mel_db": (B, F, N_MELS), "rms": (B, F), "oenv": (B, F)}
    for name in OUTPUTS:
        if name in want:
            out[name], ptr = m.out(shapes[name]) if name in shapes else m.out((B,) if name == "count" else (B, F), np.int32)
            setattr(a, name, ptr)
    ms = (C.c_float * 2)()
    if timing is not None:
        a.kernel_ms = C.cast(ms, C.c_void_p)
    m.ready()
    if lens is None:
        _lib.call("ls_onsets" if max_frames is not None else "ls_onsets_long", device, C.byref(a))
    else:
        _lib.call("ls_onsets_ragged", device, C.byref(a), lens.ctypes.data_as(C.c_void_p))
    if timing is not None:
        timing[:] = [float(ms[0]), float(ms[1])]
    if "count" in out:
        c = out["count"]
        out["counts"] = c.cpu().numpy() if m.on_device else c
    return out


def _host(a):
    return a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)


def _rows(slab, counts):
    slab = _host(slab)
    return [slab[b, :int(n)].astype(np.int64) for b, n in enumerate(counts)]


def onset_strength(y, sr=22050, pad_mode="constant", fmax=11025.0, device=0):
    """``librosa.onset.onset_strength(y=y, sr=sr)`` of one clip [L], or of a batch [B, L]."""
    y2 = y[None] if len(y.shape) == 1 else y
    o = audio_onsets(y2, sr, pad_mode=pad_mode, fmax=fmax, device=device, want=("oenv",))["oenv"]
    return o[0] if len(y.shape) == 1 else o


def rms(y, pad_mode="constant", device=0):
    """``librosa.feature.rms(S=np.abs(librosa.stft(y)))`` of one clip: [1, F]."""
    return audio_onsets(y[None], pad_mode=pad_mode, device=device, want=("rms",))["rms"]


def onset_detect(y=None, sr=22050, onset_envelope=None, units="frames", backtrack=False, pad_mode="constant", fmax=11025.0,
                 delta=0.07, device=0):
    """``librosa.onset.onset_detect`` of one clip with the reference's arguments; ``onset_envelope`` takes precedence over ``y``, as
    in librosa.  Returns a host array of frames, or of seconds (frame * 512 / sr) for ``units='time'``."""
    if backtrack:
        raise NotImplementedError("backtrack=True is not built: call onset_backtrack on the result, as the reference does")
    if units not in ("frames", "time"):
        raise ValueError(f"units must be 'frames' or 'time', got {units!r}")
    if onset_envelope is not None:
        got = audio_onsets(onset_envelope=onset_envelope[None], sr=sr, delta=delta, device=device, want=("count", "onset_raw"))
    elif y is not None:
        got = audio_onsets(y[None], sr, pad_mode=pad_mode, fmax=fmax, delta=delta, device=device, want=("count", "onset_raw"))
    else:
        raise ValueError("y or onset_envelope must be provided")
    frames = _rows(got["onset_raw"], got["counts"])[0]
    return frames if units == "frames" else frames * HOP / float(sr)


def onset_backtrack(events, energy):
    """``librosa.onset.onset_backtrack``: every event to the nearest minimum of ``energy`` at or before it (duplicates kept).  A
    handful of host integers; the batched path does it in ``ls_onsets``.  An empty ``events`` returns an empty array, where librosa
    raises."""
    events = np.asarray(_host(events), np.int64).reshape(-1)
    if events.size == 0:
        return events
    e = np.asarray(_host(energy)).reshape(-1)
    m = np.flatnonzero((e[1:-1] <= e[:-2]) & (e[1:-1] < e[2:]))
    m = np.unique(np.concatenate([[0], 1 + m])).astype(np.int64)
    return m[np.searchsorted(m, events, side="right") - 1]


def onset_times(audio, sr=16000, sr_pick=None, which="onset_raw", time_sr=None, lengths=None, **kw):
    """One array of onset times in seconds per clip of ``audio`` [B, L]: ``which`` frames * 512 / ``time_sr`` (default ``sr``).
    ``lengths`` [B]: the clips' valid samples (``audio_onsets``); every clip gets its own onsets."""
    got = audio_onsets(audio, sr, sr_pick, want=("count", which), lengths=lengths, **kw)
    return [r * HOP / float(time_sr or sr) for r in _rows(got[which], got["counts"])]


class alignment(beat_metrics.alignment):
    """scripts_beat/utils/metric.py:53-193 with the audio side on the device: ``load_audio`` returns the reference's three FRAME
    arrays and ``calculate_align`` takes frames, as the reference's does."""

    def __init__(self, sigma, order, device=0, pad_mode="constant", fmax=11025.0):
        super().__init__(sigma, order, device)
        self.pad_mode, self.fmax = pad_mode, fmax

    def load_audio(self, wave, t_start, t_end, without_file=False, sr_audio=16000):
        if not without_file:
            raise NotImplementedError("reading audio files (librosa.load) is not built: pass the samples with without_file=True")
        short_y = wave[t_start * sr_audio:t_end * sr_audio]
        # onset_detect(onset_envelope=...) without sr: the picking windows are those of librosa's default rate
        got = audio_onsets(short_y[None], sr_audio, 22050, pad_mode=self.pad_mode, fmax=self.fmax, device=self.device,
                           want=("rms", "oenv", "count", "onset_raw", "onset_bt", "onset_bt_rms"))
        self.oenv, self.rms = _host(got["oenv"])[0], _host(got["rms"])
        self.times = beat_metrics.frames_to_time(np.arange(self.oenv.shape[0]))
        return tuple(_rows(got[k], got["counts"])[0] for k in ("onset_raw", "onset_bt", "onset_bt_rms"))

    def calculate_align(self, onset_raw, onset_bt, onset_bt_rms, beat_right_arm, beat_right_shoulder, beat_right_wrist, beat_left_arm,
                        beat_left_shoulder, beat_left_wrist, pose_fps=15):
        """``onset_bt_rms`` in frames; the reference converts them with librosa.frames_to_time's defaults (22050 Hz for 16 kHz
        audio), which is part of its score."""
        return super().calculate_align(onset_raw, onset_bt, beat_metrics.frames_to_time(onset_bt_rms), beat_right_arm,
                                       beat_right_shoulder, beat_right_wrist, beat_left_arm, beat_left_shoulder, beat_left_wrist,
                                       pose_fps)
