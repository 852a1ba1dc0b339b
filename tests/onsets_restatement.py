"""Float64 restatement of the audio-onset chain the reference's scripts take from librosa 0.9.2 (``onset_detect(y=..., sr=16000,
units='time')`` on TED, ``alignment.load_audio`` of scripts_beat/utils/metric.py:60-74 on BEAT): STFT, Slaney mel, dB, spectral flux,
peak picking, backtracking.  numpy and scipy only, one function per step, in the order librosa takes them.  librosa itself was not
available where this was written: two version-dependent defaults (``pad_mode``, ``fmax``) are parameters, and
tests/test_onsets_host.py compares this module with librosa wherever the package is installed.

``dtype=np.float32`` computes as a float32 host chain would: float32 signal and window, complex64 FFT, float32 mel and dB; it is
the yardstick the GPU test takes its error bar from."""
import numpy as np
import scipy.fft
import scipy.ndimage
import scipy.signal

N_FFT, HOP, N_MELS = 2048, 512, 128
FMAX_092 = 11025.0          # hard-coded by 0.9.x's onset_strength_multi; sr / 2 from 0.10 on
DELTA = 0.07
LAG_SHIFT = 1 + N_FFT // (2 * HOP)      # lag 1 + the centring correction: 3 frames
THRESHOLD_MARGIN = 1e-4     # |x[n] - (mean + delta)| below this: the frame is decided inside float32 rounding
MINIMA_MARGIN = 1e-4        # neighbouring energies closer than this (relative): the pair's order is decided inside rounding


# ---- mel scale and filterbank (librosa.filters.mel, htk=False, norm='slaney') ----------------------------------------------------
def hz_to_mel(f):
    f = np.asanyarray(f, np.float64)
    f_sp, min_log_hz = 200.0 / 3, 1000.0
    min_log_mel, logstep = min_log_hz / f_sp, np.log(6.4) / 27.0
    mels = f / f_sp
    if f.ndim:
        log_t = f >= min_log_hz
        mels[log_t] = min_log_mel + np.log(f[log_t] / min_log_hz) / logstep
    elif f >= min_log_hz:
        mels = min_log_mel + np.log(f / min_log_hz) / logstep
    return mels


def mel_to_hz(m):
    m = np.asanyarray(m, np.float64)
    f_sp, min_log_hz = 200.0 / 3, 1000.0
    min_log_mel, logstep = min_log_hz / f_sp, np.log(6.4) / 27.0
    freqs = f_sp * m
    if m.ndim:
        log_t = m >= min_log_mel
        freqs[log_t] = min_log_hz * np.exp(logstep * (m[log_t] - min_log_mel))
    elif m >= min_log_mel:
        freqs = min_log_hz * np.exp(logstep * (m - min_log_mel))
    return freqs


def mel_frequencies(n_mels=128, fmin=0.0, fmax=11025.0):
    return mel_to_hz(np.linspace(hz_to_mel(fmin), hz_to_mel(fmax), n_mels))


def mel_filterbank(sr, n_fft=N_FFT, n_mels=N_MELS, fmin=0.0, fmax=FMAX_092):
    """[n_mels, 1 + n_fft // 2] float32, as librosa stores it: the triangles are written into a float32 array, which is then
    scaled in place by the float64 Slaney norms."""
    weights = np.zeros((n_mels, 1 + n_fft // 2), np.float32)
    fftfreqs = np.linspace(0, float(sr) / 2, 1 + n_fft // 2)
    mel_f = mel_frequencies(n_mels + 2, fmin, fmax)
    fdiff = np.diff(mel_f)
    ramps = np.subtract.outer(mel_f, fftfreqs)
    for i in range(n_mels):
        lower = -ramps[i] / fdiff[i]
        upper = ramps[i + 2] / fdiff[i + 1]
        weights[i] = np.maximum(0, np.minimum(lower, upper))
    enorm = 2.0 / (mel_f[2:n_mels + 2] - mel_f[:n_mels])
    weights *= enorm[:, np.newaxis]
    return weights


def hann_window(n_fft=N_FFT):
    return scipy.signal.get_window("hann", n_fft, fftbins=True)


# ---- spectrum ----------------------------------------------------------------------------------------------------------------------
def n_frames(length):
    return 1 + int(length) // HOP


def frames(y, pad_mode="constant"):
    """[F, 2048]: y padded by 1024 on both sides (zeros, or numpy's 'reflect'), cut every 512 samples."""
    y = np.asarray(y)
    if pad_mode == "reflect" and y.shape[-1] <= N_FFT // 2:
        raise ValueError("reflect padding needs more than 1024 samples")
    yp = np.pad(y, N_FFT // 2, mode=pad_mode)
    F = n_frames(y.shape[-1])
    return np.stack([yp[t * HOP: t * HOP + N_FFT] for t in range(F)])


def power_spectrum(y, pad_mode="constant", dtype=np.float64):
    """P[k, t] = |rfft(frame_t * window)[k]|^2, [1025, F]."""
    y = np.asarray(y, dtype)
    fr = frames(y, pad_mode) * hann_window().astype(dtype)
    Z = scipy.fft.rfft(fr.astype(dtype), axis=1)          # complex64 for a float32 input
    P = Z.real ** 2 + Z.imag ** 2
    return np.ascontiguousarray(P.T)


def mel_db(P, sr, fmax=FMAX_092):
    """S = 10 log10(max(1e-10, W @ P)), before the clip-wide clamp."""
    W = mel_filterbank(sr, fmax=fmax).astype(P.dtype)
    M = W @ P
    return (10.0 * np.log10(np.maximum(P.dtype.type(1e-10), M))).astype(P.dtype)


def onset_strength_from_db(S):
    S = np.maximum(S, S.max() - S.dtype.type(80.0))
    d = np.maximum(S.dtype.type(0.0), S[:, 1:] - S[:, :-1]).mean(axis=0, dtype=S.dtype)
    F = S.shape[1]
    return np.concatenate([np.zeros(LAG_SHIFT, S.dtype), d])[:F]


def onset_strength(y, sr, pad_mode="constant", fmax=FMAX_092, dtype=np.float64):
    return onset_strength_from_db(mel_db(power_spectrum(y, pad_mode, dtype), sr, fmax))


def rms(y, pad_mode="constant", dtype=np.float64):
    """librosa.feature.rms(S=|stft(y)|): rows 0 and 1024 halved, sqrt(2 sum / 2048^2)."""
    x = power_spectrum(y, pad_mode, dtype).copy()
    x[0] *= 0.5
    x[-1] *= 0.5
    return np.sqrt(2 * x.sum(axis=0) / N_FFT ** 2)


# ---- peak picking ------------------------------------------------------------------------------------------------------------------
def pick_parameters(sr_pick, hop=HOP):
    """(pre_max, post_max, pre_avg, post_avg, wait) of onset_detect's defaults, in frames."""
    pre_max = int(0.03 * sr_pick // hop)
    pre_avg = int(0.10 * sr_pick // hop)
    return pre_max, int(0.00 * sr_pick // hop) + 1, pre_avg, pre_avg + 1, pre_max


def normalise(oenv):
    x = np.asarray(oenv) - np.min(oenv)
    return x / (x.max() + np.finfo(x.dtype).tiny)


def moving_max_and_mean(x, pre_max, post_max, pre_avg, post_avg):
    """util.peak_pick of 0.9.2: the scipy filters with its origins, then its two edge loops, which truncate the averaging window."""
    max_length = pre_max + post_max
    max_origin = int(np.ceil(0.5 * (pre_max - post_max)))
    mov_max = scipy.ndimage.maximum_filter1d(x, int(max_length), mode="constant", origin=max_origin, cval=x.min())
    avg_length = pre_avg + post_avg
    avg_origin = int(np.ceil(0.5 * (pre_avg - post_avg)))
    mov_avg = scipy.ndimage.uniform_filter1d(x, int(avg_length), mode="nearest", origin=avg_origin)
    n = 0
    while n - pre_avg < 0 and n < x.shape[0]:
        start = max(n - pre_avg, 0)
        mov_avg[n] = np.mean(x[start: n + post_avg])
        n += 1
    n = max(x.shape[0] - post_avg, 0)
    while n < x.shape[0]:
        start = max(n - pre_avg, 0)
        mov_avg[n] = np.mean(x[start: n + post_avg])
        n += 1
    return mov_max, mov_avg


def peak_pick(x, pre_max, post_max, pre_avg, post_avg, delta, wait):
    mov_max, mov_avg = moving_max_and_mean(x, pre_max, post_max, pre_avg, post_avg)
    detections = x * (x == mov_max)
    detections = detections * (detections >= (mov_avg + delta))
    peaks, last = [], -np.inf
    for i in np.nonzero(detections)[0]:
        if i > last + wait:
            peaks.append(i)
            last = i
    return np.array(peaks, dtype=np.int64)


def onset_detect_envelope(oenv, sr_pick=22050, delta=DELTA):
    """onset_detect(onset_envelope=oenv, sr=sr_pick, backtrack=False), in frames."""
    oenv = np.asarray(oenv)
    if not oenv.any():
        return np.array([], dtype=np.int64)
    return peak_pick(normalise(oenv), *pick_parameters(sr_pick)[:4], delta, pick_parameters(sr_pick)[4])


def threshold_margins(oenv, sr_pick=22050, delta=DELTA):
    """|x[n] - (moving mean + delta)| per frame, for the set-aside rule of the GPU test."""
    x = normalise(np.asarray(oenv, np.float64))
    _, mov_avg = moving_max_and_mean(x, *pick_parameters(sr_pick)[:4])
    return np.abs(x - (mov_avg + delta))


# ---- backtracking ------------------------------------------------------------------------------------------------------------------
def minima(energy):
    e = np.asarray(energy)
    m = np.flatnonzero((e[1:-1] <= e[:-2]) & (e[1:-1] < e[2:]))
    return np.unique(np.concatenate([[0], 1 + m])).astype(np.int64)


def onset_backtrack(events, energy):
    """Every event to the nearest minimum of ``energy`` at or before it (duplicates kept); no event gives an empty array, where
    librosa raises."""
    events = np.asarray(events, np.int64)
    if events.size == 0:
        return events
    m = minima(energy)
    return m[np.searchsorted(m, events, side="right") - 1]


def close_pairs(energy, margin=MINIMA_MARGIN):
    """close[i]: energy[i] and energy[i + 1] differ by less than ``margin`` relative, so their order may flip in float32."""
    e = np.asarray(energy, np.float64)
    return np.abs(e[1:] - e[:-1]) < margin * np.maximum(np.abs(e[1:]), np.abs(e[:-1]))


# ---- the two callers -----------------------------------------------------------------------------------------------------------------
def ted_onset_times(y, sr=16000, pad_mode="constant", fmax=FMAX_092, dtype=np.float64):
    """librosa.onset.onset_detect(y=y, sr=16000, units='time') (scripts/test_RAG_ted.py:113)."""
    fr = onset_detect_envelope(onset_strength(y, sr, pad_mode, fmax, dtype), sr_pick=sr)
    return fr * HOP / float(sr)


def load_audio(y, t_start, t_end, sr_audio=16000, pad_mode="constant", fmax=FMAX_092, dtype=np.float64):
    """alignment.load_audio(..., without_file=True) (scripts_beat/utils/metric.py:60-74): the three frame arrays."""
    short = np.asarray(y)[t_start * sr_audio: t_end * sr_audio]
    oenv = onset_strength(short, sr_audio, pad_mode, fmax, dtype)
    raw = onset_detect_envelope(oenv)              # no sr given: the picking windows are those of 22050 Hz
    return raw, onset_backtrack(raw, oenv), onset_backtrack(raw, rms(short, pad_mode, dtype))


# ---- the seeded test clips -----------------------------------------------------------------------------------------------------------
def test_clip(seed, length, sr=16000):
    """Gaussian noise of sigma 0.01 plus 3-8 decaying tone bursts (150-3000 Hz, amplitude 0.2-1), float32."""
    rng = np.random.default_rng(seed)
    y = rng.normal(0.0, 0.01, length)
    t = np.arange(length) / sr
    for _ in range(int(rng.integers(3, 9))):
        t0 = rng.uniform(0.0, max(length / sr - 0.05, 0.01))
        f, a, tau = rng.uniform(150, 3000), rng.uniform(0.2, 1.0), rng.uniform(0.02, 0.12)
        on = t >= t0
        y[on] += a * np.exp(-(t[on] - t0) / tau) * np.sin(2 * np.pi * f * (t[on] - t0))
    return y.astype(np.float32)


test_clip.__test__ = False
