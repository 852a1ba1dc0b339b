"""The resampler restated in numpy float64 from its definition (include/ls_hip.h, "Audio front end"); it never calls the library.  The
taps are an argument, so a test can feed it the library's own float32 taps or ones designed here.

    g = gcd(in_sr, out_sr), up = out_sr / g, down = in_sr / g, q = max(up, down), half = zeros * q
    h[i] = up * (rolloff / q) * sinc(rolloff * (i - half) / q) * kaiser(2 half + 1, beta)[i]
    y[m] = sum_k h[m down - k up + half] x[k],  k in [ceil((m down - half) / up), floor((m down + half) / up)] cut to [0, n),
    m in [0, ceil(n up / down))
"""
from math import gcd

import numpy as np


def ratio(in_sr, out_sr, zeros):
    g = gcd(int(in_sr), int(out_sr))
    up, down = int(out_sr) // g, int(in_sr) // g
    return up, down, int(zeros) * max(up, down)


def design(up, down, zeros, beta=12.0, rolloff=0.95):
    q = max(up, down)
    half = zeros * q
    i = np.arange(2 * half + 1, dtype=np.float64)
    return up * (rolloff / q) * np.sinc(rolloff * (i - half) / q) * np.kaiser(2 * half + 1, beta)


def decided(n, up, down, half, finishing=False):
    """D(n): the outputs decided by n samples of a running series, or of one that ends there."""
    if finishing:
        return -((-n * up) // down)
    return max(0, (n * up - 1 - half) // down + 1)


def mixdown(x):
    """float32 mono [.., n] of [.., n] or interleaved [.., n, C], float32 or int16, exactly as specified: float32 -- the sum in channel
    order in float32, times float32(1 / C); int16 -- the int32 sum converted (exact), times float32(1 / (32768 C))."""
    x = np.asarray(x)
    if x.ndim == 2:
        x = x[..., None]
    C = x.shape[-1]
    if x.dtype == np.int16:
        s = x.astype(np.int32).sum(axis=-1).astype(np.float32)
        return s * np.float32(1.0 / (32768.0 * C))
    assert x.dtype == np.float32
    s = x[..., 0].copy()
    for c in range(1, C):
        s = (s + x[..., c]).astype(np.float32)
    return (s * np.float32(1.0 / C)).astype(np.float32)


def resample(x, up, down, half, h):
    """``(y, mag)`` float64 [ceil(n up / down)] of the mono series ``x`` [n]: the outputs, and sum_k |h_k| |x_k| over the same terms."""
    x = np.asarray(x, np.float64)
    h = np.asarray(h, np.float64)
    assert x.ndim == 1 and h.shape == (2 * half + 1,)
    n = x.shape[0]
    n_out = decided(n, up, down, half, True)
    y, mag = np.zeros(n_out), np.zeros(n_out)
    for m in range(n_out):
        lo = max(0, -((half - m * down) // up))          # ceil((m down - half) / up)
        hi = min(n - 1, (m * down + half) // up)
        if hi < lo:
            continue
        k = np.arange(lo, hi + 1)
        taps = h[m * down - k * up + half]
        y[m] = np.dot(taps, x[k])
        mag[m] = np.dot(np.abs(taps), np.abs(x[k]))
    return y, mag


def resample_sr(x, in_sr, out_sr, zeros, h=None):
    """``(y, mag)`` of the mono series ``x`` between two rates: ``in_sr == out_sr`` is a pass-through (no filter), every other pair
    ``resample`` with the taps ``h`` (designed here at the defaults when left out)."""
    if int(in_sr) == int(out_sr):
        y = np.asarray(x, np.float64).copy()
        return y, np.abs(y)
    up, down, half = ratio(in_sr, out_sr, zeros)
    return resample(x, up, down, half, design(up, down, zeros) if h is None else h)
