"""numpy model of the split-fp32 channel mixing (k_step PREC 2, ls_step_common.h split3_bf16): x = hi + mid + lo with
round-to-nearest-even bf16 parts is exact, and the 6 partial products kept by the kernel stay within an fp32-class error
bound against float64.  No GPU."""
import numpy as np


def bf16_rne(x):
    """float32 -> nearest-even bf16, returned as float32 (what v_cvt_pk_bf16_f32 and the host image builder do)."""
    u = np.asarray(x, np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) >> 16
    return (u.astype(np.uint32) << 16).view(np.float32)


def split3(x):
    x = np.asarray(x, np.float32)
    hi = bf16_rne(x)
    r = (x - hi).astype(np.float32)
    mid = bf16_rne(r)
    lo = bf16_rne((r - mid).astype(np.float32))
    return hi, mid, lo


def _values(n=200_000, seed=5):
    g = np.random.Generator(np.random.PCG64(seed))
    parts = [g.standard_normal(n), -g.standard_normal(n) * 1e3, g.uniform(-1, 1, n) * 1e-30, g.uniform(-1, 1, n) * 1e30,
             np.ldexp(g.uniform(1, 2, n), g.integers(-100, 100, n)) * np.where(g.random(n) < 0.5, -1, 1)]
    v = np.concatenate(parts).astype(np.float32)
    # every bf16 rounding boundary case: mantissas whose low 16 bits are 0x8000 (ties), 0x7FFF, 0x8001
    m = g.integers(0, 1 << 7, n, dtype=np.uint32) << 16
    for low in (0x8000, 0x7FFF, 0x8001, 0xFFFF):
        bits = (np.uint32(127 << 23) | m | np.uint32(low)).astype(np.uint32)
        v = np.concatenate([v, bits.view(np.float32), -bits.view(np.float32)])
    return v


def test_three_part_split_is_exact():
    """Random, tiny, huge and negative values and every rounding boundary of the first split."""
    x = _values()
    hi, mid, lo = split3(x)
    for p in (hi, mid, lo):                                     # every part is a bf16 value
        assert np.array_equal(bf16_rne(p), p)
    s = (hi.astype(np.float64) + mid.astype(np.float64)) + lo.astype(np.float64)
    # exact while the lo part stays a normal number (|x| >= 2^-110); below that lo loses bits to the subnormal range, and the
    # remainder is under 2^-133 in absolute terms
    big = np.abs(x) >= 2.0 ** -110
    assert big.sum() > 0.9 * x.size
    assert np.array_equal(s[big], x[big].astype(np.float64))
    assert np.all(np.abs(s[~big] - x[~big].astype(np.float64)) <= 2.0 ** -133)
    nz = big
    assert np.all(np.abs(mid[nz]) <= np.abs(x[nz]) * 2.0 ** -8)
    assert np.all(np.abs(lo[nz]) <= np.abs(x[nz]) * 2.0 ** -16)


def _dot_split(w, u, terms):
    """K-long dot products from the bf16 parts: each bf16 x bf16 product exact, the kept terms summed smallest first in float64
    (the model of the products; the MFMA's own fp32 accumulation is measured on the GPU, tests/test_gpu_split_fp32.py)."""
    W, U = split3(w), split3(u)
    order = {6: [(2, 0), (1, 1), (0, 2), (1, 0), (0, 1), (0, 0)],
             9: [(2, 2), (2, 1), (1, 2), (2, 0), (1, 1), (0, 2), (1, 0), (0, 1), (0, 0)]}[terms]
    acc = np.zeros(w.shape[0])
    for i, j in order:
        acc = acc + (W[i].astype(np.float64) * U[j].astype(np.float64)).sum(-1)
    return acc


def test_six_term_products_within_fp32_class_bound():
    """Channel mixing at K = 512 with LayerNorm-like operands and weight-like values.  The dropped terms (i + j >= 3) cost at most
    2 * 2^-24 + 2^-32 of |w||u| per product in the worst case (|a1| <= 2^-8 |a|, |a2| <= 2^-16 |a|); on these values, where the
    two bounds are rarely tight together and the signs are random, the error stays below 3 * 2^-25 of sum |w||u|."""
    g = np.random.Generator(np.random.PCG64(11))
    w = (g.standard_normal((256, 512)) * 0.04).astype(np.float32)
    u = g.standard_normal((256, 512)).astype(np.float32)
    exact = (w.astype(np.float64) * u.astype(np.float64)).sum(-1)
    mag = (np.abs(w.astype(np.float64)) * np.abs(u.astype(np.float64))).sum(-1)
    e6 = np.abs(_dot_split(w, u, 6) - exact)
    e9 = np.abs(_dot_split(w, u, 9) - exact)
    assert np.all(e9 <= mag * 1e-15)                             # all nine terms: the products are exact
    assert np.all(e6 <= mag * (2 * 2.0 ** -24 + 2.0 ** -32))    # the worst-case bound
    assert np.all(e6 <= mag * 3 * 2.0 ** -25)                     # what these values reach
    assert np.max(e6 / mag) < 2.0 ** -24
