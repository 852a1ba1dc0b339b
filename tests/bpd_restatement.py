"""CPU restatement of calc_bpd_loop (scripts/diffusion/gaussian_diffusion.py:1591-1646) with _vb_terms_bpd (:1213-1246), _prior_bpd
(:1573-1589) and the likelihood helpers of scripts/diffusion/losses.py on the numpy oracle, plus the inputs the fixtures G20 / G20k
(tests/golden/make_golden_bpd.py) and their tests share.  Not a test module.

Arithmetic as the reference writes it: tables cast fp64 -> fp32 per column (Schedule.f32 = _extract_into_tensor), every intermediate in
`dtype` (float32: the reference's; float64: the same formulas on the same fp32 inputs, the yardstick of the reference's own rounding).
Pinned to the reference by tests/test_bpd_host.py before anything on the GPU is compared with it.
"""
import numpy as np

from oracle.rag_oracle import RagOracle, Schedule, q_sample  # noqa: F401  (re-exported for the tests)

F32 = np.float32
LN2 = np.log(2.0)
SEED_TAPE = 20201          # q_sample noise and style eps of the fixture loops
SEED_GRID = 20202          # the designed grid of G20k
TOL = 2e-4                 # this project's single-result tolerance on a model output (tests/test_gpu_plms.py)
FRAGILE_NATS = float(np.log(2.0 ** -18 / 1e-12))       # 15.16: what one ulp of tanh can move log(q) of a fragile element by
Q_CLAMP, Q_FRAGILE = 1e-12, 2.0 ** -18


def normal_kl(mean1, logvar1, mean2, logvar2, dtype=F32):
    """losses.py:33-39, operands already arrays of `dtype`."""
    h = dtype
    return h(0.5) * (h(-1.0) + logvar2 - logvar1 + np.exp(logvar1 - logvar2) + ((mean1 - mean2) ** 2) * np.exp(-logvar2))


def approx_cdf(x, dtype=F32):
    """losses.py:42-47 (np.sqrt(2 / pi) becomes a `dtype` scalar next to a tensor; th.pow(x, 3) is x * x * x)."""
    h = dtype
    return h(0.5) * (h(1.0) + np.tanh(h(np.sqrt(2.0 / np.pi)) * (x + h(0.044715) * (x * x * x))))


def discretized_q(x, means, log_scales, dtype=F32):
    """The probability whose clamped log discretized_gaussian_log_likelihood returns (losses.py:62-75), before the clamp."""
    h = dtype
    centered = x - means
    inv_stdv = np.exp(-log_scales)
    cdf_plus = approx_cdf(inv_stdv * (centered + h(1.0 / 255.0)), dtype)
    cdf_min = approx_cdf(inv_stdv * (centered - h(1.0 / 255.0)), dtype)
    return np.where(x < h(-0.999), cdf_plus, np.where(x > h(0.999), h(1.0) - cdf_min, cdf_plus - cdf_min))


def _col(sch, name, t, dtype):
    """_extract_into_tensor: the fp64 table entry of every sample cast to fp32 (then to `dtype`), broadcast over the sample's plane."""
    return getattr(sch, name)[np.asarray(t, dtype=np.int64)].astype(F32).astype(dtype).reshape(-1, 1, 1, 1)


def vb_terms(sch, x_start, x_t, pred_xstart, noise, t, clip_denoised=False, dtype=F32):
    """The three per-sample numbers of one column from (x_0, x_t, the model's x_0 prediction, the q_sample noise): t is one schedule
    index per sample.  Returns (vb [B], xstart_mse [B], mse [B] or None, pred_xstart used, q of the decoder NLL [B,J,F,T])."""
    h = dtype
    t = np.asarray(t, dtype=np.int64).reshape(-1)
    x0, xt, px = (np.asarray(v, dtype=F32).astype(h) for v in (x_start, x_t, pred_xstart))
    if clip_denoised:
        px = np.clip(px, h(-1), h(1))
    c1, c2 = _col(sch, "posterior_mean_coef1", t, h), _col(sch, "posterior_mean_coef2", t, h)
    lv = np.broadcast_to(_col(sch, "posterior_log_variance_clipped", t, h), x0.shape)
    true_mean = c1 * x0 + c2 * xt
    mean = c1 * px + c2 * xt
    flat = lambda a: a.reshape(a.shape[0], -1).mean(axis=1, dtype=h)      # noqa: E731  mean_flat
    kl = flat(normal_kl(true_mean, lv, mean, lv, h)) / h(LN2)
    q = discretized_q(x0, mean, h(0.5) * lv, h)
    nll = flat(-np.log(np.maximum(q, h(Q_CLAMP)))) / h(LN2)
    vb = np.where(t == 0, nll, kl).astype(h)
    xs = flat((px - x0) ** 2)
    ms = None
    if noise is not None:
        eps = (_col(sch, "sqrt_recip_alphas_cumprod", t, h) * xt - px) / _col(sch, "sqrt_recipm1_alphas_cumprod", t, h)
        ms = flat((eps - np.asarray(noise, dtype=F32).astype(h)) ** 2)
    return vb, xs, ms, px, q


def fragile_count(q64):
    """Elements per sample whose float64 q lies in (1e-12, 2^-18): there one ulp of an fp32 tanh moves log(q) by up to FRAGILE_NATS."""
    q64 = np.asarray(q64)
    return ((q64 > Q_CLAMP) & (q64 < Q_FRAGILE)).reshape(q64.shape[0], -1).sum(axis=1)


def q_mean_variance(sch, x_start, t):
    x_start = np.asarray(x_start, dtype=F32)
    return (_col(sch, "sqrt_alphas_cumprod", t, F32) * x_start,
            np.broadcast_to((1.0 - sch.alphas_cumprod)[np.asarray(t)].astype(F32).reshape(-1, 1, 1, 1), x_start.shape),
            np.broadcast_to(_col(sch, "log_one_minus_alphas_cumprod", t, F32), x_start.shape))


def prior_bpd(sch, x_start):
    B = len(x_start)
    mean, _, lv = q_mean_variance(sch, x_start, np.full(B, sch.num_timesteps - 1))
    kl = normal_kl(mean, lv, F32(0.0), F32(0.0))
    return (kl.reshape(B, -1).mean(axis=1, dtype=F32) / F32(LN2)).astype(F32)


def bpd_loop(model, sch, y, x_start, noise_tape, eps_tape, clip_denoised=True, hoisted=True, columns=None, dtype=F32, keep=None, f64=None):
    """calc_bpd_loop.  noise_tape [T, B, J, F, T'] and eps_tape [T, 2, B, 512] in column order (column k = schedule index T - 1 - k).
    keep (a dict): k -> (x_t, pred_xstart, q).  f64 (a dict): receives vb / xstart_mse / mse re-evaluated in float64 from the model's
    own fp32 pred_xstart, and n_frag [B], the fragile count of the t = 0 column (when that column is run)."""
    x_start = np.asarray(x_start, dtype=F32)
    B, T = x_start.shape[0], sch.num_timesteps
    cols = range(T) if columns is None else columns
    if hoisted:
        model.prepare(y)
    vb, xs, ms = (np.zeros((B, T), dtype) for _ in range(3))
    for k in cols:
        i = T - 1 - k
        x_t = q_sample(sch, x_start, i, noise_tape[k])
        t_model = np.full((B,), sch.timestep_map[i], dtype=np.int64)
        px = model.cfg_forward(x_t, t_model, y, eps_tape[k, 0], eps_tape[k, 1], hoisted)
        vb[:, k], xs[:, k], ms[:, k], px, q = vb_terms(sch, x_start, x_t, px, noise_tape[k], np.full(B, i), clip_denoised, dtype)
        if keep is not None:
            keep[k] = (x_t, px, q)
        if f64 is not None:
            for name in ("vb", "xstart_mse", "mse"):
                f64.setdefault(name, np.zeros((B, T)))
            f64["vb"][:, k], f64["xstart_mse"][:, k], f64["mse"][:, k], _, q64 = vb_terms(sch, x_start, x_t, px, noise_tape[k], np.full(B, i),
                                                                                          False, np.float64)
            if i == 0:
                f64["n_frag"] = fragile_count(q64)
    prior = prior_bpd(sch, x_start)
    return {"total_bpd": (vb.sum(axis=1, dtype=dtype) + prior).astype(dtype), "prior_bpd": prior, "vb": vb, "xstart_mse": xs, "mse": ms}


# ---------------------------------------------------------------------------------------------- tolerance rule R (the issue's)
def rule_r(ref, ref_f64, xstart_mse_ref, n_frag=None, n_elem=None):
    """Per-entry bound of the three [B, T] outputs: r * |ref| + 2 * |ref - ref_f64| with r = 2 * TOL / sqrt(min xstart_mse) -- an x_0
    prediction within TOL of the reference's moves each (x_0 - pred)^2 term by at most 2 TOL / |x_0 - pred| relatively; the second
    term is the reference's own arithmetic noise.  n_frag (vb only): the last column (t = 0) gets n_frag[b] * 15.16 / (n ln 2) bits."""
    r = 2.0 * TOL / np.sqrt(float(np.min(xstart_mse_ref)))
    bound = r * np.abs(ref.astype(np.float64)) + 2.0 * np.abs(ref.astype(np.float64) - ref_f64.astype(np.float64))
    if n_frag is not None:
        bound[:, -1] += np.asarray(n_frag, dtype=np.float64) * FRAGILE_NATS / (n_elem * LN2)
    return bound


# ---------------------------------------------------------------------------------------------- fixture inputs (G20 / G20k)
B = 4
#: tag -> (diffusion_steps, respacing, clip_denoised)
LOOPS = {
    "ted": {"G20_ddim100": (1000, "ddim100", False), "G20_ddim100_clip": (1000, "ddim100", True), "G20_full1000": (1000, "", True)},
    "beat": {"G20_ddim100": (1000, "ddim100", True)},
}
#: the x_start seed of synth.make_init_image per dataset (changed, never the cap, if a dataset's fragile share exceeds 1 %)
X_START_SEED = {"ted": None, "beat": None}
GRID_T = (0, 1, 50, 99)             # uniform schedule indices of G20k (ddim100)
GRID_MIXED = (0, 37, 98, 99)        # and one vector with a different index per sample


def loop_tape(cfg, n_cols, seed=SEED_TAPE, batch=B):
    """(q_sample noise [n_cols, B, J, F, T], style eps [n_cols, 2, B, 512]) of a fixture loop, column by column in the reference's draw
    order (so a prefix of a longer tape is the shorter tape)."""
    g = np.random.Generator(np.random.PCG64(seed))
    nz = np.empty((n_cols, batch, cfg.njoints, cfg.nfeats, cfg.nframes), F32)
    eps = np.empty((n_cols, 2, batch, 512), F32)
    for k in range(n_cols):
        nz[k] = g.standard_normal(nz.shape[1:]).astype(F32)
        eps[k] = g.standard_normal(eps.shape[1:]).astype(F32)
    return nz, eps


def grid_inputs(cfg, sch, t, seed=SEED_GRID, batch=B):
    """The designed grid of G20k at schedule indices t [B]: x_start uniform in [-1.2, 1.2] (both +-0.999 branches occur), x_t from
    q_sample, pred_xstart = x_start - z * sigma_t * sign with |z| from [0, 3] u [8, 40] (so q of the decoder NLL is either well
    conditioned or clamps outright: no fragile element).  Returns (x_start, x_t, pred_xstart, noise)."""
    g = np.random.Generator(np.random.PCG64(seed))
    shp = (batch, cfg.njoints, cfg.nfeats, cfg.nframes)
    x0 = g.uniform(-1.2, 1.2, shp).astype(F32)
    noise = g.standard_normal(shp).astype(F32)
    z = np.where(g.random(shp) < 0.7, g.uniform(0.0, 3.0, shp), g.uniform(8.0, 40.0, shp))
    sign = np.where(g.random(shp) < 0.5, -1.0, 1.0)
    t = np.asarray(t, dtype=np.int64)
    sigma = np.exp(0.5 * sch.posterior_log_variance_clipped[t]).reshape(-1, 1, 1, 1)
    x_t = (_col(sch, "sqrt_alphas_cumprod", t, F32) * x0 + _col(sch, "sqrt_one_minus_alphas_cumprod", t, F32) * noise).astype(F32)
    pred = (x0 - z * sigma * sign).astype(F32)
    return x0, x_t, pred, noise
