"""CPU restatement of the PLMS sampler and of the DDIM reverse step (scripts/diffusion/gaussian_diffusion.py:1016-1211, 857-893) on the
numpy oracle, plus the inputs the PLMS fixtures (tests/golden/make_golden_plms.py) and their tests share.  Not a test module.

Arithmetic as the reference writes it: tables cast fp64 -> fp32 per step (Schedule.f32 = _extract_into_tensor), square roots in fp32
on the cast value, every intermediate fp32.  Pinned to the reference by tests/test_plms_host.py (fixtures G17 / G18) before anything
on the GPU is compared with it.
"""
import numpy as np

from oracle.rag_oracle import RagOracle, Schedule, q_sample  # noqa: F401  (re-exported for the tests)

F32 = np.float32
SEED_TAPE = 71717          # x_T and style eps of the fixture loops
SEED_STEP = 71718          # x, history planes and style eps of the single-step fixtures


def check_order(order):
    if isinstance(order, bool) or not isinstance(order, (int, np.integer)) or not 1 <= order <= 4:
        raise ValueError('order is invalid (should be int from 1-4).')


def _eps_from_xstart(sch, x, i, x0):
    return ((sch.f32("sqrt_recip_alphas_cumprod", i) * x - x0) / sch.f32("sqrt_recipm1_alphas_cumprod", i)).astype(F32)


def _mean_from_eps(sch, x, i, eps):
    abp = sch.f32("alphas_cumprod_prev", i)
    pred = (sch.f32("sqrt_recip_alphas_cumprod", i) * x - sch.f32("sqrt_recipm1_alphas_cumprod", i) * eps).astype(F32)
    return (pred * np.sqrt(abp) + np.sqrt(F32(1) - abp) * eps).astype(F32)


def _x0(model, sch, y, x, i, eps_pair, clip_denoised, hoisted):
    t_model = np.full((x.shape[0],), sch.timestep_map[i], dtype=np.int64)        # _WrappedModel, respace.py:125-130
    x0 = model.cfg_forward(x, t_model, y, eps_pair[0], eps_pair[1], hoisted)
    return np.clip(x0, -1, 1).astype(F32) if clip_denoised else x0               # process_xstart BEFORE eps is derived


def plms_step(model, sch, y, x, i, eps_pairs, order, old_eps, clip_denoised=False, hoisted=True):
    """plms_sample at schedule index i.  eps_pairs: the (cond, uncond) style eps of the evaluations this step makes, in order (two
    pairs when old_eps is None).  Returns (sample, pred_xstart, old_eps carried forward)."""
    check_order(order)
    x = np.asarray(x, dtype=F32)
    x0 = _x0(model, sch, y, x, i, eps_pairs[0], clip_denoised, hoisted)
    eps = _eps_from_xstart(sch, x, i, x0)
    if order > 1 and old_eps is None:
        abp = sch.f32("alphas_cumprod_prev", i)
        old = [eps]
        mean_pred = (x0 * np.sqrt(abp) + np.sqrt(F32(1) - abp) * eps).astype(F32)
        x0_2 = _x0(model, sch, y, mean_pred, i - 1, eps_pairs[1], clip_denoised, hoisted)
        eps_2 = _eps_from_xstart(sch, mean_pred, i - 1, x0_2)
        eps_p = ((eps + eps_2) / F32(2)).astype(F32)
    else:
        old = list(old_eps) + [eps]
        cur = min(order, len(old))
        if cur == 1:
            eps_p = old[-1]
        elif cur == 2:
            eps_p = (F32(3) * old[-1] - old[-2]) / F32(2)
        elif cur == 3:
            eps_p = (F32(23) * old[-1] - F32(16) * old[-2] + F32(5) * old[-3]) / F32(12)
        else:
            eps_p = (F32(55) * old[-1] - F32(59) * old[-2] + F32(37) * old[-3] - F32(9) * old[-4]) / F32(24)
        eps_p = eps_p.astype(F32)
    mean_pred = _mean_from_eps(sch, x, i, eps_p)
    if len(old) >= order:
        old.pop(0)
    return (mean_pred if i != 0 else x0), x0, old


def plms_loop(model, sch, y, x_init, eps_tape, order, skip_timesteps=0, init_image=None, clip_denoised=False, hoisted=True,
              yields=None):
    """plms_sample_loop_progressive.  eps_tape [n_exec + 1, 2, B, 512] in evaluation order.  Returns the final sample, or with
    yields = a list: [(sample, pred_xstart)] of every step."""
    check_order(order)
    img = np.asarray(x_init, dtype=F32)
    if skip_timesteps and init_image is None:
        init_image = np.zeros_like(img)
    indices = list(range(sch.num_timesteps - skip_timesteps))[::-1]
    assert order > 1 and len(indices) >= 2 and len(eps_tape) == len(indices) + 1
    if init_image is not None:
        img = q_sample(sch, np.asarray(init_image, dtype=F32), indices[0], img)
    if hoisted:
        model.prepare(y)
    old, e = None, 0
    for i in indices:
        n = 2 if old is None else 1
        img, x0, old = plms_step(model, sch, y, img, i, [eps_tape[e + j] for j in range(n)], order, old, clip_denoised, hoisted)
        e += n
        if yields is not None:
            yields.append((img, x0))
    assert e == len(eps_tape)
    return img


def ddim_reverse_step(model, sch, y, x, t, eps_pair, clip_denoised=False, hoisted=True):
    """ddim_reverse_sample; t: one schedule index per sample ([B] ints).  Returns (sample, pred_xstart)."""
    x = np.asarray(x, dtype=F32)
    t = np.asarray(t, dtype=np.int64)
    t_model = sch.timestep_map[t]
    if hoisted:
        model.prepare(y)
    x0 = model.cfg_forward(x, t_model, y, eps_pair[0], eps_pair[1], hoisted)
    if clip_denoised:
        x0 = np.clip(x0, -1, 1).astype(F32)
    col = lambda name: getattr(sch, name)[t].astype(F32).reshape(-1, 1, 1, 1)      # noqa: E731
    eps = ((col("sqrt_recip_alphas_cumprod") * x - x0) / col("sqrt_recipm1_alphas_cumprod")).astype(F32)
    abn = col("alphas_cumprod_next")
    return (x0 * np.sqrt(abn) + np.sqrt(F32(1) - abn) * eps).astype(F32), x0


def eps_tol(sch, t, tol):
    """Bound for an eps plane, eps = (sqrt_recip_ac[t] * x - x0) / sqrt_recipm1_ac[t] (_predict_eps_from_xstart): an error d of the
    model output x0 -- which `tol` bounds -- IS d / sqrt_recipm1_ac[t] in eps, whatever computes it.  The divisor is 0.0064 at t = 0 of the
    ddim100 tables (eps values of several hundred, one fp32 ulp of them 6e-5), about 1 at t = 50.  So eps is held to `tol` in the units of
    the x0 it was derived from: |d eps| * min(1, sqrt_recipm1_ac[t]) < tol.  samples and pred_xstart keep the plain bound."""
    return tol / min(1.0, float(sch.f32("sqrt_recipm1_alphas_cumprod", t)))


# ---------------------------------------------------------------------------------------------- fixture inputs (G17 / G18)
B = 4
#: tag -> (diffusion_steps, respacing, skip_timesteps, init_image?, clip_denoised, order, yields kept (None = all; negative = from the end))
LOOPS = {
    "ted": {
        "G17_o4": (1000, "ddim100", 88, True, False, 4, None),
        "G17_o2": (1000, "ddim100", 88, True, False, 2, (0, 1, -1)),
        "G17_o3": (1000, "ddim100", 88, True, False, 3, (0, 1, -1)),
        "G17_o2_clip": (1000, "ddim100", 88, True, True, 2, (-1,)),
        "G17_o3_full1000": (1000, "", 990, False, False, 3, (-1,)),
    },
    # BEAT arrays are ten times TED's: samples of the first and the last yield only (the last pred_xstart IS the last sample, t = 0),
    # and the first yield's pred_xstart once (the first evaluation's, the same for every order)
    "beat": {
        "G17_o2": (1000, "ddim100", 88, True, False, 2, (0, -1)),
        "G17_o4": (1000, "ddim100", 88, True, False, 4, (0, -1)),
    },
}
#: tag -> (respacing, t, order, history planes handed in)
STEPS = {"G17_step_o3_t50": ("ddim100", 50, 3, 2), "G17_step_o4_t50": ("ddim100", 50, 4, 3),
         "G17_step_o3_t0": ("ddim100", 0, 3, 2), "G17_step_o4_t0": ("ddim100", 0, 4, 3)}
#: tag -> (respacing, t)
REVERSE = {"ted": {"G18_t0": ("ddim100", 0), "G18_t50": ("ddim100", 50), "G18_t99": ("ddim100", 99), "G18_full1000_t999": ("", 999)},
           "beat": {"G18_t50": ("ddim100", 50)}}


def loop_tape(cfg, n_eval, seed=SEED_TAPE, batch=B):
    """(x_T [B,J,F,T], style eps [n_eval, 2, B, 512]) of a fixture loop."""
    g = np.random.Generator(np.random.PCG64(seed))
    x_init = g.standard_normal((batch, cfg.njoints, cfg.nfeats, cfg.nframes)).astype(F32)
    return x_init, g.standard_normal((n_eval, 2, batch, 512)).astype(F32)


def step_inputs(cfg, seed=SEED_STEP, batch=B):
    """(x, three history planes oldest first, one pair of style eps) of the single-step fixtures."""
    g = np.random.Generator(np.random.PCG64(seed))
    shp = (batch, cfg.njoints, cfg.nfeats, cfg.nframes)
    x = g.standard_normal(shp).astype(F32)
    hist = [g.standard_normal(shp).astype(F32) for _ in range(3)]
    return x, hist, g.standard_normal((2, batch, 512)).astype(F32)


def kept(n_exec, keep):
    return list(range(n_exec)) if keep is None else [k % n_exec for k in keep]
