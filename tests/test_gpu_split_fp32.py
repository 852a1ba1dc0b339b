"""Split-fp32 channel mixing (the default 'fp32' precision of the fused step kernel, k_step PREC 2) against the fp32-MFMA kernel
('fp32_mfma', PREC 0) on the GPU:

  * accuracy gate: single forwards of TED and BEAT, cond and uncond, at t in {0, 500, 999}, against a float64 evaluation of the
    same forward (oracle/rag_torch_cpu.py's hoisted forward run in double).  The split path's max-abs and RMS error may be at most
    1.25x those of the fp32 MFMA on the same inputs.
  * loop: a 1000-step DDPM loop at B = 512 on the same Philox seed lands within the loop tolerance of the fp32-MFMA loop.
  * graph replay equals plain launches bitwise."""
import numpy as np
import pytest
import torch

from livelyspeaker_amd import synth

pytestmark = pytest.mark.gpu

TOL_LOOP = 3e-4          # the full-loop tolerance of tests/test_gpu_parity.py
GATE = 1.25
B_FWD = 8


def _engine(ds):
    from livelyspeaker_amd import _lib
    cfg = synth.CONFIGS[ds]
    eng = _lib.Engine(cfg.njoints, cfg.nfeats, cfg.n_prefix_tokens, cfg.audio_len, n_emotions=cfg.n_emotions)
    eng.load_state_dict(synth.make_state_dict(cfg))
    return cfg, eng


def _fp64_forward(cfg, y, x, t, eps_c, eps_u):
    """(cond, uncond) outputs of the hoisted forward, every parameter and activation in float64."""
    from oracle.rag_torch_cpu import TorchCpuSampler
    s = TorchCpuSampler(synth.make_state_dict(cfg), cfg.njoints, cfg.nfeats, cfg.n_prefix_tokens)
    s.P = {k: v.double() for k, v in s.P.items()}
    s.pe = torch.as_tensor(np.asarray(s.pe)).double()
    yd = {k: (torch.from_numpy(np.asarray(v)).double() if np.asarray(v).dtype.kind == "f" else torch.from_numpy(np.asarray(v)))
          for k, v in y.items()}
    with torch.no_grad():
        s.prepare(yd)
        temb = s.time_embed(torch.tensor([t], dtype=torch.long))[0]
        xd, ec, eu = (torch.from_numpy(np.asarray(a, dtype=np.float64)) for a in (x, eps_c, eps_u))
        out = {}
        for name, sc in (("c", 1.0), ("u", 0.0)):
            yd["scale"] = torch.full((x.shape[0],), sc, dtype=torch.float64)
            out[name] = s.cfg_forward_hoisted(xd, temb, yd, ec, eu).numpy()
    return out


@pytest.fixture(scope="module", params=["ted", "beat"])
def fwd_ctx(request):
    ds = request.param
    cfg, eng = _engine(ds)
    eng.set_path("fused")                       # the fused kernel is the one with the split-fp32 form
    y = synth.make_cond(cfg, B_FWD)
    eng.prepare(y)
    eng.set_schedule(synth.schedule(1000))
    yield cfg, eng, y
    eng.close()


@pytest.mark.parametrize("t", [0, 500, 999])
def test_forward_error_vs_fp64_within_gate_of_fp32_mfma(fwd_ctx, t):
    cfg, eng, y = fwd_ctx
    g = np.random.Generator(np.random.PCG64(4321 + t))
    x = g.standard_normal((B_FWD, cfg.njoints, cfg.nfeats, cfg.nframes)).astype(np.float32)
    eps = g.standard_normal((2, B_FWD, 512)).astype(np.float32)
    ref = _fp64_forward(cfg, y, x, t, eps[0], eps[1])
    err, outs = {}, {}
    for mode in ("fp32_mfma", "fp32"):
        eng.set_precision(mode)
        oc, ou, _ = eng.forward(x, np.full((B_FWD,), t), eps[0], eps[1])
        outs[mode] = np.concatenate([np.asarray(oc).ravel(), np.asarray(ou).ravel()])
        d = np.concatenate([(np.asarray(oc, np.float64) - ref["c"]).ravel(), (np.asarray(ou, np.float64) - ref["u"]).ravel()])
        err[mode] = (float(np.abs(d).max()), float(np.sqrt(np.mean(d * d))))
    eng.set_precision("fp32")
    print(f"t={t}: max-abs / RMS vs fp64: fp32_mfma {err['fp32_mfma'][0]:.3e} / {err['fp32_mfma'][1]:.3e}, "
          f"split-fp32 {err['fp32'][0]:.3e} / {err['fp32'][1]:.3e}")
    # the two modes ran different kernels (PREC 2 and PREC 0): their sums round differently, so the outputs cannot be bitwise equal
    assert not np.array_equal(outs["fp32"], outs["fp32_mfma"])
    assert err["fp32"][0] <= GATE * err["fp32_mfma"][0], err
    assert err["fp32"][1] <= GATE * err["fp32_mfma"][1], err


def _loop(eng, mode, use_graph=True):
    eng.set_precision(mode)
    return np.asarray(eng.sample(sampler=0, philox_seed=7, use_graph=use_graph))


@pytest.fixture(scope="module")
def loop_ctx():
    cfg, eng = _engine("ted")
    eng.set_schedule(synth.schedule(1000))
    eng.prepare(synth.make_cond(cfg, 512))
    yield eng
    eng.close()


def test_ddpm_1000_steps_b512_split_vs_fp32_mfma(loop_ctx):
    eng = loop_ctx
    ref = _loop(eng, "fp32_mfma")
    got = _loop(eng, "fp32")
    d = float(np.abs(got - ref).max())
    print(f"1000-step DDPM, B = 512: max|split-fp32 - fp32_mfma| = {d:.3e}")
    assert np.isfinite(got).all()
    assert 0 < d < TOL_LOOP                      # 0 would mean 'fp32' still ran the fp32-MFMA kernel


def test_graph_replay_equals_plain_launches(loop_ctx):
    eng = loop_ctx
    a = _loop(eng, "fp32", use_graph=True)
    b = _loop(eng, "fp32", use_graph=True)       # replay of the captured graph
    c = _loop(eng, "fp32", use_graph=False)
    assert np.array_equal(a, b) and np.array_equal(a, c)
