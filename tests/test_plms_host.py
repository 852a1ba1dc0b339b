"""CPU: the restatement of PLMS and of the DDIM reverse step (tests/plms_restatement.py) against the fixtures G17 / G18 that
tests/golden/make_golden_plms.py produced by importing the reference, the alphas_cumprod_next table, and what the new entry points of
GaussianDiffusion refuse before an engine is touched."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import plms_restatement as pr
from conftest import GOLDEN, max_abs
from livelyspeaker_amd import synth
from livelyspeaker_amd.cfg_sampler import ClassifierFreeSampleModel
from livelyspeaker_amd.model_util import create_model_and_diffusion

TOL = 2e-4      # the bound tests/test_oracle_golden.py uses for its loops


def eps_tol(sch, t):
    return pr.eps_tol(sch, t, TOL)


def mk_args(steps=1000, njoints=9):
    return SimpleNamespace(mdm_condm="text", latent_dim=512, ff_size=1024, layers=8, cond_mask_prob=0.1,
                           arch="trans_enc", emb_trans_dec=False, dataset="humanml", lang_model=None, mlpact="silu",
                           diffusion_steps=steps, noise_schedule="cosine", sigma_small=True, lambda_vel=1.0,
                           lambda_rcxyz=0.0, lambda_fc=0.0, njoints=njoints)


@pytest.fixture(scope="module")
def golden_plms():
    return {ds: np.load(os.path.join(GOLDEN, f"{ds}_golden_plms.npz")) for ds in ("ted", "beat")}


def _oracle(ds):
    cfg = synth.CONFIGS[ds]
    return cfg, pr.RagOracle(synth.make_state_dict(cfg), cfg.njoints, cfg.nfeats, cfg.n_prefix_tokens)


def test_fixture_files_are_small_and_complete(golden_plms):
    for ds in ("ted", "beat"):
        assert os.path.getsize(os.path.join(GOLDEN, f"{ds}_golden_plms.npz")) < 1_000_000
        for tag in pr.LOOPS[ds]:
            assert f"{tag}_samples" in golden_plms[ds].files
        for tag in pr.REVERSE[ds]:
            assert f"{tag}_sample" in golden_plms[ds].files
    for tag in pr.STEPS:
        assert f"{tag}_sample" in golden_plms["ted"].files


@pytest.mark.parametrize("ds,tag", [(ds, tag) for ds in ("ted", "beat") for tag in pr.LOOPS[ds]])
def test_restated_plms_loop_matches_the_reference(golden_plms, ds, tag):
    g = golden_plms[ds]
    cfg, oracle = _oracle(ds)
    steps, resp, skip, use_init, clip, order, keep = pr.LOOPS[ds][tag]
    sch = pr.Schedule(steps, resp)
    n_exec = sch.num_timesteps - skip
    x_init, eps = pr.loop_tape(cfg, n_exec + 1)
    ys = []
    final = pr.plms_loop(oracle, sch, synth.make_cond(cfg, pr.B), x_init, eps, order, skip_timesteps=skip,
                         init_image=synth.make_init_image(cfg, pr.B) if use_init else None, clip_denoised=clip, yields=ys)
    ks = pr.kept(n_exec, keep)
    assert list(g[f"{tag}_yields"]) == ks and len(ys) == n_exec
    for j, k in enumerate(ks):
        d = max_abs(ys[k][0], g[f"{tag}_samples"][j])
        print(f"{ds} {tag} yield {k}: sample {d:.2e}")
        assert d < TOL, (k, d)
        if ds == "ted":
            d = max_abs(ys[k][1], g[f"{tag}_x0"][j])
            assert d < TOL, (k, d)
    if ds == "beat":
        assert max_abs(ys[0][1], g["G17_first_x0"]) < TOL
    assert np.array_equal(final, ys[-1][0]) and np.array_equal(ys[-1][0], ys[-1][1])         # t = 0: sample is pred_xstart


def test_orders_are_told_apart_by_the_fixtures(golden_plms):
    """Orders 2 / 3 / 4 differ from each other by far more than any tolerance here: a wrong order or history cannot hide."""
    g = golden_plms["ted"]
    last = {o: g[f"G17_o{o}_samples"][-1] for o in (2, 3, 4)}
    for a, b in ((2, 3), (3, 4), (2, 4)):
        assert max_abs(last[a], last[b]) > 0.1
    assert max_abs(g["G17_o2_samples"][0], g["G17_o4_samples"][0]) == 0.0      # the two-evaluation first step does not depend on it


@pytest.mark.parametrize("tag", list(pr.STEPS))
def test_restated_plms_step_with_a_given_history_matches_the_reference(golden_plms, tag):
    """sample / pred_xstart at the plain TOL; the eps plane at TOL in x0's units (pr.eps_tol: measured 2.3e-5 at t = 50 against 2e-4,
    8.5e-4 at t = 0 -- |eps| up to 1.2e3 there -- against 3.1e-2)."""
    g = golden_plms["ted"]
    cfg, oracle = _oracle("ted")
    resp, t, order, nh = pr.STEPS[tag]
    sch = pr.Schedule(1000, resp)
    x, hist, eps = pr.step_inputs(cfg)
    y = synth.make_cond(cfg, pr.B)
    oracle.prepare(y)
    sample, x0, old = pr.plms_step(oracle, sch, y, x, t, [eps], order, hist[3 - nh:])
    assert max_abs(sample, g[f"{tag}_sample"]) < TOL and max_abs(x0, g[f"{tag}_x0"]) < TOL
    d = max_abs(old[-1], g[f"{tag}_last_eps"])
    print(f"{tag}: last eps differs by {d:.2e} (|eps| max {np.abs(old[-1]).max():.1f}), bound {eps_tol(sch, t):.2e}")
    assert len(old) == int(g[f"{tag}_len"].item()) == order - 1 and d < eps_tol(sch, t)
    if t == 0:
        assert np.array_equal(sample, x0)


@pytest.mark.parametrize("ds,tag", [(ds, tag) for ds in ("ted", "beat") for tag in pr.REVERSE[ds]])
def test_restated_ddim_reverse_step_matches_the_reference(golden_plms, ds, tag):
    g = golden_plms[ds]
    cfg, oracle = _oracle(ds)
    resp, t = pr.REVERSE[ds][tag]
    sch = pr.Schedule(1000, resp)
    x, _, eps = pr.step_inputs(cfg)
    sample, x0 = pr.ddim_reverse_step(oracle, sch, synth.make_cond(cfg, pr.B), x, np.full((pr.B,), t), eps)
    assert max_abs(sample, g[f"{tag}_sample"]) < TOL
    if ds == "ted":
        assert max_abs(x0, g[f"{tag}_x0"]) < TOL
    if t == sch.num_timesteps - 1:          # alpha_bar_next = 0: the sample is eps itself
        eps_host = (sch.f32("sqrt_recip_alphas_cumprod", t) * x - x0) / sch.f32("sqrt_recipm1_alphas_cumprod", t)
        assert max_abs(sample, eps_host) < 1e-6


@pytest.mark.parametrize("steps,resp", [(1000, ""), (1000, "ddim100")])
def test_alphas_cumprod_next_is_the_reference_table(golden, steps, resp):
    _, diff = create_model_and_diffusion(mk_args(steps), resp)
    want = np.append(diff.alphas_cumprod[1:], 0.0)          # gaussian_diffusion.py:178
    assert diff.alphas_cumprod_next.dtype == np.float64 and np.array_equal(diff.alphas_cumprod_next, want)
    assert np.array_equal(diff.alphas_cumprod_next, golden["ted"][f"G0_{steps}_{resp or 'full'}_alphas_cumprod_next"])
    assert np.array_equal(diff.alphas_cumprod_next, pr.Schedule(steps, resp).alphas_cumprod_next)


def test_new_samplers_refuse_bad_arguments_before_an_engine_exists():
    model, diff = create_model_and_diffusion(mk_args(steps=5), "")
    cfgm = ClassifierFreeSampleModel(model)
    y = {"dummy": torch.zeros(2)}
    shape = (2, 9, 3, 34)
    x, t = torch.zeros(shape), torch.full((2,), 3)
    state = torch.get_rng_state()
    for bad in (0, 5, 2.5, True, "2"):
        for call in (lambda: diff.plms_sample_loop(cfgm, shape, model_kwargs={"y": y}, order=bad),
                     lambda: diff.plms_sample_loop_progressive(cfgm, shape, model_kwargs={"y": y}, order=bad),
                     lambda: diff.plms_sample(cfgm, x, t, model_kwargs={"y": y}, order=bad)):
            with pytest.raises(ValueError, match="order is invalid"):
                call()
    for fn in (diff.plms_sample_loop, diff.plms_sample_loop_progressive):
        with pytest.raises(ValueError, match="ddim_sample_loop"):                 # the reference dies with a TypeError at its first step
            fn(cfgm, shape, model_kwargs={"y": y}, order=1)
        with pytest.raises(ValueError, match="at least two executed steps"):
            fn(cfgm, shape, model_kwargs={"y": y}, order=2, skip_timesteps=4)
        with pytest.raises(NotImplementedError):
            fn(cfgm, shape, model_kwargs={"y": y}, cond_fn=lambda *a: None)
        with pytest.raises(NotImplementedError):
            fn(cfgm, shape, model_kwargs={"y": y}, denoised_fn=lambda v: v)
        with pytest.raises(NotImplementedError, match="inpainting"):
            fn(cfgm, shape, model_kwargs={"y": {"inpainting_mask": torch.zeros(shape, dtype=torch.bool), "inpainted_motion": torch.zeros(shape)}})
    with pytest.raises(ValueError, match="order=1"):
        diff.plms_sample(cfgm, x, t, model_kwargs={"y": y}, order=1)
    with pytest.raises(NotImplementedError):
        diff.plms_sample(cfgm, x, t, model_kwargs={"y": y}, cond_fn=lambda *a: None)
    with pytest.raises(NotImplementedError):
        diff.plms_sample(cfgm, x, t, model_kwargs={"y": y}, cond_fn_with_grad=True)
    with pytest.raises(ValueError, match="njoints"):
        diff.plms_sample_loop_progressive(cfgm, (2, 9, 3, 30), model_kwargs={"y": y})
    with pytest.raises(ValueError, match="model_kwargs"):
        diff.plms_sample_loop_progressive(cfgm, shape, model_kwargs=None)
    gen = diff.plms_sample_loop_progressive(cfgm, list(shape), model_kwargs={"y": y}, device="cpu", order=4)     # accepted: nothing has run yet
    assert hasattr(gen, "__next__")
    with pytest.raises(AssertionError, match="deterministic"):
        diff.ddim_reverse_sample(cfgm, x, t, model_kwargs={"y": y}, eta=0.1)
    with pytest.raises(NotImplementedError):
        diff.ddim_reverse_sample(cfgm, x, t, model_kwargs={"y": y}, denoised_fn=lambda v: v)
    with pytest.raises(NotImplementedError, match="inpainting"):
        diff.ddim_reverse_sample(cfgm, x, t, model_kwargs={"y": {"inpainting_mask": torch.zeros(shape, dtype=torch.bool), "inpainted_motion": torch.zeros(shape)}})
    assert torch.equal(state, torch.get_rng_state())          # none of the refusals drew anything


def test_abi_mirror_of_the_plms_step_arguments(tmp_path):
    """LsPlmsStepArgs against what a C compiler makes of include/ls_hip.h; the sampler codes and the renamed order field."""
    import ctypes
    import subprocess
    from conftest import ROOT
    from livelyspeaker_amd import _lib
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ls_hip.h"\nint main(void) {\n'
                   '    printf("%zu %zu %zu %zu %d %d\\n", sizeof(ls_plms_step_args), offsetof(ls_plms_step_args, hist), offsetof(ls_plms_step_args, eps_out),\n'
                   '           offsetof(ls_sample_args, plms_order), LS_SAMPLER_PLMS, LS_SAMPLER_DDIM_REVERSE);\n    return 0;\n}\n')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    A = _lib.LsPlmsStepArgs
    assert got == [ctypes.sizeof(A), A.hist.offset, A.eps_out.offset, _lib.LsSampleArgs.plms_order.offset,
                   _lib.LS_SAMPLER_PLMS, _lib.LS_SAMPLER_DDIM_REVERSE]
    assert "ls_plms_step" in _lib.EXPORTS
