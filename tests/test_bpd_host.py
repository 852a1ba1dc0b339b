"""The variational bound in bits per dimension on the host: q_mean_variance / _prior_bpd against the reference (fixture G20), the CPU
restatement (tests/bpd_restatement.py) against every G20 loop and the kernel-level grid G20k, the draw order of calc_bpd_loop's torch_cpu
mode on a stub engine, and the refusals that need no GPU.  Fixtures: tests/golden/make_golden_bpd.py."""
import ctypes
import os
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import bpd_restatement as br
from conftest import GOLDEN, ROOT
from livelyspeaker_amd import _lib, synth
from livelyspeaker_amd import gaussian_diffusion as gd
from livelyspeaker_amd.cfg_sampler import ClassifierFreeSampleModel
from livelyspeaker_amd.model_util import create_model_and_diffusion

LN2 = np.log(2.0)


def mk_args(steps=1000, njoints=9):
    return SimpleNamespace(mdm_condm="text", latent_dim=512, ff_size=1024, layers=8, cond_mask_prob=0.1, arch="trans_enc",
                           emb_trans_dec=False, dataset="humanml", lang_model=None, mlpact="silu", diffusion_steps=steps,
                           noise_schedule="cosine", sigma_small=True, lambda_vel=1.0, lambda_rcxyz=0.0, lambda_fc=0.0, njoints=njoints)


@pytest.fixture(scope="module")
def golden_bpd():
    return {ds: np.load(os.path.join(GOLDEN, f"{ds}_golden_bpd.npz")) for ds in ("ted", "beat")}


def x_start_of(ds):
    cfg = synth.CONFIGS[ds]
    seed = br.X_START_SEED[ds]
    return synth.make_init_image(cfg, br.B) if seed is None else synth.make_init_image(cfg, br.B, seed)


def check_rule_r(got, g, tag, n_elem, what=""):
    """Rule R on the three [B, T] outputs and on total_bpd (the sum of its columns' bounds); prior_bpd to 2e-7 bits.  Prints each
    figure before it asserts."""
    xs_ref = g[f"{tag}_xstart_mse"]
    total_bound = 0.0
    for k in ("vb", "xstart_mse", "mse"):
        ref, f64 = g[f"{tag}_{k}"], g[f"{tag}_{k}_f64"]
        bound = br.rule_r(ref, f64, xs_ref, g[f"{tag}_n_frag"] if k == "vb" else None, n_elem)
        err = np.abs(np.asarray(got[k], dtype=np.float64) - ref)
        worst = float((err / bound).max())
        print(f"{what}{tag} {k}: worst |err| / bound {worst:.3f} (max rel err {float((err / np.abs(ref)).max()):.2e})")
        assert worst <= 1.0, (tag, k, worst)
        if k == "vb":
            total_bound = bound.sum(axis=1)
    dp = float(np.abs(np.asarray(got["prior_bpd"], dtype=np.float64) - g[f"{tag}_prior_bpd"]).max())
    dt = np.abs(np.asarray(got["total_bpd"], dtype=np.float64) - g[f"{tag}_total_bpd"])
    print(f"{what}{tag} prior_bpd |err| {dp:.2e}, total_bpd worst |err| / bound {float((dt / total_bound).max()):.3f}")
    assert dp <= 2e-7
    assert (dt <= total_bound).all()


def test_fixture_files_are_small_and_complete(golden_bpd):
    for ds in ("ted", "beat"):
        assert os.path.getsize(os.path.join(GOLDEN, f"{ds}_golden_bpd.npz")) < (1 << 20)
        n_elem = x_start_of(ds)[0].size
        for tag, (steps, resp, _) in br.LOOPS[ds].items():
            T = br.Schedule(steps, resp).num_timesteps
            for k in ("vb", "xstart_mse", "mse"):
                assert golden_bpd[ds][f"{tag}_{k}"].shape == golden_bpd[ds][f"{tag}_{k}_f64"].shape == (br.B, T)
            assert golden_bpd[ds][f"{tag}_n_frag"].max() <= 0.01 * n_elem           # the cap the t = 0 allowance rests on
    assert float(golden_bpd["ted"]["G20k_q_min"].reshape(-1)[0]) >= 2.0 ** -10


def test_q_mean_variance_and_prior_bpd_match_the_reference(golden_bpd):
    g = golden_bpd["ted"]
    _, diff = create_model_and_diffusion(mk_args(), "ddim100")
    x0 = torch.from_numpy(x_start_of("ted"))
    t = torch.from_numpy(g["G20_qmv_t"])
    mean, var, lv = diff.q_mean_variance(x0, t)
    assert mean.shape == var.shape == lv.shape == x0.shape
    assert np.array_equal(mean.numpy(), g["G20_qmv_mean"])
    assert np.array_equal(var[:, 0, 0, 0].numpy(), g["G20_qmv_variance"]) and np.array_equal(lv[:, 0, 0, 0].numpy(), g["G20_qmv_log_variance"])
    for ds in ("ted", "beat"):
        for tag, (steps, resp, _) in br.LOOPS[ds].items():
            _, diff = create_model_and_diffusion(mk_args(steps, synth.CONFIGS[ds].njoints), resp)
            p = diff._prior_bpd(torch.from_numpy(x_start_of(ds)))
            d = float(np.abs(p.numpy().astype(np.float64) - golden_bpd[ds][f"{tag}_prior_bpd"]).max())
            print(f"{ds} {tag}: prior_bpd {p.numpy()} |err| {d:.2e}")
            assert p.shape == (br.B,) and d <= 2e-7


@pytest.mark.parametrize("ds,tag", [(ds, tag) for ds in ("ted", "beat") for tag in br.LOOPS[ds]])
def test_restated_loop_matches_the_reference(golden_bpd, ds, tag):
    steps, resp, clip = br.LOOPS[ds][tag]
    cfg = synth.CONFIGS[ds]
    sch = br.Schedule(steps, resp)
    T = sch.num_timesteps
    # the ddim100 loops run whole; of the unspaced 1000 columns (50 s on the numpy oracle) every tenth, the first 3 and the last 30 are run
    cols = list(range(T)) if T <= 100 else sorted(set(range(0, T, 10)) | set(range(3)) | set(range(T - 30, T)))
    nz, eps = br.loop_tape(cfg, T)
    model = br.RagOracle(synth.make_state_dict(cfg), cfg.njoints, cfg.nfeats, cfg.n_prefix_tokens, nframes=cfg.nframes)
    x0 = x_start_of(ds)
    r = br.bpd_loop(model, sch, synth.make_cond(cfg, br.B), x0, nz, eps, clip, columns=cols)
    g = golden_bpd[ds]
    if len(cols) < T:               # columns not run take the reference's values: the bounds of the others are checked as they are
        for k in ("vb", "xstart_mse", "mse"):
            skip = np.setdiff1d(np.arange(T), cols)
            r[k][:, skip] = g[f"{tag}_{k}"][:, skip]
        r["total_bpd"] = (r["vb"].sum(axis=1, dtype=np.float32) + r["prior_bpd"]).astype(np.float32)
    check_rule_r(r, g, tag, x0[0].size, what=f"{ds} restatement ")


def test_restated_terms_match_the_reference_on_the_designed_grid(golden_bpd):
    g = golden_bpd["ted"]
    cfg = synth.TED
    sch = br.Schedule(1000, "ddim100")
    q_min = float(g["G20k_q_min"].reshape(-1)[0])
    nll_tol = 4 * 2.0 ** -24 / (q_min * LN2)
    for tv in [(t,) * br.B for t in br.GRID_T] + [br.GRID_MIXED]:
        tag = "G20k_t" + ("mixed" if tv == br.GRID_MIXED else str(tv[0]))
        x0, x_t, px, noise = br.grid_inputs(cfg, sch, tv)
        vb, xs, ms, _, q = br.vb_terms(sch, x0, x_t, px, noise, tv)
        rows0 = np.asarray(tv) == 0
        assert br.fragile_count(q[rows0].astype(np.float64)).max() == 0 if rows0.any() else True
        for name, got in (("vb", vb), ("xstart_mse", xs), ("mse", ms)):
            ref, f64 = g[f"{tag}_{name}"].astype(np.float64), g[f"{tag}_{name}_f64"]
            err = np.abs(got.astype(np.float64) - ref)
            rel_bound = (1e-5 + 2 * np.abs(ref - f64) / np.abs(ref)) * np.abs(ref)
            bound = np.where(rows0, nll_tol, rel_bound) if name == "vb" else rel_bound
            print(f"{tag} {name}: {got} worst |err| / bound {float((err / bound).max()):.3f}")
            assert (err <= bound).all(), (tag, name, err, bound)


class _StubEngine:
    """Records what calc_bpd_loop hands to the engine; stands in for libls_hip.so in the draw-order tests."""
    J, F, T, D, batch, n_steps, device = 9, 3, 34, 512, 2, 0, 0

    def __init__(self):
        self.calls = []

    def set_schedule(self, sched):
        self.n_steps = sched.num_timesteps

    def bpd(self, x_start, out, columns=None, noise_tape=None, eps_tape=None, **kw):
        self.calls.append((columns, noise_tape.clone(), eps_tape.clone(), kw))
        for o in out:
            o[:, columns[0]:columns[0] + columns[1]] = 1.0
        return out


@pytest.mark.parametrize("native,segment_bytes", [(True, 256 << 20), (False, 256 << 20), (True, 3 * (2 * 2 * 512 + 2 * 918) * 4)])
def test_torch_cpu_draw_order_and_generator_end_state(monkeypatch, native, segment_bytes):
    """Per column: randn_like(x_start), randn(B, 1, D) of the cond pass, of the uncond pass; nothing else; the generator ends where plain
    torch draws end -- natively or with torch's own calls, in one piece or in three-column segments."""
    inner, diff = create_model_and_diffusion(mk_args(), "ddim10")
    T, B, D = diff.num_timesteps, 2, 512
    eng = _StubEngine()
    model = ClassifierFreeSampleModel(inner)
    monkeypatch.setattr(type(inner), "_engine_prepared", lambda self, y: eng)
    diff.native_host_rng, diff.tape_segment_bytes = native, segment_bytes
    x0 = torch.from_numpy(synth.make_init_image(synth.TED, B))
    torch.manual_seed(4242)
    r = diff.calc_bpd_loop(model, x0, model_kwargs={"y": {}})
    after = torch.randn(5)
    torch.manual_seed(4242)
    want = [(torch.randn_like(x0), torch.randn(B, 1, D), torch.randn(B, 1, D)) for _ in range(T)]
    assert torch.equal(after, torch.randn(5))
    got_nz = torch.cat([c[1] for c in eng.calls])
    got_eps = torch.cat([c[2] for c in eng.calls])
    assert got_nz.shape[0] == T and [c[0] for c in eng.calls] == ([(0, T)] if segment_bytes > 1 << 20 else [(0, 3), (3, 3), (6, 3), (9, 1)])
    for k in range(T):
        assert torch.equal(got_nz[k], want[k][0]) and torch.equal(got_eps[k, 0], want[k][1][:, 0]) and torch.equal(got_eps[k, 1], want[k][2][:, 0])
    assert diff.last_tape_segments == len(eng.calls)
    from livelyspeaker_amd import torch_rng
    assert diff.last_host_rng_native == (native and torch_rng.variant() >= 0)
    assert set(r) == {"total_bpd", "prior_bpd", "vb", "xstart_mse", "mse"} and r["vb"].shape == (B, T)
    assert torch.allclose(r["total_bpd"], torch.full((B,), float(T)) + r["prior_bpd"])


def test_refusals_that_need_no_engine():
    model, diff = create_model_and_diffusion(mk_args(), "ddim10")
    cfgm = ClassifierFreeSampleModel(model)
    x0 = torch.from_numpy(synth.make_init_image(synth.TED, 2))
    y = {k: torch.from_numpy(v) for k, v in synth.make_cond(synth.TED, 2).items()}
    inp = dict(y, inpainting_mask=torch.zeros(2, 9, 3, 34, dtype=torch.bool), inpainted_motion=torch.zeros(2, 9, 3, 34))
    with pytest.raises(NotImplementedError, match="inpainting"):
        diff.calc_bpd_loop(cfgm, x0, model_kwargs={"y": inp})
    with pytest.raises(NotImplementedError, match="inpainting"):
        diff._vb_terms_bpd(cfgm, x0, x0, torch.zeros(2, dtype=torch.long), model_kwargs={"y": inp})
    diff.noise_source = "torch_device"
    with pytest.raises(NotImplementedError, match="torch_device"):
        diff.calc_bpd_loop(cfgm, x0, model_kwargs={"y": y})
    diff.noise_source = "nonsense"
    with pytest.raises(ValueError, match="noise_source"):
        diff.calc_bpd_loop(cfgm, x0, model_kwargs={"y": y})


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-GPU failure mode")
def test_calc_bpd_loop_without_a_gpu_fails_loudly():
    model, diff = create_model_and_diffusion(mk_args(), "ddim10")
    cfgm = ClassifierFreeSampleModel(model)
    y = {k: torch.from_numpy(v) for k, v in synth.make_cond(synth.TED, 2).items()}
    with pytest.raises(_lib.EngineError):
        diff.calc_bpd_loop(cfgm, torch.from_numpy(synth.make_init_image(synth.TED, 2)), model_kwargs={"y": y})


def test_abi_mirrors_of_the_bpd_arguments(tmp_path):
    """LsBpdArgs / LsVbTermsArgs against what a C compiler makes of include/ls_hip.h; the ABI version stays 5."""
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ls_hip.h"\nint main(void) {\n'
                   '    printf("%zu %zu %zu %zu %zu %zu %d\\n", sizeof(ls_bpd_args), offsetof(ls_bpd_args, x_start), offsetof(ls_bpd_args, mse),\n'
                   '           sizeof(ls_vb_terms_args), offsetof(ls_vb_terms_args, indices), offsetof(ls_vb_terms_args, pred_out), LS_ABI_VERSION);\n'
                   '    return 0;\n}\n')
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    A, V = _lib.LsBpdArgs, _lib.LsVbTermsArgs
    assert got == [ctypes.sizeof(A), A.x_start.offset, A.mse.offset, ctypes.sizeof(V), V.indices.offset, V.pred_out.offset, 5]
    assert {"ls_bpd", "ls_vb_terms"} <= set(_lib.EXPORTS)
    assert gd.GaussianDiffusion.calc_bpd_loop.__doc__
