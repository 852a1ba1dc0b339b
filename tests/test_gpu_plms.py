"""The PLMS sampler (plms_sample / plms_sample_loop / plms_sample_loop_progressive, gaussian_diffusion.py:1016-1211) and the DDIM reverse
step (ddim_reverse_sample, :857-893) on the GPU: against the reference's own outputs (fixtures G17 / G18, tests/golden/make_golden_plms.py)
through the Python API, on every kernel family, graph replay against plain launches, the three noise sources, multi-piece plans and a
long-sequence model against the CPU restatement (tests/plms_restatement.py, itself pinned to the fixtures by tests/test_plms_host.py)."""
import os

import numpy as np
import pytest

import plms_restatement as pr
from conftest import GOLDEN, max_abs
from livelyspeaker_amd import synth
from test_gpu_boundary import _wrapped
from test_gpu_coop import _engine as _engine_on
from test_gpu_sampler_surface import _Tape

pytestmark = pytest.mark.gpu
TOL, TOL_LOOP = 2e-4, 3e-4          # single results / every yield of a loop (tests/test_gpu_sampler_surface.py)
DEV = "cuda:0"


def eps_tol(sch, t):
    return pr.eps_tol(sch, t, TOL)


def _golden(ds):
    return np.load(os.path.join(GOLDEN, f"{ds}_golden_plms.npz"))


def _draws(x_init, eps):
    return [x_init] + [eps[e, p][:, None, :] for e in range(len(eps)) for p in range(2)]


def _cond(cfg, B, **kw):
    import torch
    return {k: torch.from_numpy(v).to(DEV) for k, v in synth.make_cond(cfg, B, **kw).items()}


def _oracle(cfg):
    return pr.RagOracle(synth.make_state_dict(cfg), cfg.njoints, cfg.nfeats, cfg.n_prefix_tokens, nframes=cfg.nframes)


@pytest.mark.parametrize("ds", ["ted", "beat"])
def test_plms_loops_vs_reference_and_bitwise_the_whole_loop(ds):
    import torch
    g = _golden(ds)
    for tag, (steps, resp, skip, use_init, clip, order, keep) in pr.LOOPS[ds].items():
        cfg, model, diffusion = _wrapped(ds, resp, steps)
        n_exec = diffusion.num_timesteps - skip
        x_init, eps = pr.loop_tape(cfg, n_exec + 1)
        y = _cond(cfg, pr.B)
        init = torch.from_numpy(synth.make_init_image(cfg, pr.B)).to(DEV) if use_init else None
        kw = dict(clip_denoised=clip, model_kwargs={"y": y}, skip_timesteps=skip, init_image=init, progress=False, order=order)
        with _Tape(_draws(x_init, eps)) as tp:
            outs = []
            for r in diffusion.plms_sample_loop_progressive(model, x_init.shape, **kw):
                assert set(r) == {"sample", "pred_xstart", "old_eps"} and isinstance(r["old_eps"], list)
                assert all(e.device == r["sample"].device for e in r["old_eps"])
                outs.append((r["sample"].cpu().numpy(), r["pred_xstart"].cpu().numpy(), len(r["old_eps"])))
        assert tp.i == 1 + 2 * (n_exec + 1) == len(tp.draws) and len(outs) == n_exec
        assert [o[2] for o in outs] == [min(k + 1, order - 1) for k in range(n_exec)]       # the history carried forward (:1092-1093)
        ks = pr.kept(n_exec, keep)
        assert list(g[f"{tag}_yields"]) == ks
        for j, k in enumerate(ks):
            d = max_abs(outs[k][0], g[f"{tag}_samples"][j])
            dx = max_abs(outs[k][1], g[f"{tag}_x0"][j]) if ds == "ted" else (max_abs(outs[0][1], g["G17_first_x0"]) if k == 0 else 0.0)
            print(f"{ds} {tag} yield {k}: sample {d:.2e} pred_xstart {dx:.2e}")
            assert d < TOL_LOOP and dx < TOL_LOOP, (tag, k, d, dx)
        assert np.array_equal(outs[-1][0], outs[-1][1])                                     # t = 0: the sample IS pred_xstart
        if clip:
            assert max(float(np.abs(o[1]).max()) for o in outs) <= 1.0
        with _Tape(_draws(x_init, eps)) as tp:
            whole = diffusion.plms_sample_loop(model, x_init.shape, **kw)
        assert tp.i == len(tp.draws)
        assert np.array_equal(whole.cpu().numpy(), outs[-1][0]), tag                        # the same launches: bitwise the last yield
        model.model.engine().close()


@pytest.mark.parametrize("on_gpu", [True, False])
def test_plms_single_steps_with_a_given_history_vs_reference(on_gpu):
    """sample and pred_xstart against G17 at the plain 2e-4.  The returned list's last entry (the step's eps plane) is held to the same
    2e-4 in the units of the x0 it is derived from (plms_restatement.eps_tol): at t = 50 that IS 2e-4 (measured 7.6e-6); at t = 0 of
    ddim100 eps = (x - x0) / 0.0064, values up to 1.2e3 with an fp32 ulp of 6e-5 -- measured 1.07e-3 on MI355X and 8.5e-4 for the CPU
    restatement against the reference (x0 itself: 6.8e-6), bound 3.1e-2.  A plain 2e-4 there would ask x0 to 1.3e-6, below what two
    fp32 evaluations of the network in different summation orders agree to."""
    import torch
    g = _golden("ted")
    dev = DEV if on_gpu else "cpu"
    for resp in ("ddim100",):
        cfg, model, diffusion = _wrapped("ted", resp, 1000)
        sch = pr.Schedule(1000, resp)
        x, hist, eps = pr.step_inputs(cfg)
        y = {k: v.to(dev) for k, v in _cond(cfg, pr.B).items()}
        for tag, (resp_t, t, order, nh) in pr.STEPS.items():
            assert resp_t == resp
            given = [torch.from_numpy(h).to(dev) for h in hist[3 - nh:]]
            with _Tape([eps[0][:, None, :], eps[1][:, None, :]]) as tp:
                r = diffusion.plms_sample(model, torch.from_numpy(x).to(dev), torch.full((pr.B,), t, dtype=torch.long).to(dev), clip_denoised=False,
                                          model_kwargs={"y": y}, order=order, old_out={"old_eps": given})
            assert tp.i == 2
            ds_, dx = max_abs(r["sample"].cpu().numpy(), g[f"{tag}_sample"]), max_abs(r["pred_xstart"].cpu().numpy(), g[f"{tag}_x0"])
            de = max_abs(r["old_eps"][-1].cpu().numpy(), g[f"{tag}_last_eps"])
            print(f"{tag} [{dev}]: sample {ds_:.2e} pred_xstart {dx:.2e} last eps {de:.2e} (bound {eps_tol(sch, t):.2e})")
            assert ds_ < TOL and dx < TOL and de < eps_tol(sch, t)
            assert len(r["old_eps"]) == int(g[f"{tag}_len"].item()) and r["old_eps"] is given      # the caller's list, as in the reference
            assert str(r["old_eps"][-1].device) == str(r["sample"].device)
            if t == 0:
                assert torch.equal(r["sample"], r["pred_xstart"])
        model.model.engine().close()


@pytest.mark.parametrize("ds", ["ted", "beat"])
def test_ddim_reverse_sample_vs_reference(ds):
    import torch
    g = _golden(ds)
    for tag, (resp, t) in pr.REVERSE[ds].items():
        cfg, model, diffusion = _wrapped(ds, resp, 1000)
        x, _, eps = pr.step_inputs(cfg)
        with _Tape([eps[0][:, None, :], eps[1][:, None, :]]) as tp:
            r = diffusion.ddim_reverse_sample(model, torch.from_numpy(x).to(DEV), torch.full((pr.B,), t, dtype=torch.long).to(DEV),
                                              clip_denoised=False, model_kwargs={"y": _cond(cfg, pr.B)})
        assert tp.i == 2 and set(r) == {"sample", "pred_xstart"}
        d = max_abs(r["sample"].cpu().numpy(), g[f"{tag}_sample"])
        dx = max_abs(r["pred_xstart"].cpu().numpy(), g[f"{tag}_x0"]) if ds == "ted" else 0.0
        print(f"{ds} {tag}: sample {d:.2e} pred_xstart {dx:.2e}")
        assert d < TOL and dx < TOL
        model.model.engine().close()


def test_ddim_reverse_sample_per_sample_t_and_the_last_table_entry():
    import torch
    cfg, model, diffusion = _wrapped("ted", "ddim100", 1000)
    oracle, sch = _oracle(cfg), pr.Schedule(1000, "ddim100")
    x, _, eps = pr.step_inputs(cfg)
    t = np.array([0, 37, 98, 99])
    with _Tape([eps[0][:, None, :], eps[1][:, None, :]]):
        r = diffusion.ddim_reverse_sample(model, torch.from_numpy(x).to(DEV), torch.from_numpy(t).to(DEV), clip_denoised=True,
                                          model_kwargs={"y": _cond(cfg, pr.B)})
    want, want0 = pr.ddim_reverse_step(oracle, sch, synth.make_cond(cfg, pr.B), x, t, eps, clip_denoised=True)
    d, dx = max_abs(r["sample"].cpu().numpy(), want), max_abs(r["pred_xstart"].cpu().numpy(), want0)
    print(f"ddim_reverse_sample, t = {t.tolist()}: sample {d:.2e} pred_xstart {dx:.2e}")
    assert d < TOL and dx < TOL and float(r["pred_xstart"].abs().max()) <= 1.0
    model.model.engine().close()
    # alpha_bar_next = 0 at the last entry of the unspaced tables: the sample is eps itself -- the table shift and the sign conventions
    cfg, model, diffusion = _wrapped("ted", "", 1000)
    with _Tape([eps[0][:, None, :], eps[1][:, None, :]]):
        r = diffusion.ddim_reverse_sample(model, torch.from_numpy(x).to(DEV), torch.full((pr.B,), 999, dtype=torch.long).to(DEV),
                                          clip_denoised=False, model_kwargs={"y": _cond(cfg, pr.B)})
    sch = pr.Schedule(1000, "")
    x0 = r["pred_xstart"].cpu().numpy()
    eps_host = (sch.f32("sqrt_recip_alphas_cumprod", 999) * x - x0) / sch.f32("sqrt_recipm1_alphas_cumprod", 999)
    d = max_abs(r["sample"].cpu().numpy(), eps_host)
    print(f"ddim_reverse_sample at t = 999 (alpha_bar_next = 0): |sample - eps| {d:.2e}")
    assert d < TOL
    model.model.engine().close()


FAMILIES = [("fused", 0), ("batch", 1), ("coop", 2), ("coop8", 2), ("coop4", 2), ("coop2", 2), ("pass", 3), ("pass4", 3)]


@pytest.mark.parametrize("path,family", FAMILIES)
@pytest.mark.parametrize("ds", ["ted", "beat"])
def test_order4_fixture_loop_on_every_kernel_family(ds, path, family):
    from livelyspeaker_amd import _lib
    g = _golden(ds)
    steps, resp, skip, _, clip, order, _ = pr.LOOPS[ds]["G17_o4"]
    cfg, eng = _engine_on(ds, path)
    try:
        sch = pr.Schedule(steps, resp)
        n_exec = sch.num_timesteps - skip
        x_init, eps = pr.loop_tape(cfg, n_exec + 1)
        eng.set_schedule(sch)
        eng.prepare(synth.make_cond(cfg, pr.B))
        kw = dict(sampler=_lib.LS_SAMPLER_PLMS, plms_order=order, x_init=x_init, eps_tape=eps, skip_timesteps=skip,
                  init_image=synth.make_init_image(cfg, pr.B), clip_denoised=clip)
        got = eng.sample(**kw)
        tm = eng.timing()
        assert tm["step_path"] == family and tm["n_step_launches"] == n_exec + 1 and tm["graph_replayed"] == 0
        d = max_abs(got, g["G17_o4_samples"][-1])
        print(f"{ds} [{path}]: PLMS order 4, {n_exec} steps: max|hip - reference| = {d:.2e}")
        assert d < TOL_LOOP
        again = eng.sample(**kw)
        assert eng.timing()["graph_replayed"] == 1 and np.array_equal(got, again)
        assert np.array_equal(got, eng.sample(use_graph=False, **kw))                  # graph replay == plain launches
    finally:
        eng.close()


def test_graph_replay_plain_launches_and_a_change_of_order():
    import torch
    cfg, model, diffusion = _wrapped("ted", "ddim100", 1000)
    oracle, sch = _oracle(cfg), pr.Schedule(1000, "ddim100")
    skip, n_exec = 88, 12
    x_init, eps = pr.loop_tape(cfg, n_exec + 1, seed=99)
    yh = synth.make_cond(cfg, pr.B)
    y = _cond(cfg, pr.B)
    init = synth.make_init_image(cfg, pr.B)
    eng = model.model.engine()

    def run(order, graph=True):
        diffusion.use_graph = graph
        with _Tape(_draws(x_init, eps)):
            return diffusion.plms_sample_loop(model, x_init.shape, clip_denoised=False, model_kwargs={"y": y}, skip_timesteps=skip,
                                              init_image=torch.from_numpy(init).to(DEV), order=order).cpu().numpy()

    a = run(2)
    assert eng.timing()["graph_replayed"] == 0
    b = run(2)
    assert eng.timing()["graph_replayed"] == 1 and np.array_equal(a, b)
    c = run(3)                                       # another order: the graph of order 2 must not be replayed
    assert eng.timing()["graph_replayed"] == 0 and max_abs(a, c) > 1e-2
    assert np.array_equal(a, run(2, graph=False)) and np.array_equal(c, run(3, graph=False))
    for order, got in ((2, a), (3, c)):
        want = pr.plms_loop(oracle, sch, yh, x_init, eps, order, skip_timesteps=skip, init_image=init)
        d = max_abs(got, want)
        print(f"order {order}: max|hip - restatement| = {d:.2e}")
        assert d < TOL_LOOP
    eng.close()


@pytest.mark.parametrize("ds,B", [("ted", 72), ("beat", 88)])
def test_multi_piece_plans_replayed_through_the_restatement(ds, B):
    """Philox, order 3, 20 executed steps (ddim100, skip_timesteps 80) on batches that `auto` runs in several launches or pieces per
    evaluation: the first and the last sample of every piece of its plan, replayed alone on the restated Philox draws (evaluation e uses step_id e: oracle/philox_oracle.step_tapes over n_exec + 1)."""
    from livelyspeaker_amd import _lib
    from oracle import philox_oracle as po
    cfg = synth.CONFIGS[ds]
    eng = _lib.Engine(cfg.njoints, cfg.nfeats, cfg.n_prefix_tokens, cfg.audio_len, n_emotions=cfg.n_emotions, path="auto")
    eng.load_state_dict(synth.make_state_dict(cfg))
    oracle = _oracle(cfg)
    try:
        seed, off, skip, order = 4242 + B, 1000, 80, 3
        y = synth.make_cond(cfg, B, scale=1.5)
        sch = pr.Schedule(1000, "ddim100")
        n_exec = sch.num_timesteps - skip
        eng.set_schedule(sch)
        eng.prepare(y)
        got = eng.sample(sampler=_lib.LS_SAMPLER_PLMS, plms_order=order, philox_seed=seed, sample_offset=off, skip_timesteps=skip)
        assert np.isfinite(got).all()
        tm = eng.timing()
        pieces, _ = _lib.plan_query(B, dataset=ds, n_cus=tm["n_cus"])
        assert sum(n for _, _, n in pieces) == B          # (on 256 CUs: one sample-split piece of several launches per evaluation)
        assert tm["step_path"] == pieces[0][0] and tm["tail_samples"] == (pieces[1][2] if len(pieces) > 1 else 0)     # the plan that ran
        pick = np.array(sorted({i for _, first, n in pieces for i in (first, first + n - 1)}))
        eps, _ = po.step_tapes(seed, off + pick, n_exec + 1, (cfg.njoints, cfg.nfeats, cfg.nframes))
        x_T = po.x_init(seed, off + pick, cfg.njoints * cfg.nfeats, cfg.nframes, (cfg.njoints, cfg.nfeats))
        want = pr.plms_loop(oracle, sch, {k: v[pick] for k, v in y.items()}, x_T, eps, order, skip_timesteps=skip)
        per = np.abs(got[pick].astype(np.float64) - want).reshape(len(pick), -1).max(axis=1)
        print(f"{ds} B={B}: plan {pieces}; samples {pick.tolist()}: max|hip - restatement| per sample {[float(f'{v:.2e}') for v in per]}")
        assert per.max() < TOL_LOOP
    finally:
        eng.close()


def test_philox_loop_is_shard_invariant():
    import torch
    cfg, model, diffusion = _wrapped("ted", "ddim100", 1000)
    B = 8
    yh = synth.make_cond(cfg, B)
    diffusion.noise_source, diffusion.philox_seed = "philox", 20260101
    shape = (B, cfg.njoints, cfg.nfeats, cfg.nframes)
    init = torch.from_numpy(synth.make_init_image(cfg, B)).to(DEV)
    alive = []      # the model keys its resident conditioning by the tensors' addresses: every shard's tensors stay allocated

    def run(first, count):
        diffusion.sample_offset = first
        y = {k: torch.from_numpy(v[first:first + count].copy()).to(DEV) for k, v in yh.items()}
        alive.append(y)
        out = diffusion.plms_sample_loop(model, (count,) + shape[1:], clip_denoised=False, model_kwargs={"y": y}, skip_timesteps=85,
                                         init_image=init[first:first + count], order=4)
        assert diffusion.last_philox_seed == 20260101
        return out.cpu().numpy()

    whole = run(0, B)
    halves = np.concatenate([run(0, B // 2), run(B // 2, B // 2)])
    assert np.isfinite(whole).all() and np.array_equal(whole, halves)
    assert not np.array_equal(whole[:B // 2], whole[B // 2:])
    model.model.engine().close()


def test_torch_device_loop_is_the_tape_loop_fed_torchs_own_device_draws():
    import torch
    from test_gpu_torch_device_rng import _seed
    cfg, model, diffusion = _wrapped("ted", "ddim100", 1000)
    B, skip, order = pr.B, 90, 3
    n_exec = diffusion.num_timesteps - skip
    shape = (B, cfg.njoints, cfg.nfeats, cfg.nframes)
    y = _cond(cfg, B)
    init = torch.from_numpy(synth.make_init_image(cfg, B)).to(DEV)
    kw = dict(clip_denoised=False, model_kwargs={"y": y}, skip_timesteps=skip, init_image=init, order=order)
    cpu_state = torch.get_rng_state()
    gen = _seed(2468, 8)
    diffusion.noise_source = "torch_device"
    got = diffusion.plms_sample_loop(model, shape, **kw).cpu().numpy()
    off_loop = gen.get_offset()
    assert torch.equal(cpu_state, torch.get_rng_state())                # the CPU generator is not touched
    gen = _seed(2468, 8)                                                # the reference's draws, made with plain torch calls on the device
    draws = [torch.randn(*shape, device=DEV)]
    for _ in range(n_exec + 1):
        draws += [torch.randn(B, 1, 512, device=DEV), torch.randn(B, 1, 512, device=DEV)]
    off_ref = gen.get_offset()
    assert off_loop == off_ref and len(draws) == 1 + 2 * (n_exec + 1)
    diffusion.noise_source = "torch_cpu"
    with _Tape([d.cpu().numpy() for d in draws]) as tp:
        want = diffusion.plms_sample_loop(model, shape, **kw).cpu().numpy()
    assert tp.i == len(tp.draws) and np.array_equal(got, want)
    model.model.engine().close()


def test_torch_cpu_loop_follows_torch_manual_seed():
    import torch
    cfg, model, diffusion = _wrapped("ted", "ddim100", 1000)
    oracle, sch = _oracle(cfg), pr.Schedule(1000, "ddim100")
    B, skip, order = pr.B, 90, 4
    n_exec = sch.num_timesteps - skip
    shape = (B, cfg.njoints, cfg.nfeats, cfg.nframes)
    init = synth.make_init_image(cfg, B)
    torch.manual_seed(1357)
    got = diffusion.plms_sample_loop(model, shape, clip_denoised=False, model_kwargs={"y": _cond(cfg, B)}, skip_timesteps=skip,
                                     init_image=torch.from_numpy(init).to(DEV), order=order).cpu().numpy()
    state_loop = torch.get_rng_state()
    torch.manual_seed(1357)
    x_T = torch.randn(*shape).numpy()
    eps = np.stack([np.stack([torch.randn(B, 1, 512)[:, 0].numpy() for _ in range(2)]) for _ in range(n_exec + 1)])
    assert torch.equal(state_loop, torch.get_rng_state())               # the generator ends where the reference's draws leave it
    want = pr.plms_loop(oracle, sch, synth.make_cond(cfg, B), x_T, eps, order, skip_timesteps=skip, init_image=init)
    d = max_abs(got, want)
    print(f"torch_cpu PLMS order {order}, {n_exec} steps from torch.manual_seed: max|hip - restatement| = {d:.2e}")
    assert d < TOL_LOOP
    with pytest.raises(ValueError, match=r"\b%d\b.*\b1024\b" % ((n_exec + 1) * 2 * B * 512 * 4)):
        diffusion.tape_segment_bytes = 1024
        diffusion.plms_sample_loop(model, shape, model_kwargs={"y": _cond(cfg, B)}, skip_timesteps=skip, order=order)
    model.model.engine().close()


def test_long_sequence_model_self_pinned():
    """SELF-PINNED: the reference cannot run 150 frames; the restatement on this repository's oracle is the only yardstick."""
    from livelyspeaker_amd import _lib
    cfg = synth.BEAT150
    eng = _lib.Engine(cfg.njoints, cfg.nfeats, cfg.n_prefix_tokens, cfg.audio_len, n_emotions=cfg.n_emotions, nframes=cfg.nframes)
    eng.load_state_dict(synth.make_state_dict(cfg))
    try:
        B, skip, order = 8, 94, 2
        sch = pr.Schedule(1000, "ddim100")
        n_exec = sch.num_timesteps - skip
        y = synth.make_cond(cfg, B)
        x_init, eps = pr.loop_tape(cfg, n_exec + 1, seed=150, batch=B)
        init = synth.make_init_image(cfg, B)
        eng.set_schedule(sch)
        eng.prepare(y)
        kw = dict(sampler=_lib.LS_SAMPLER_PLMS, plms_order=order, x_init=x_init, eps_tape=eps, skip_timesteps=skip, init_image=init)
        got = eng.sample(**kw)
        assert eng.timing()["step_path"] == 1
        want = pr.plms_loop(_oracle(cfg), sch, y, x_init, eps, order, skip_timesteps=skip, init_image=init)
        d = max_abs(got, want)
        print(f"150 frames, B = {B}, PLMS order {order}, {n_exec} steps: max|hip - restatement| = {d:.2e}")
        assert d < TOL_LOOP
        assert np.array_equal(got, eng.sample(use_graph=False, **kw))
    finally:
        eng.close()


def test_engine_refuses_what_plms_does_not_take():
    from livelyspeaker_amd import _lib
    cfg, eng = _engine_on("ted", "fused")
    try:
        eng.set_schedule(pr.Schedule(1000, "ddim100"))
        eng.prepare(synth.make_cond(cfg, 2))
        x_init, eps = pr.loop_tape(cfg, 13, batch=2)
        base = dict(sampler=_lib.LS_SAMPLER_PLMS, x_init=x_init, eps_tape=eps, skip_timesteps=88)
        for bad in (dict(plms_order=1), dict(plms_order=5), dict(plms_order=2, skip_timesteps=99, eps_tape=eps[:2]), dict(plms_order=2, const_noise=True),
                    dict(plms_order=2, eta=0.5)):
            with pytest.raises(_lib.EngineError):
                eng.sample(**dict(base, **bad))
        with pytest.raises(_lib.EngineError):
            eng.sample(sampler=_lib.LS_SAMPLER_DDIM_REVERSE, x_init=x_init, eps_tape=eps[:12], noise_tape=np.zeros((12,) + x_init.shape, np.float32),
                       skip_timesteps=88)
        assert np.isfinite(eng.sample(plms_order=2, **base)).all()          # and the handle is still good
    finally:
        eng.close()
