"""The variational bound in bits per dimension on the GPU (calc_bpd_loop / _vb_terms_bpd, gaussian_diffusion.py:1591-1646 / :1213-1246; ls_bpd,
ls_vb_terms, csrc/ls_bpd.hip): the reduction kernel against the reference's element functions on a designed grid (fixture G20k), the
loop against the reference's own loops (G20) through the Python API and on every kernel family, graph replay against plain launches and
column segments, the noise sources, multi-piece plans and a long-sequence model against the CPU restatement (tests/bpd_restatement.py,
itself pinned to the fixtures by tests/test_bpd_host.py).  Tolerances: rule R of bpd_restatement.rule_r, the kernel-level bounds below."""
import os

import numpy as np
import pytest

import bpd_restatement as br
from conftest import GOLDEN
from livelyspeaker_amd import synth
from test_bpd_host import check_rule_r, x_start_of
from test_gpu_boundary import _wrapped
from test_gpu_coop import _engine as _engine_on
from test_gpu_plms import FAMILIES
from test_gpu_sampler_surface import _Tape

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LN2 = np.log(2.0)


def _golden(ds):
    return np.load(os.path.join(GOLDEN, f"{ds}_golden_bpd.npz"))


def _draws(nz, eps):
    return [a for k in range(len(nz)) for a in (nz[k], eps[k, 0][:, None, :], eps[k, 1][:, None, :])]


def _cond(cfg, B, **kw):
    import torch
    return {k: torch.from_numpy(v).to(DEV) for k, v in synth.make_cond(cfg, B, **kw).items()}


def _oracle(cfg):
    return br.RagOracle(synth.make_state_dict(cfg), cfg.njoints, cfg.nfeats, cfg.n_prefix_tokens, nframes=cfg.nframes)


def _np(r):
    return {k: v.detach().cpu().numpy() for k, v in r.items()}


def _outs(B, T):
    return tuple(np.full((B, T), np.nan, np.float32) for _ in range(3))


def _check_against_restatement(got, ref, f64, cols, n_elem, what):
    """Rule R on the columns `cols` of (vb, xstart_mse, mse) against a restatement run (fp32 `ref`, float64 `f64` of the same run)."""
    xs_ref = ref["xstart_mse"][:, cols]
    for j, k in enumerate(("vb", "xstart_mse", "mse")):
        bound = br.rule_r(ref[k][:, cols], f64[k][:, cols], xs_ref, f64.get("n_frag") if (k == "vb" and cols[-1] == ref[k].shape[1] - 1) else None, n_elem)
        err = np.abs(got[j][:, cols].astype(np.float64) - ref[k][:, cols])
        print(f"{what} {k}: worst |err| / bound {float((err / bound).max()):.3f} (max rel err {float((err / np.abs(ref[k][:, cols])).max()):.2e})")
        assert (err <= bound).all(), (what, k)


# ------------------------------------------------------------------------------------------------ the kernel alone
def test_vb_terms_kernel_vs_the_reference_grid():
    """KL columns and both MSEs: relative 1e-5 + 2 |ref - ref_f64| / |ref|.  NLL rows: absolute 4 * 2^-24 / (q_min ln 2) bits -- four
    ulps of 1.0 in q, divided by the smallest unclamped q of the grid (no fragile element: asserted by the generator)."""
    import torch
    g = _golden("ted")
    cfg, eng = _engine_on("ted", "fused")
    try:
        sch = br.Schedule(1000, "ddim100")
        eng.set_schedule(sch)
        eng.prepare(synth.make_cond(cfg, br.B))
        nll_tol = 4 * 2.0 ** -24 / (float(g["G20k_q_min"].reshape(-1)[0]) * LN2)
        for tv in [(t,) * br.B for t in br.GRID_T] + [br.GRID_MIXED]:
            mixed = tv == br.GRID_MIXED
            tag = "G20k_t" + ("mixed" if mixed else str(tv[0]))
            x0, x_t, px, noise = br.grid_inputs(cfg, sch, tv)
            kw = dict(indices=np.asarray(tv, dtype=np.int64)) if mixed else dict(index=tv[0])
            vb, xs, ms, pred = eng.vb_terms(x0, x_t, px, noise, **kw)
            assert np.array_equal(pred, px)
            rows0 = np.asarray(tv) == 0
            for name, got in (("vb", vb), ("xstart_mse", xs), ("mse", ms)):
                ref, f64 = g[f"{tag}_{name}"].astype(np.float64), g[f"{tag}_{name}_f64"]
                err = np.abs(got.astype(np.float64) - ref)
                rel_bound = (1e-5 + 2 * np.abs(ref - f64) / np.abs(ref)) * np.abs(ref)
                bound = np.where(rows0, nll_tol, rel_bound) if name == "vb" else rel_bound
                print(f"{tag} {name}: got {got} |err| {err} bound {bound}")
                assert (err <= bound).all(), (tag, name)
            if mixed:
                # row b of the mixed vector == row b of the uniform call at t_b on the same planes, bitwise; device indices == host indices
                for b, t in enumerate(tv):
                    u = eng.vb_terms(x0, x_t, px, noise, index=int(t))
                    assert all(np.array_equal(u[j][b], (vb, xs, ms)[j][b]) for j in range(3)), (b, t)
                dv = eng.vb_terms(*(torch.from_numpy(a).to(DEV) for a in (x0, x_t, px, noise)), indices=torch.tensor(tv, device=DEV))
                assert all(np.array_equal(dv[j].cpu().numpy(), (vb, xs, ms)[j]) for j in range(3))
                # without noise: no mse, the same vb; clip_denoised: the clamped plane comes back and is what the terms are computed from
                nn = eng.vb_terms(x0, x_t, px, None, **kw)
                assert nn[2] is None and np.array_equal(nn[0], vb) and np.array_equal(nn[1], xs)
                cl = eng.vb_terms(x0, x_t, px, noise, clip_denoised=True, **kw)
                assert np.array_equal(cl[3], np.clip(px, -1, 1))
                un = eng.vb_terms(x0, x_t, np.clip(px, -1, 1), noise, **kw)
                assert all(np.array_equal(cl[j], un[j]) for j in range(3))
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------ the loop against the reference
@pytest.mark.parametrize("ds,tag", [(ds, tag) for ds in ("ted", "beat") for tag in br.LOOPS[ds]])
def test_calc_bpd_loop_vs_reference(ds, tag):
    g = _golden(ds)
    steps, resp, clip = br.LOOPS[ds][tag]
    cfg, model, diffusion = _wrapped(ds, resp, steps)
    import torch
    T = diffusion.num_timesteps
    nz, eps = br.loop_tape(cfg, T)
    x0 = torch.from_numpy(x_start_of(ds)).to(DEV)
    with _Tape(_draws(nz, eps)) as tp:
        r = diffusion.calc_bpd_loop(model, x0, clip_denoised=clip, model_kwargs={"y": _cond(cfg, br.B)})
    assert tp.i == 3 * T == len(tp.draws)
    assert set(r) == {"total_bpd", "prior_bpd", "vb", "xstart_mse", "mse"} and all(v.device == x0.device for v in r.values())
    assert r["vb"].shape == r["xstart_mse"].shape == r["mse"].shape == (br.B, T) and r["total_bpd"].shape == r["prior_bpd"].shape == (br.B,)
    tm = model.model.engine().timing()
    assert tm["n_step_launches"] == T
    check_rule_r(_np(r), g, tag, x0[0].numel(), what=f"{ds} hip ")
    model.model.engine().close()


def test_vb_terms_bpd_single_columns_vs_the_loop_fixture():
    import torch
    from livelyspeaker_amd.gaussian_diffusion import _ref_strides
    g = _golden("ted")
    tag = "G20_ddim100"
    steps, resp, clip = br.LOOPS["ted"][tag]
    cfg, model, diffusion = _wrapped("ted", resp, steps)
    T = diffusion.num_timesteps
    nz, eps = br.loop_tape(cfg, T)
    x0h = x_start_of("ted")
    x0 = torch.from_numpy(x0h).to(DEV)
    y = _cond(cfg, br.B)
    bound = br.rule_r(g[f"{tag}_vb"], g[f"{tag}_vb_f64"], g[f"{tag}_xstart_mse"], g[f"{tag}_n_frag"], x0h[0].size)
    for t in (50, 0):
        k = T - 1 - t
        tt = torch.full((br.B,), t, dtype=torch.long, device=DEV)
        x_t = diffusion.q_sample(x0, tt, torch.from_numpy(nz[k]).to(DEV))
        with _Tape([eps[k, 0][:, None, :], eps[k, 1][:, None, :]]) as tp:
            r = diffusion._vb_terms_bpd(model, x0, x_t, tt, clip_denoised=clip, model_kwargs={"y": y})
        assert tp.i == 2 and set(r) == {"output", "pred_xstart"} and r["output"].shape == (br.B,)
        assert r["pred_xstart"].stride() == _ref_strides(torch.empty(x0.shape)).stride()
        err = np.abs(r["output"].cpu().numpy().astype(np.float64) - g[f"{tag}_vb"][:, k])
        print(f"_vb_terms_bpd t = {t}: {r['output'].cpu().numpy()} |err| / bound {err / bound[:, k]}")
        assert (err <= bound[:, k]).all()
    model.model.engine().close()


def test_graph_replay_plain_launches_segments_and_a_flipped_clip():
    import torch
    cfg, model, diffusion = _wrapped("ted", "ddim100", 1000)
    eng = model.model.engine()
    x0 = torch.from_numpy(x_start_of("ted")).to(DEV)
    y = _cond(cfg, br.B)

    def run(clip=True, graph=True, seg=256 << 20):
        diffusion.use_graph, diffusion.tape_segment_bytes = graph, seg
        torch.manual_seed(8642)
        return _np(diffusion.calc_bpd_loop(model, x0, clip_denoised=clip, model_kwargs={"y": y}))

    same = lambda a, b: all(np.array_equal(a[k], b[k]) for k in a)      # noqa: E731
    a = run()
    assert eng.timing()["graph_replayed"] == 0 and diffusion.last_tape_segments == 1
    b = run()
    assert eng.timing()["graph_replayed"] == 1 and same(a, b)
    c = run(clip=False)                                 # the graph of clip_denoised=True must not be replayed
    assert eng.timing()["graph_replayed"] == 0 and not np.array_equal(a["vb"], c["vb"])
    assert same(a, run(graph=False)) and same(c, run(clip=False, graph=False))
    per_col = (2 * br.B * 512 + x0.numel()) * 4
    d = run(seg=per_col * 60)                           # two column segments: 60 + 40
    assert diffusion.last_tape_segments == 2 and same(a, d)
    eng.close()


@pytest.mark.parametrize("path,family", FAMILIES)
@pytest.mark.parametrize("ds", ["ted", "beat"])
def test_ddim100_loop_on_every_kernel_family(ds, path, family):
    g = _golden(ds)
    tag = "G20_ddim100" + ("_clip" if ds == "ted" else "")
    steps, resp, clip = br.LOOPS[ds][tag]
    cfg, eng = _engine_on(ds, path)
    try:
        sch = br.Schedule(steps, resp)
        T = sch.num_timesteps
        nz, eps = br.loop_tape(cfg, T)
        x0 = x_start_of(ds)
        eng.set_schedule(sch)
        eng.prepare(synth.make_cond(cfg, br.B))
        vb, xs, ms = eng.bpd(x0, _outs(br.B, T), noise_tape=nz, eps_tape=eps, clip_denoised=clip)
        tm = eng.timing()
        assert tm["step_path"] == family and tm["n_step_launches"] == T and tm["graph_replayed"] == 0
        prior = br.prior_bpd(sch, x0)
        check_rule_r({"vb": vb, "xstart_mse": xs, "mse": ms, "prior_bpd": prior, "total_bpd": vb.sum(axis=1) + prior}, g, tag, x0[0].size,
                     what=f"{ds} [{path}] ")
        again = eng.bpd(x0, _outs(br.B, T), noise_tape=nz, eps_tape=eps, clip_denoised=clip)
        assert eng.timing()["graph_replayed"] == 1 and all(np.array_equal(p, q) for p, q in zip((vb, xs, ms), again))
        sub = eng.bpd(x0, _outs(br.B, T), columns=(37, 5), noise_tape=nz[37:42], eps_tape=eps[37:42], clip_denoised=clip, use_graph=False)
        assert all(np.array_equal(p[:, 37:42], q[:, 37:42]) and np.isnan(q[:, :37]).all() and np.isnan(q[:, 42:]).all() for p, q in zip((vb, xs, ms), sub))
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------ Philox
def test_philox_loop_is_shard_invariant():
    import torch
    cfg, model, diffusion = _wrapped("ted", "ddim100", 1000)
    B = 8
    yh = synth.make_cond(cfg, B)
    x0 = torch.from_numpy(synth.make_init_image(cfg, B)).to(DEV)
    diffusion.noise_source, diffusion.philox_seed = "philox", 20260202
    alive = []      # the model keys its resident conditioning by the tensors' addresses: every shard's tensors stay allocated

    def run(first, count):
        diffusion.sample_offset = first
        y = {k: torch.from_numpy(v[first:first + count].copy()).to(DEV) for k, v in yh.items()}
        alive.append(y)
        r = _np(diffusion.calc_bpd_loop(model, x0[first:first + count], model_kwargs={"y": y}))
        assert diffusion.last_philox_seed == 20260202
        return r

    whole, h0, h1 = run(0, B), run(0, B // 2), run(B // 2, B // 2)
    for k in ("vb", "xstart_mse", "mse"):               # the loop's outputs: bitwise
        assert np.isfinite(whole[k]).all() and np.array_equal(whole[k], np.concatenate([h0[k], h1[k]])), k
    for k in ("prior_bpd", "total_bpd"):                # torch reductions on the caller's device: their summation order follows the batch shape
        assert np.allclose(whole[k], np.concatenate([h0[k], h1[k]]), rtol=1e-6, atol=0), k
    assert not np.array_equal(whole["vb"][:B // 2], whole["vb"][B // 2:])
    model.model.engine().close()


@pytest.mark.parametrize("ds,B", [("ted", 72), ("beat", 88)])
def test_multi_piece_plans_replayed_through_the_restatement(ds, B):
    """Philox on batches that `auto` runs in several launches or pieces per evaluation: the first and the last sample of every piece of
    its plan, replayed alone on the restated Philox draws (column k uses step_id k: oracle/philox_oracle.step_tapes), under rule R with
    ref_f64 from the restatement's own float64 run.  The call covers the schedule's last 12 columns (t = 11 .. 0), a sub-range."""
    from livelyspeaker_amd import _lib
    from oracle import philox_oracle as po
    cfg = synth.CONFIGS[ds]
    eng = _lib.Engine(cfg.njoints, cfg.nfeats, cfg.n_prefix_tokens, cfg.audio_len, n_emotions=cfg.n_emotions, path="auto")
    eng.load_state_dict(synth.make_state_dict(cfg))
    try:
        seed, off = 2020 + B, 1000
        y = synth.make_cond(cfg, B, scale=1.5)
        x0 = synth.make_init_image(cfg, B)
        sch = br.Schedule(1000, "ddim100")
        T = sch.num_timesteps
        cols = list(range(T - 12, T))
        eng.set_schedule(sch)
        eng.prepare(y)
        got = eng.bpd(x0, _outs(B, T), columns=(cols[0], len(cols)), philox_seed=seed, sample_offset=off)
        tm = eng.timing()
        pieces, _ = _lib.plan_query(B, dataset=ds, n_cus=tm["n_cus"])
        assert sum(n for _, _, n in pieces) == B and tm["step_path"] == pieces[0][0] and tm["n_step_launches"] == len(cols)
        assert all(np.isfinite(o[:, cols]).all() for o in got)
        pick = np.array(sorted({i for _, first, n in pieces for i in (first, first + n - 1)}))
        eps, nz = po.step_tapes(seed, off + pick, T, (cfg.njoints, cfg.nfeats, cfg.nframes))
        f64 = {}
        ref = br.bpd_loop(_oracle(cfg), sch, {k: v[pick] for k, v in y.items()}, x0[pick], nz, eps, True, columns=cols, f64=f64)
        _check_against_restatement([o[pick] for o in got], ref, f64, cols, x0[0].size, f"{ds} B={B} plan {pieces} samples {pick.tolist()}")
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------ torch's CPU stream
def test_torch_cpu_loop_follows_torch_manual_seed():
    import torch
    cfg, model, diffusion = _wrapped("ted", "ddim100", 1000)
    T = diffusion.num_timesteps
    x0 = torch.from_numpy(x_start_of("ted")).to(DEV)
    y = _cond(cfg, br.B)
    torch.manual_seed(97531)
    a = _np(diffusion.calc_bpd_loop(model, x0, model_kwargs={"y": y}))
    state_loop = torch.get_rng_state()
    torch.manual_seed(97531)
    draws = [d.numpy() for _ in range(T) for d in (torch.randn_like(x0.cpu()), torch.randn(br.B, 1, 512), torch.randn(br.B, 1, 512))]
    assert torch.equal(state_loop, torch.get_rng_state())               # the generator ends where the reference's draws leave it
    with _Tape(draws) as tp:                                            # the same draws handed in through torch's own (patched) calls
        b = _np(diffusion.calc_bpd_loop(model, x0, model_kwargs={"y": y}))
    assert tp.i == len(draws) and all(np.array_equal(a[k], b[k]) for k in a)
    model.model.engine().close()


def test_long_sequence_model_self_pinned():
    """SELF-PINNED: the reference cannot run 150 frames; the restatement on this repository's oracle is the only yardstick.  BEAT150,
    B = 8, ddim100: the schedule's first 2 and last 6 columns (two calls over sub-ranges)."""
    from livelyspeaker_amd import _lib
    cfg = synth.BEAT150
    eng = _lib.Engine(cfg.njoints, cfg.nfeats, cfg.n_prefix_tokens, cfg.audio_len, n_emotions=cfg.n_emotions, nframes=cfg.nframes)
    eng.load_state_dict(synth.make_state_dict(cfg))
    try:
        B = 8
        sch = br.Schedule(1000, "ddim100")
        T = sch.num_timesteps
        y = synth.make_cond(cfg, B)
        x0 = synth.make_init_image(cfg, B)
        nz, eps = br.loop_tape(cfg, T, seed=150, batch=B)
        eng.set_schedule(sch)
        eng.prepare(y)
        outs = _outs(B, T)
        eng.bpd(x0, outs, columns=(0, 2), noise_tape=nz[:2], eps_tape=eps[:2])
        eng.bpd(x0, outs, columns=(T - 6, 6), noise_tape=nz[T - 6:], eps_tape=eps[T - 6:])
        assert eng.timing()["step_path"] == 1
        cols = [0, 1] + list(range(T - 6, T))
        f64 = {}
        ref = br.bpd_loop(_oracle(cfg), sch, y, x0, nz, eps, True, columns=cols, f64=f64)
        _check_against_restatement(outs, ref, f64, cols, x0[0].size, "150 frames B=8")
        plain = _outs(B, T)
        eng.bpd(x0, plain, columns=(T - 6, 6), noise_tape=nz[T - 6:], eps_tape=eps[T - 6:], use_graph=False)
        assert all(np.array_equal(p[:, T - 6:], q[:, T - 6:]) for p, q in zip(outs, plain))
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_leave_the_handle_usable():
    import torch
    from livelyspeaker_amd import _lib
    cfg, model, diffusion = _wrapped("ted", "ddim100", 1000)
    T = diffusion.num_timesteps
    x0 = torch.from_numpy(x_start_of("ted")).to(DEV)
    y = _cond(cfg, br.B)
    diffusion.noise_source, diffusion.philox_seed = "philox", 7
    good = _np(diffusion.calc_bpd_loop(model, x0, model_kwargs={"y": y}))
    eng = model.model.engine()
    still_good = lambda: all(np.array_equal(good[k], v) for k, v in _np(diffusion.calc_bpd_loop(model, x0, model_kwargs={"y": y})).items())      # noqa: E731

    diffusion.noise_source = "torch_device"
    with pytest.raises(NotImplementedError, match="torch_device"):
        diffusion.calc_bpd_loop(model, x0, model_kwargs={"y": y})
    diffusion.noise_source = "philox"
    assert still_good()
    inp = dict(y, inpainting_mask=torch.zeros(x0.shape, dtype=torch.bool, device=DEV), inpainted_motion=torch.zeros_like(x0))
    with pytest.raises(NotImplementedError, match="inpainting"):
        diffusion.calc_bpd_loop(model, x0, model_kwargs={"y": inp})
    with pytest.raises(ValueError, match="shape"):
        diffusion.calc_bpd_loop(model, x0[:2], model_kwargs={"y": y})
    assert still_good()
    outs = tuple(torch.empty(br.B, T, device=DEV) for _ in range(3))
    for bad in (dict(columns=(T - 1, 2)), dict(columns=(-1, 2)), dict(columns=(0, 0)), dict(columns=(T, 1))):
        with pytest.raises(_lib.EngineError, match="columns"):
            eng.bpd(x0, outs, philox_seed=7, **bad)
    with pytest.raises(_lib.EngineError):                               # TAPE mode without tapes
        eng.bpd(x0, outs)
    with pytest.raises(_lib.EngineError):                               # outputs of the wrong shape
        eng.bpd(x0, tuple(torch.empty(br.B, T - 1, device=DEV) for _ in range(3)), philox_seed=7)
    a = _lib.LsBpdArgs()
    a.noise_mode, a.col_count = _lib.LS_NOISE_TORCH_DEVICE, T
    assert eng.lib.ls_bpd(eng.h, a) == -5 and b"TORCH_DEVICE" in eng.lib.ls_last_error(eng.h)
    with pytest.raises(_lib.EngineError, match="outside"):
        eng.vb_terms(x0, x0, x0, x0, index=T)
    with pytest.raises(_lib.EngineError, match="outside"):
        eng.vb_terms(x0, x0, x0, x0, indices=np.array([0, 1, 2, T], dtype=np.int64))
    assert still_good()
    eng.close()
