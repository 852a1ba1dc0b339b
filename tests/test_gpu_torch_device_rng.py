"""noise_source='torch_device': the reference's draws as a GPU run of it makes them (torch's device generator), generated on the device
inside the captured loop (csrc/ls_torch_philox.hip).  Judged against torch itself: the primitive against torch.randn, whole loops against
the same loops fed the tape that plain torch.randn / randn_like calls on the device draw (through the existing TAPE path), bitwise, with
the generator left where those calls leave it and the CPU generator untouched."""
import numpy as np
import pytest

from conftest import max_abs
from livelyspeaker_amd import _lib, synth
from test_gpu_boundary import _wrapped
from test_gpu_sampler_surface import _Tape

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIZES = [1, 3, 4, 255, 256, 257, 3672, 470016, 524287, 524288, 524289, 2097152, 2097153, 2454528, 5000000]


def _props():
    import torch
    p = torch.cuda.get_device_properties(0)
    return p.multi_processor_count, p.max_threads_per_multi_processor


@pytest.fixture(scope="module")
def bare_engine():
    cfg = synth.TED
    eng = _lib.Engine(cfg.njoints, cfg.nfeats, cfg.n_prefix_tokens, cfg.audio_len, device=0)
    yield eng
    eng.close()


@pytest.mark.parametrize("seed", [0, 1, 2 ** 63 + 5])
@pytest.mark.parametrize("offset", [0, 4, 49380, 2 ** 40])
def test_primitive_is_torch_randn_bitwise(bare_engine, seed, offset):
    import torch
    n_cu, thr = _props()
    for n in SIZES:
        g = torch.Generator(device=DEV)
        g.manual_seed(seed)
        g.set_offset(offset)
        want = torch.randn(n, device=DEV, generator=g)
        got = bare_engine.torch_randn(seed, offset, torch.full((n,), float("nan"), device=DEV))
        assert torch.equal(got, want), (seed, offset, n, int((got != want).sum()))
        assert g.get_offset() - offset == _lib.torch_randn_advance(n, n_cu, thr), n


def _seed(seed, offset):
    import torch
    gen = torch.cuda.default_generators[0]
    gen.manual_seed(seed)
    gen.set_offset(offset)
    return gen


def _reference_draws(seed, offset, shape, n_exec, *, x=True, inz=False, first=None):
    """What the reference's loop draws on the GPU, made with plain torch calls on the device from (seed, offset): x_T, then per step
    randn(B,1,512) x2, [randn_like(inpainted_motion) while t > 0], randn_like(x) -- x contiguous at the first step (or the caller's
    `noise`), in the model output's [T][B][J][F] memory order afterwards.  Returns the draws (numpy, logical layout) and the offset left."""
    import torch
    gen = _seed(seed, offset)
    B, J, F, T = shape
    later = torch.empty(T, B, J, F, device=DEV).permute(1, 2, 3, 0)
    out = [torch.randn(*shape, device=DEV)] if x else []
    for k in range(n_exec):
        out += [torch.randn(B, 1, 512, device=DEV), torch.randn(B, 1, 512, device=DEV)]
        if inz and k < n_exec - 1:
            out.append(torch.randn(*shape, device=DEV))
        out.append(torch.randn_like(later if k else (first if first is not None else torch.empty(shape, device=DEV))))
    return [a.cpu().numpy() for a in out], gen.get_offset()


CASES = {
    "ddpm12": dict(steps=12),
    "ddim100_skip90_init": dict(steps=1000, resp="ddim100", ddim=True, skip=90, init=True),
    "const_noise": dict(steps=12, const=True),
    "noise_given": dict(steps=12, noise=True),
    "dump_steps": dict(steps=12, dump=[0, 5, 11]),
    "inpainting": dict(steps=12, inpaint=True),
}


def _run_case(ds, case, B=4, seed=20261016, offset=49380, model=None, diffusion=None, compare=True, after=None):
    """One loop in torch_device mode against the same loop on the torch-drawn tape; returns (model, diffusion, result).  after():
    called right behind the torch_device loop (before the comparison loop runs)."""
    import torch
    c = CASES[case]
    if model is None:
        cfg, model, diffusion = _wrapped(ds, c.get("resp", ""), c["steps"])
    cfg = synth.CONFIGS[ds]
    shape = (B, cfg.njoints, cfg.nfeats, cfg.nframes)
    n_exec = diffusion.num_timesteps - c.get("skip", 0)
    y = {k: torch.from_numpy(v).to(DEV) for k, v in synth.make_cond(cfg, B).items()}
    inz = False
    if c.get("inpaint"):
        mask, motion, _ = synth.make_inpainting(cfg, B, n_exec)
        y["inpainting_mask"], y["inpainted_motion"] = torch.from_numpy(mask).to(DEV), torch.from_numpy(motion).to(DEV)
        inz = cfg.n_prefix_tokens == 1            # the TED tree re-noises the given motion each step (the BEAT tree does not)
    noise = torch.from_numpy(synth.NoiseTape(cfg, B, 1, seed=77).x_init).to(DEV) if c.get("noise") else None
    init = torch.from_numpy(synth.make_init_image(cfg, B)).to(DEV) if c.get("init") else None
    loop = diffusion.ddim_sample_loop if c.get("ddim") else diffusion.p_sample_loop
    kw = dict(noise=noise, clip_denoised=False, model_kwargs={"y": y}, skip_timesteps=c.get("skip", 0), init_image=init,
              const_noise=c.get("const", False), progress=False)
    if c.get("dump"):
        kw["dump_steps"] = c["dump"]
    draws, end = _reference_draws(seed, offset, shape, n_exec, x=noise is None, inz=inz, first=noise)
    _seed(seed, offset)
    cpu_state = torch.get_rng_state()
    diffusion.noise_source = "torch_device"
    got = loop(model, shape, **kw)
    if after is not None:
        after()
    assert torch.cuda.default_generators[0].get_offset() == end, case
    assert torch.equal(torch.get_rng_state(), cpu_state), case
    if compare:
        diffusion.noise_source = "torch_cpu"
        with _Tape(draws) as tp:
            want = loop(model, shape, **kw)
        assert tp.i == len(draws), case
        for a, b in zip(got if c.get("dump") else [got], want if c.get("dump") else [want]):
            assert torch.equal(a.cpu(), b.cpu()), (ds, case, max_abs(a.cpu().numpy(), b.cpu().numpy()))
    return model, diffusion, got


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("ds", ["ted", "beat"])
def test_whole_loop_is_torchs_own_device_draws_bitwise(ds, case):
    model, diffusion, _ = _run_case(ds, case)
    assert diffusion.last_device_rng_native
    model.model.engine().close()


@pytest.mark.parametrize("path,expect", [("fused", (0, 0)), ("batch", (1, 0)), ("coop8", (2, 8)), ("coop4", (2, 4)), ("coop2", (2, 2)),
                                         ("pass", (3, 0)), ("pass4", (3, 0)), ("mixer", (1, 4))])
def test_every_kernel_family_reads_the_generated_draws(path, expect):
    """TAPE mode on the torch-drawn tape vs TORCH_DEVICE mode, engine level, under each step-kernel selector."""
    import torch
    from oracle import rag_oracle as orc
    cfg = synth.BEAT150 if path == "mixer" else synth.TED
    B, steps, seed, off = (3 if path == "mixer" else 4), 8, 99, 4
    eng = _lib.Engine(cfg.njoints, cfg.nfeats, cfg.n_prefix_tokens, cfg.audio_len, n_emotions=cfg.n_emotions, nframes=cfg.nframes,
                      path="coop" if path == "mixer" else path)
    try:
        if path == "mixer":
            eng.set_path("coop")                # a long-sequence model: the one-launch mixer at any batch size
        eng.load_state_dict(synth.make_state_dict(cfg))
        eng.set_schedule(orc.Schedule(steps, ""))
        eng.prepare(synth.make_cond(cfg, B))
        shape = (B, cfg.njoints, cfg.nfeats, cfg.nframes)
        draws, end = _reference_draws(seed, off, shape, steps)
        x_T = torch.from_numpy(draws[0]).to(DEV)
        eps = torch.from_numpy(np.stack([np.stack([draws[1 + 3 * k][:, 0], draws[2 + 3 * k][:, 0]]) for k in range(steps)])).to(DEV)
        nz = torch.from_numpy(np.stack([draws[3 + 3 * k] for k in range(steps)])).to(DEV)
        want = eng.sample(x_init=x_T, eps_tape=eps, noise_tape=nz)
        got = eng.sample(torch_state=(seed, off), device_out=True)
        t = eng.timing()
        assert (t["step_path"], t["coop_slices"]) == expect, (path, t)
        assert torch.equal(got, want), (path, max_abs(got.cpu().numpy(), want.cpu().numpy()))
    finally:
        eng.close()


@pytest.mark.parametrize("ds", ["ted", "beat"])
def test_progressive_generators_end_where_the_loops_end(ds):
    import torch
    for case in ("ddpm12", "ddim100_skip90_init"):
        c = CASES[case]
        cfg, model, diffusion = _wrapped(ds, c.get("resp", ""), c["steps"])
        B = 4
        shape = (B, cfg.njoints, cfg.nfeats, cfg.nframes)
        y = {k: torch.from_numpy(v).to(DEV) for k, v in synth.make_cond(cfg, B).items()}
        init = torch.from_numpy(synth.make_init_image(cfg, B)).to(DEV) if c.get("init") else None
        diffusion.noise_source = "torch_device"
        prog = diffusion.ddim_sample_loop_progressive if c.get("ddim") else diffusion.p_sample_loop_progressive
        loop = diffusion.ddim_sample_loop if c.get("ddim") else diffusion.p_sample_loop
        kw = dict(clip_denoised=False, model_kwargs={"y": y}, skip_timesteps=c.get("skip", 0), init_image=init, progress=False)
        gen = _seed(5, 8)
        last = None
        for r in prog(model, shape, **kw):
            last = r["sample"]
        end = gen.get_offset()
        _seed(5, 8)
        whole = loop(model, shape, **kw)
        assert gen.get_offset() == end and torch.equal(whole.cpu(), last.cpu()), (ds, case)
        model.model.engine().close()


def test_graph_replay_ring_wrap_and_full_batch():
    import torch
    model, diffusion, _ = _run_case("ted", "ddpm12", compare=False)          # captures the loop
    eng = model.model.engine()
    seen = []
    _run_case("ted", "ddpm12", seed=3, offset=1 << 40, model=model, diffusion=diffusion,   # same shapes, a new generator state: replayed
              after=lambda: seen.append(eng.timing()))
    assert seen[0]["graph_replayed"] == 1 and seen[0]["tape_upload_ms"] == 0, seen
    # a ring of 3 steps: 12 steps refill it four times, inside the captured loop
    cfg = synth.TED
    diffusion.device_ring_bytes = 3 * (2 * 4 * 512 + 4 * cfg.njoints * cfg.nfeats * cfg.nframes) * 4
    _run_case("ted", "ddpm12", seed=11, model=model, diffusion=diffusion)
    _run_case("ted", "inpainting", seed=12, model=model, diffusion=diffusion)
    eng.close()
    # the headline batch, 20 steps
    cfg, model, diffusion = _wrapped("ted", "", 20)
    CASES["ddpm20"] = dict(steps=20)
    try:
        _run_case("ted", "ddpm20", B=512, seed=2 ** 63 + 5, model=model, diffusion=diffusion)
        assert diffusion.last_device_rng_native
    finally:
        del CASES["ddpm20"]
        model.model.engine().close()


def test_values_match_the_cpu_oracle_on_the_torch_drawn_tape():
    import torch
    from oracle import rag_oracle as orc
    cfg, B, steps = synth.TED, 2, 6
    sd = synth.make_state_dict(cfg)
    eng = _lib.Engine(cfg.njoints, cfg.nfeats, cfg.n_prefix_tokens, cfg.audio_len, device=0)
    try:
        eng.load_state_dict(sd)
        sch = orc.Schedule(steps, "")
        eng.set_schedule(sch)
        y = synth.make_cond(cfg, B)
        eng.prepare(y)
        shape = (B, cfg.njoints, cfg.nfeats, cfg.nframes)
        draws, _ = _reference_draws(42, 0, shape, steps)
        eps = np.stack([np.stack([draws[1 + 3 * k][:, 0], draws[2 + 3 * k][:, 0]]) for k in range(steps)])
        nz = np.stack([draws[3 + 3 * k] for k in range(steps)])
        got = eng.sample(torch_state=(42, 0), device_out=True).cpu().numpy()
        want = orc.sample_loop(orc.RagOracle(sd, cfg.njoints, cfg.nfeats, cfg.n_prefix_tokens), sch, y, draws[0], eps, nz)
        d = max_abs(got, want)
        print(f"torch_device loop vs CPU oracle on torch's draws: {d:.3e}")
        assert d <= 2e-4, d
    finally:
        eng.close()


def test_fallback_to_torchs_draws_is_bitwise_the_native_loop():
    import torch
    from livelyspeaker_amd import gaussian_diffusion as gd
    model, diffusion, native = _run_case("ted", "ddpm12", compare=False)
    assert diffusion.last_device_rng_native
    saved = dict(gd._DEVICE_RNG_OK)
    try:
        gd._DEVICE_RNG_OK[0] = False           # the self-check failed: torch's own device calls draw the tape
        for seg in (None, 3):                  # one piece, and 3-step device segments through the segmented TAPE path
            if seg:
                cfg = synth.TED
                diffusion.tape_segment_bytes = seg * (2 * 4 * 512 + 4 * cfg.njoints * cfg.nfeats * cfg.nframes) * 4
            _, _, got = _run_case("ted", "ddpm12", model=model, diffusion=diffusion, compare=False)
            assert not diffusion.last_device_rng_native
            assert torch.equal(got.cpu(), native.cpu()), seg
        assert diffusion.last_tape_segments == 4
    finally:
        gd._DEVICE_RNG_OK.clear()
        gd._DEVICE_RNG_OK.update(saved)
        model.model.engine().close()


def test_direct_model_call_draws_its_style_eps_on_the_device():
    import torch
    cfg, model, _ = _wrapped("ted", "", 12)
    rag = model.model
    B = 4
    y = {k: torch.from_numpy(v).to(DEV) for k, v in synth.make_cond(cfg, B).items()}
    x = torch.from_numpy(synth.NoiseTape(cfg, B, 1).x_init).to(DEV)
    t = torch.full((B,), 7, dtype=torch.long, device=DEV)
    rag.noise_source = "torch_device"
    gen = _seed(9, 0)
    cpu_state = torch.get_rng_state()
    out = rag(x, t, y=y)["output"]
    assert gen.get_offset() == _lib.torch_randn_advance(B * 512, *_props()) and torch.equal(torch.get_rng_state(), cpu_state)
    _seed(9, 0)
    eps = torch.randn(B, 1, 512, device=DEV).cpu().numpy()
    rag.noise_source = "torch_cpu"
    with _Tape([eps]):
        want = rag(x, t, y=y)["output"]
    assert torch.equal(out.cpu(), want.cpu())
    rag.engine().close()
