"""CPU: the "identical seeds" draw order of every sampling entry point (livelyspeaker_amd/ref_draws.py) against the reference's lines
written out as literal torch calls: which normals a call draws from torch's CPU generator, in which order, shapes and memory orders, and
where it leaves the generator.  The engine is a recording stand-in; nothing here imports ref_draws."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from livelyspeaker_amd import _lib, long_form, synth, torch_rng
from livelyspeaker_amd import gaussian_diffusion as gd
from livelyspeaker_amd.cfg_sampler import ClassifierFreeSampleModel
from livelyspeaker_amd.model_util import create_gaussian_diffusion, create_model_and_diffusion

B, J, F, T, D = 3, 9, 3, 34, 512
SHAPE = (B, J, F, T)
STEPS, SKIP, SEED = 5, 2, 4711
ARGS = SimpleNamespace(mdm_condm="text", latent_dim=512, ff_size=1024, layers=8, cond_mask_prob=0.1, arch="trans_enc", emb_trans_dec=False,
                       dataset="humanml", lang_model=None, mlpact="silu", diffusion_steps=STEPS, noise_schedule="cosine", sigma_small=True,
                       lambda_vel=1.0, lambda_rcxyz=0.0, lambda_fc=0.0, njoints=J)


class _Recorder:
    """Keeps what the sampler hands to the engine; stands in for libls_hip.so."""
    J, F, T, D, batch, n_steps, device = J, F, T, D, B, STEPS, 0

    def __init__(self):
        self.calls = []

    def _keep(self, name, args, kw):
        keep = lambda v: v.clone() if torch.is_tensor(v) else v      # noqa: E731
        self.calls.append((name, [keep(a) for a in args], {k: keep(v) for k, v in kw.items()}))

    def set_schedule(self, sched):
        self.n_steps = sched.num_timesteps

    def sample(self, **kw):
        self._keep("sample", (), kw)
        seg = kw.get("segment")
        last = seg is None or seg[0] + seg[1] == self.n_steps - kw["skip_timesteps"]
        return np.zeros(SHAPE, np.float32) if last else None

    def bpd(self, x_start, out, **kw):
        self._keep("bpd", (x_start,), kw)
        for o in out:
            o[:] = 1.0

    def long_prepare(self, *args, **kw):
        self._keep("long_prepare", args, kw)

    def long_sample(self, **kw):
        self._keep("long_sample", (), kw)
        return np.zeros((B, J, F, T + 2 * (T - 4)), np.float32)

    def step(self, *args, **kw):
        self._keep("step", args, kw)
        return np.zeros(SHAPE, np.float32), np.zeros(SHAPE, np.float32)

    def plms_step(self, *args, **kw):
        self._keep("plms_step", args, kw)
        return np.zeros(SHAPE, np.float32), np.zeros(SHAPE, np.float32), np.zeros(SHAPE, np.float32)

    def kw(self, name="sample"):
        found = [c for c in self.calls if c[0] == name]
        assert len(found) == 1, [c[0] for c in self.calls]
        return found[0][2]


@pytest.fixture(scope="module")
def rag():
    return create_model_and_diffusion(ARGS, "")[0]


@pytest.fixture
def rig(rag, monkeypatch):
    """(a fresh diffusion object, the CFG-wrapped model, the recording engine behind it)."""
    eng = _Recorder()
    monkeypatch.setattr(type(rag), "_engine_prepared", lambda self, y: eng)
    monkeypatch.setattr(type(rag), "engine", lambda self: eng)
    return create_gaussian_diffusion(ARGS, ""), ClassifierFreeSampleModel(rag), eng


def later_proto():
    """x after the first executed step: the model output's permuted view (OutputProcess, RAG.py:209-210), memory order [T][B][J][F]."""
    return torch.empty(T, B, J, F).permute(1, 2, 3, 0)


def strided_noise():
    return torch.randn(T, B, J, F, generator=torch.Generator().manual_seed(3)).permute(1, 2, 3, 0)


def run_seeded(fn):
    """fn() from torch.manual_seed(SEED) with a cached double sample left behind; returns (fn's result, the generator state it leaves)."""
    torch.manual_seed(SEED)
    torch.randn(3)
    res = fn()
    return res, torch.get_rng_state()


def state_is(state, literal):
    """`literal` makes the reference's draws from the same start; the generator must end where the call under test left it."""
    want, end = run_seeded(literal)
    assert torch.equal(state, end), "the generator does not end where the reference's draws leave it"
    return want


def ref_steps(n_exec, first_proto, inpainted=None):
    """The loop body's draws (gaussian_diffusion.py:718-743 -> p_sample :507-558 / ddim_sample :745-798 -> p_mean_variance :284-399)."""
    eps, nz, inz = [], [], []
    x_proto = first_proto
    for k in range(n_exec):
        t = n_exec - 1 - k
        eps.append(torch.stack([torch.randn(B, 1, D)[:, 0],                 # cond pass: reparameterize (RAG.py:10-13)
                                torch.randn(B, 1, D)[:, 0]]))               # uncond pass
        if inpainted is not None:
            inz.append(torch.randn_like(inpainted) if t > 0 else torch.zeros(SHAPE))    # q_sample(inpainted_motion, t - 1) while t[0] > 0 (:318)
        nz.append(torch.randn_like(x_proto).contiguous())                   # :543 / :787
        x_proto = later_proto()
    return torch.stack(eps), torch.stack(nz), (torch.stack(inz) if inz else None)


def loop_fn(diff, name):
    return getattr(diff, name)


LOOPS = ["p_sample_loop", "ddim_sample_loop"]


@pytest.mark.parametrize("loop", LOOPS)
@pytest.mark.parametrize("const_noise", [False, True])
def test_loop_draws_x_T_then_each_steps_pair_and_noise(rig, loop, const_noise):
    diff, model, eng = rig
    _, state = run_seeded(lambda: loop_fn(diff, loop)(model, SHAPE, clip_denoised=False, model_kwargs={"y": {}}, device="cpu", const_noise=const_noise))

    def literal():
        x = torch.randn(*SHAPE)                                             # :701-704
        if const_noise:
            x = x[[0]].repeat(B, 1, 1, 1)
        return (x,) + ref_steps(STEPS, torch.empty(SHAPE))
    x, eps, nz, _ = state_is(state, literal)
    kw = eng.kw()
    assert torch.equal(kw["x_init"], x) and torch.equal(kw["eps_tape"], eps) and torch.equal(kw["noise_tape"], nz)
    assert kw["const_noise"] is const_noise and "inpaint" not in kw and "use_graph" in kw and diff.last_tape_segments == 1


@pytest.mark.parametrize("loop", LOOPS)
def test_loop_with_strided_noise_follows_its_strides_at_the_first_step(rig, loop):
    diff, model, eng = rig
    noise = strided_noise()
    assert not noise.is_contiguous()
    _, state = run_seeded(lambda: loop_fn(diff, loop)(model, SHAPE, noise=noise, model_kwargs={"y": {}}, device="cpu"))
    eps, nz, _ = state_is(state, lambda: ref_steps(STEPS, noise))           # no x_T draw; x of the first step IS `noise`
    kw = eng.kw()
    assert kw["x_init"] is not None and torch.equal(kw["x_init"], noise)
    assert torch.equal(kw["eps_tape"], eps) and torch.equal(kw["noise_tape"], nz)
    assert not torch.equal(nz[0], run_seeded(lambda: ref_steps(1, torch.empty(SHAPE)))[0][1][0])     # a contiguous first step draws otherwise
    assert not diff.last_host_rng_native


@pytest.mark.parametrize("loop", LOOPS)
def test_loop_with_noise_init_image_and_skip_draws_a_contiguous_first_step(rig, loop):
    diff, model, eng = rig
    noise, init = strided_noise(), torch.ones(SHAPE)
    _, state = run_seeded(lambda: loop_fn(diff, loop)(model, SHAPE, noise=noise, init_image=init, skip_timesteps=SKIP, model_kwargs={"y": {}},
                                                       device="cpu"))
    eps, nz, _ = state_is(state, lambda: ref_steps(STEPS - SKIP, torch.empty(SHAPE)))     # x = q_sample(init_image, t, noise): a new tensor (:714-716)
    kw = eng.kw()
    assert torch.equal(kw["eps_tape"], eps) and torch.equal(kw["noise_tape"], nz) and kw["skip_timesteps"] == SKIP
    assert torch.equal(kw["x_init"], noise) and torch.equal(kw["init_image"], init)


@pytest.mark.parametrize("loop", LOOPS)
@pytest.mark.parametrize("n_prefix", [1, 2])
def test_loop_inpainting_draws_the_renoise_only_on_the_one_prefix_model(rig, rag, monkeypatch, loop, n_prefix):
    """The TED tree (one prefix token) re-noises inpainted_motion with q_sample(., t - 1) while t[0] > 0 -- one randn_like between the
    model call and the step's noise at every step but the last; the BEAT tree (two prefix tokens) mixes it in as it is: no such draw."""
    diff, model, eng = rig
    monkeypatch.setattr(rag, "n_prefix_tokens", n_prefix)
    motion = strided_noise() * 0.5
    y = {"inpainting_mask": torch.zeros(SHAPE, dtype=torch.bool), "inpainted_motion": motion}
    _, state = run_seeded(lambda: loop_fn(diff, loop)(model, SHAPE, model_kwargs={"y": y}, device="cpu"))
    x, eps, nz, inz = state_is(state, lambda: (torch.randn(*SHAPE),) + ref_steps(STEPS, torch.empty(SHAPE), motion if n_prefix == 1 else None))
    kw = eng.kw()
    assert torch.equal(kw["x_init"], x) and torch.equal(kw["eps_tape"], eps) and torch.equal(kw["noise_tape"], nz)
    mask, mot, got_inz, renoise = kw["inpaint"]
    assert mask is y["inpainting_mask"] and mot is motion and renoise is (n_prefix == 1)
    if n_prefix == 1:
        assert torch.equal(got_inz, inz) and not got_inz[-1].any() and all(got_inz[k].any() for k in range(STEPS - 1))
    else:
        assert got_inz is None and inz is None


@pytest.mark.parametrize("loop", LOOPS)
def test_segmented_tapes_are_the_one_piece_tapes(rig, monkeypatch, loop):
    diff, model, eng = rig
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)                    # the segmented path is for the GPU build only
    monkeypatch.setattr(gd.GaussianDiffusion, "_tape_ring", lambda self, K, B_, D_, shape:
                        [(torch.empty(K, 2, B_, D_), torch.empty((K,) + tuple(shape))) for _ in range(2)])      # (no page-locked memory here)
    call = lambda: loop_fn(diff, loop)(model, SHAPE, clip_denoised=False, model_kwargs={"y": {}}, device="cpu")      # noqa: E731
    _, one_state = run_seeded(call)
    one = eng.kw()
    eng.calls.clear()
    diff.tape_segment_bytes = 2 * 2 * (2 * B * D + B * J * F * T) * 4                # room for two 2-step segments
    _, seg_state = run_seeded(call)
    seg = [c[2] for c in eng.calls]
    assert torch.equal(one_state, seg_state)
    assert [c["segment"] for c in seg] == [(0, 2), (2, 2), (4, 1)] and diff.last_tape_segments == 3 and diff.last_host_rng_ms > 0
    assert torch.equal(torch.cat([c["eps_tape"] for c in seg]), one["eps_tape"])
    assert torch.equal(torch.cat([c["noise_tape"] for c in seg]), one["noise_tape"])
    assert all(torch.equal(c["x_init"], one["x_init"]) and not c["x_init"].is_cuda for c in seg)
    assert all("use_graph" not in c and c["two_pass_always"] is False for c in seg) and "use_graph" in one
    x, eps, nz, _ = state_is(seg_state, lambda: (torch.randn(*SHAPE),) + ref_steps(STEPS, torch.empty(SHAPE)))
    assert torch.equal(one["x_init"], x) and torch.equal(one["eps_tape"], eps) and torch.equal(one["noise_tape"], nz)


def test_plms_loop_draws_x_T_and_one_pair_per_evaluation(rig):
    diff, model, eng = rig
    _, state = run_seeded(lambda: diff.plms_sample_loop(model, SHAPE, model_kwargs={"y": {}}, device="cpu", skip_timesteps=SKIP))
    n_exec = STEPS - SKIP

    def literal():          # :1100-1211: the first step evaluates the model twice, every later one once; plms_sample adds no noise
        x = torch.randn(*SHAPE)
        return x, torch.stack([torch.stack([torch.randn(B, 1, D)[:, 0], torch.randn(B, 1, D)[:, 0]]) for _ in range(n_exec + 1)])
    x, eps = state_is(state, literal)
    kw = eng.kw()
    assert torch.equal(kw["x_init"], x) and torch.equal(kw["eps_tape"], eps) and "noise_tape" not in kw
    assert tuple(kw["eps_tape"].shape) == (n_exec + 1, 2, B, D) and kw["sampler"] == _lib.LS_SAMPLER_PLMS


def long_call(diff, model, **kw):
    y = synth.make_long_cond(synth.TED, B, 3)
    return long_form.sample_long(diff, model, y["audio"], y["seed_poses"], y["vid_indices"], y["scale"], **kw)


def ref_windows(W, n_exec):
    """One sample loop per window (the chain of the reference's callers): x_T, then the window's steps."""
    xs, eps, nz = [], [], []
    for _ in range(W):
        xs.append(torch.randn(*SHAPE))
        e, n, _ = ref_steps(n_exec, torch.empty(SHAPE))
        eps.append(e)
        nz.append(n)
    return torch.stack(xs), torch.stack(eps), torch.stack(nz)


def test_long_form_draws_window_after_window(rig):
    diff, model, eng = rig
    _, state = run_seeded(lambda: long_call(diff, model, skip_timesteps=SKIP))
    x, eps, nz = state_is(state, lambda: ref_windows(3, STEPS - SKIP))
    kw = eng.kw("long_sample")
    assert torch.equal(kw["x_init"], x) and torch.equal(kw["eps_tape"], eps) and torch.equal(kw["noise_tape"], nz)
    assert tuple(kw["noise_tape"].shape) == (3, STEPS - SKIP) + SHAPE and eng.kw("long_prepare")["n_windows"] == 3


def _no_normals(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("philox mode drew a normal from torch")
    monkeypatch.setattr(torch, "randn", refuse)
    monkeypatch.setattr(torch, "randn_like", refuse)


PHILOX_CALLS = {
    "p_sample_loop": lambda d, m: d.p_sample_loop(m, SHAPE, model_kwargs={"y": {}}, device="cpu"),
    "ddim_sample_loop": lambda d, m: d.ddim_sample_loop(m, SHAPE, model_kwargs={"y": {}}, device="cpu"),
    "plms_sample_loop": lambda d, m: d.plms_sample_loop(m, SHAPE, model_kwargs={"y": {}}, device="cpu"),
    "calc_bpd_loop": lambda d, m: d.calc_bpd_loop(m, torch.zeros(SHAPE), model_kwargs={"y": {}}),
    "sample_long": long_call,
}


@pytest.mark.parametrize("pinned", [None, 20261018])
@pytest.mark.parametrize("entry", sorted(PHILOX_CALLS))
def test_philox_mode_consumes_exactly_one_randint(rig, monkeypatch, entry, pinned):
    diff, model, eng = rig
    diff.noise_source, diff.philox_seed, diff.sample_offset = "philox", pinned, 6
    torch.manual_seed(SEED)
    _no_normals(monkeypatch)
    PHILOX_CALLS[entry](diff, model)
    state = torch.get_rng_state()
    torch.manual_seed(SEED)
    drawn = int(torch.randint(0, 2 ** 62, (1,)).item())                     # drawn also when philox_seed pins the key
    assert torch.equal(state, torch.get_rng_state())
    kw = eng.kw({"calc_bpd_loop": "bpd", "sample_long": "long_sample"}.get(entry, "sample"))
    assert kw["philox_seed"] == diff.last_philox_seed == (drawn if pinned is None else pinned) and kw["sample_offset"] == 6
    assert kw.get("eps_tape") is None and kw.get("noise_tape") is None and kw.get("x_init") is None


def _step_inputs(inpaint):
    x = strided_noise()
    y = {}
    if inpaint:
        y = {"inpainting_mask": torch.zeros(SHAPE, dtype=torch.bool), "inpainted_motion": strided_noise() * 0.5}
    return x, y


@pytest.mark.parametrize("name", ["p_sample", "ddim_sample"])
@pytest.mark.parametrize("inpaint,t", [(False, 3), (True, 3), (True, 0)])
def test_single_step_draws_the_pair_the_renoise_and_the_step_noise(rig, name, inpaint, t):
    diff, model, eng = rig
    x, y = _step_inputs(inpaint)
    _, state = run_seeded(lambda: getattr(diff, name)(model, x, torch.full((B,), t), clip_denoised=False, model_kwargs={"y": y}))

    def literal():
        eps_c, eps_u = torch.randn(B, 1, D), torch.randn(B, 1, D)           # RAG.py:10-13, cond pass then uncond pass
        inz = torch.randn_like(y["inpainted_motion"]) if (inpaint and t > 0) else None      # :318
        return eps_c, eps_u, inz, torch.randn_like(x)                        # :543 / :787, in x's memory order
    eps_c, eps_u, inz, noise = state_is(state, literal)
    name_, args, kw = eng.calls[-1]
    assert name_ == "step" and torch.equal(args[3], eps_c) and torch.equal(args[4], eps_u)
    assert torch.equal(args[5], noise) and args[5].stride() == x.stride()
    if inpaint:
        assert (kw["inpaint"][2] is None) if inz is None else torch.equal(kw["inpaint"][2], inz)
    else:
        assert kw["inpaint"] is None


def test_plms_sample_draws_four_eps_at_a_first_step_and_two_afterwards(rig):
    diff, model, eng = rig
    x = strided_noise()
    out, state = run_seeded(lambda: diff.plms_sample(model, x, torch.full((B,), 3), model_kwargs={"y": {}}, order=3))
    want = state_is(state, lambda: [torch.randn(B, 1, D) for _ in range(4)])   # two evaluations (:1064-1070), a pair each; no step noise
    _, args, kw = eng.calls[-1]
    assert all(torch.equal(a, b) for a, b in zip(list(args[3]) + list(kw["eps2"]), want))
    _, state = run_seeded(lambda: diff.plms_sample(model, out["sample"], torch.full((B,), 2), model_kwargs={"y": {}}, order=3, old_out=out))
    want = state_is(state, lambda: [torch.randn(B, 1, D) for _ in range(2)])
    _, args, kw = eng.calls[-1]
    assert all(torch.equal(a, b) for a, b in zip(args[3], want)) and kw["eps2"] is None


def _tapes_of(entry, diff, model, eng):
    eng.calls.clear()
    if entry == "loop":
        _, state = run_seeded(lambda: diff.p_sample_loop(model, SHAPE, model_kwargs={"y": {}}, device="cpu"))
        kw = eng.kw()
    elif entry == "long":
        _, state = run_seeded(lambda: long_call(diff, model))
        kw = eng.kw("long_sample")
    else:
        _, state = run_seeded(lambda: diff.calc_bpd_loop(model, torch.from_numpy(synth.make_init_image(synth.TED, B)), model_kwargs={"y": {}}))
        kw = eng.kw("bpd")
    return [kw[k] for k in ("x_init", "eps_tape", "noise_tape") if k in kw], state


@pytest.mark.parametrize("entry", ["loop", "long", "bpd"])
def test_native_and_torch_paths_give_the_same_tapes_and_end_state(rig, entry):
    diff, model, eng = rig
    diff.native_host_rng = False
    torch_tapes, torch_state = _tapes_of(entry, diff, model, eng)
    assert not diff.last_host_rng_native and len(torch_tapes) == (2 if entry == "bpd" else 3)
    if torch_rng.variant() < 0:
        pytest.skip("no native restatement reproduces this torch build: the torch path is the only one")
    diff.native_host_rng = True
    native_tapes, native_state = _tapes_of(entry, diff, model, eng)
    assert diff.last_host_rng_native
    assert all(torch.equal(a, b) for a, b in zip(native_tapes, torch_tapes)) and torch.equal(native_state, torch_state)


def test_patched_randn_sees_every_draw_of_the_loop(rig, monkeypatch):
    diff, model, eng = rig
    seen = []
    real_randn, real_like = torch.randn, torch.randn_like

    def randn(*a, **k):
        seen.append(tuple(a))
        return real_randn(*a, **k)

    def randn_like(p, **k):
        seen.append(("like", tuple(p.shape), p.stride()))
        return real_like(p, **k)
    monkeypatch.setattr(torch, "randn", randn)
    monkeypatch.setattr(torch, "randn_like", randn_like)
    _, state = run_seeded(lambda: diff.p_sample_loop(model, SHAPE, model_kwargs={"y": {}}, device="cpu"))
    assert not diff.last_host_rng_native                                    # the native stream stood aside
    n_setup = len(seen)
    monkeypatch.undo()
    x, eps, nz, _ = state_is(state, lambda: (torch.randn(*SHAPE),) + ref_steps(STEPS, torch.empty(SHAPE)))
    kw = eng.calls[-1][2]
    assert torch.equal(kw["x_init"], x) and torch.equal(kw["eps_tape"], eps) and torch.equal(kw["noise_tape"], nz)
    want = [(3,), SHAPE]                                                    # run_seeded's own randn(3), then x_T
    for k in range(STEPS):
        proto = torch.empty(SHAPE) if k == 0 else later_proto()
        want += [(B, 1, D), (B, 1, D), ("like", SHAPE, proto.stride())]
    assert seen[:n_setup] == want
