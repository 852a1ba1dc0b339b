"""Per-row Philox keys of a sampling call on the GPU (``diffusion.row_keys`` -> ls_set_row_keys, csrc/ls_philox_rows.hip).

Row b draws every stream at ``gidx = row_keys[b]`` in place of ``sample_offset + b``.  The draws are written to device tapes by the
arithmetic of csrc/ls_philox.h and read by the step kernels as tapes, so ``row_keys = o + arange(B)`` must be the call at
``sample_offset = o`` BIT FOR BIT, on every kernel family, and keys no offset can express must replay through the CPU oracle.  B = 5
(odd, more than one workgroup on every family), 12 executed steps (1000 steps respaced to 100, skip 88), both datasets, synthetic weights."""
import numpy as np
import pytest
import torch

from conftest import max_abs
from livelyspeaker_amd import synth
from test_gpu_long_stream import DEV, T, _parts
from test_gpu_philox import TOL_LOOP

pytestmark = [pytest.mark.gpu, pytest.mark.engine_path_auto]
# every kernel family ls_set_path can force at a batch of 5: tests/test_gpu_coop.py and tests/test_gpu_pass.py enumerate the last five
FORMS = ["fused", "batch", "coop8", "coop4", "coop2", "pass", "pass4"]
SEED, O = 0x5EED_0F_C11B5, 11


def _cond(cfg, B, scale=1.5):
    return {k: torch.from_numpy(v).to(DEV) for k, v in synth.make_cond(cfg, B, seed=synth.SEED_COND + 5200, scale=scale).items()}


def _call(parts, y, row_keys=None, offset=0):
    cfg, model, diffusion, sampler, skip, _ = parts
    loop = diffusion.ddim_sample_loop if sampler == "ddim" else diffusion.p_sample_loop
    B = int(y["scale"].shape[0])
    diffusion.row_keys, diffusion.sample_offset = row_keys, offset
    try:
        x = loop(model, (B, cfg.njoints, cfg.nfeats, T), clip_denoised=False, model_kwargs={"y": y}, skip_timesteps=skip, init_image=None,
                 progress=False, dump_steps=None, noise=None, const_noise=False)
    finally:
        diffusion.row_keys, diffusion.sample_offset = None, 0
    return x.contiguous(), model.model.engine().timing()


class _Philox:
    """``noise_source='philox'`` under one pinned seed on a cached model, on the kernel family ``form``; everything put back on the way out."""

    def __init__(self, parts, form="fused"):
        self.model, self.diffusion, self.form = parts[1], parts[2], form

    def __enter__(self):
        d = self.diffusion
        self.was = (d.noise_source, d.philox_seed, d.device_ring_bytes, self.model.model.step_path)
        d.noise_source, d.philox_seed, self.model.model.step_path = "philox", SEED, self.form
        return self

    def __exit__(self, *exc):
        d = self.diffusion
        d.noise_source, d.philox_seed, d.device_ring_bytes, self.model.model.step_path = self.was
        return False


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("schedule", ["ddim", "ddpm"])
@pytest.mark.parametrize("ds", ["ted", "beat"])
def test_keys_that_spell_an_offset_are_that_offset_bitwise(ds, schedule, form):
    parts = _parts(ds, schedule)
    y = _cond(parts[0], 5)
    keys = O + np.arange(5)
    with _Philox(parts, form):
        want, _ = _call(parts, y, offset=O)
        plain, _ = _call(parts, y)
        assert bool(torch.isfinite(want).all()) and not torch.equal(want, plain)            # the offset matters
        first, t1 = _call(parts, y, row_keys=keys)                                          # a keyed loop is never the unkeyed one's graph: captured
        again, t2 = _call(parts, y, row_keys=torch.from_numpy(keys))                        # ... and replayed
        print(f"{ds} {schedule} [{form}]: max |keyed - offset| = {float((first - want).abs().max()):.3e}, replayed {t1['graph_replayed']} {t2['graph_replayed']}")
        assert torch.equal(first, want), float((first - want).abs().max())
        assert torch.equal(again, want)
        if parts[2].use_graph:
            assert (t1["graph_replayed"], t2["graph_replayed"]) == (0, 1)
        back, _ = _call(parts, y, offset=O)                                                # the keys are gone with the call that set them
        assert torch.equal(back, want)


@pytest.mark.parametrize("schedule", ["ddim", "ddpm"])
@pytest.mark.parametrize("ds", ["ted", "beat"])
def test_ring_refills_inside_the_loop_change_nothing(ds, schedule):
    """A ring of two steps (TED) or one (BEAT: a step's draws are larger than the budget): six or twelve refills inside the captured loop."""
    parts = _parts(ds, schedule)
    y = _cond(parts[0], 5)
    with _Philox(parts):
        want, _ = _call(parts, y, offset=O)
        parts[2].device_ring_bytes = 100_000
        got, _ = _call(parts, y, row_keys=(O + np.arange(5)).tolist())
        assert torch.equal(got, want), float((got - want).abs().max())


@pytest.mark.parametrize("schedule", ["ddim", "ddpm"])
@pytest.mark.parametrize("ds", ["ted", "beat"])
def test_rows_and_keys_permuted_together_permute_the_output(ds, schedule):
    parts = _parts(ds, schedule)
    y = _cond(parts[0], 5)
    perm = torch.tensor([3, 0, 4, 2, 1], device=DEV)
    keys = np.array([41, 7, (1 << 40) + 3, 1000, 2], dtype=np.uint64)
    with _Philox(parts):
        base, _ = _call(parts, y, row_keys=keys)
        yp = {k: v[perm].contiguous() for k, v in y.items()}
        got, _ = _call(parts, yp, row_keys=keys[perm.cpu().numpy()])
    assert not torch.equal(base[0], base[1])
    assert torch.equal(got, base[perm]), float((got - base[perm]).abs().max())


@pytest.mark.parametrize("ds,schedule", [("ted", "ddim"), ("ted", "ddpm"), ("beat", "ddpm")])
def test_keys_no_offset_can_spell_replay_through_the_oracle(ds, schedule):
    """gidx = 7, 2^32 + 5 (the high counter word) and (3 << 48) + 1 (the window bits): x_T, the style eps and -- under DDPM -- the step
    noise of each row from the numpy restatement, through the CPU oracle.  A wrong counter word moves the result by O(1)."""
    from oracle import philox_oracle as po
    from oracle import rag_oracle as orc
    parts = _parts(ds, schedule)
    cfg, skip = parts[0], parts[4]
    gidx = [7, (1 << 32) + 5, (3 << 48) + 1]
    y = _cond(cfg, 3)
    with _Philox(parts):
        got, _ = _call(parts, y, row_keys=gidx)
        low, _ = _call(parts, y, row_keys=[g & 0xFFFFFFFF for g in gidx])
    sch = orc.Schedule(1000, "ddim100" if schedule == "ddim" else "100")
    n_exec = sch.num_timesteps - skip
    assert n_exec == 12
    g64 = np.array(gidx, dtype=np.uint64)
    eps, noise = po.step_tapes(SEED, g64, n_exec, (cfg.njoints, cfg.nfeats, cfg.nframes))
    x_T = po.x_init(SEED, g64, cfg.njoints * cfg.nfeats, cfg.nframes, (cfg.njoints, cfg.nfeats))
    oracle = orc.RagOracle(synth.make_state_dict(cfg), cfg.njoints, cfg.nfeats, cfg.n_prefix_tokens)
    want = orc.sample_loop(oracle, sch, {k: v.cpu().numpy() for k, v in y.items()}, x_T, eps, noise, ddim=schedule == "ddim", skip_timesteps=skip,
                           init_image=None)
    d = [max_abs(got[b].cpu().numpy(), want[b]) for b in range(3)]
    print(f"{ds} {schedule}: max |hip - oracle| per row {[float(f'{v:.2e}') for v in d]}")
    assert max(d) < TOL_LOOP
    # the check has teeth: rows 1 and 2 with their high words dropped are far away, row 0 (no high word) is the same row
    assert torch.equal(low[0], got[0]) and min(max_abs(low[b].cpu().numpy(), want[b]) for b in (1, 2)) > 1e-2
