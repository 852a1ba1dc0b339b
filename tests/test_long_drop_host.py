"""Host side of ``sample_long(audio_lengths=, drop_finished=True)``: the batch plan (long_form.plan_drop -> ls_long_plan_drop), the
packed draws of RefDraws.windows(batches=), the refusals raised before an engine exists and the ABI.  No GPU."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

from livelyspeaker_amd import _lib, long_form, ref_draws, synth
from test_long_form_host import _no_engine, _parts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def lengths_for(windows, cfg):
    """Audio lengths that need exactly these window counts, through plan_windows' arithmetic: W windows cover up to
    audio_len + (W - 1) * 32000 samples; 1000 samples less still needs the W-th window."""
    lens = [cfg.audio_len + (int(W) - 1) * long_form.AUDIO_STRIDE - 1000 for W in windows]
    assert [W for W, _ in long_form.plan_lengths(lens, cfg)] == [int(W) for W in windows]
    return np.array(lens, np.int64)


@pytest.mark.parametrize("ds", ["ted", "beat"])
def test_plan_drop_table(ds):
    cfg = synth.CONFIGS[ds]
    order, windows, active, offsets = long_form.plan_drop(lengths_for([2, 3, 1, 3, 1], cfg), cfg)
    assert order.tolist() == [1, 3, 0, 2, 4]                        # a stable sort, longest first: ties keep the caller's order
    assert windows.tolist() == [3, 3, 2, 1, 1]
    assert active.tolist() == [5, 3, 2] and offsets.tolist() == [0, 5, 8, 10]
    # window w runs the clips with W_b > w, and they are the slots [0, B_w)
    for w, n in enumerate(active):
        assert sorted(order[:n].tolist()) == [b for b, W in enumerate([2, 3, 1, 3, 1]) if W > w]
    order, windows, active, offsets = long_form.plan_drop(lengths_for([2, 2, 2, 2], cfg), cfg)
    assert order.tolist() == [0, 1, 2, 3] and active.tolist() == [4, 4] and offsets.tolist() == [0, 4, 8]
    order, windows, active, offsets = long_form.plan_drop(lengths_for([3], cfg), cfg)
    assert order.tolist() == [0] and windows.tolist() == [3] and active.tolist() == [1, 1, 1] and offsets.tolist() == [0, 1, 2, 3]
    AL = cfg.audio_len
    order, windows, active, offsets = long_form.plan_drop([AL, AL + 1, 1, AL + long_form.AUDIO_STRIDE, AL + long_form.AUDIO_STRIDE + 1], cfg)
    assert windows[np.argsort(order)].tolist() == [1, 2, 1, 2, 3]   # per clip: exactly audio_len is one window, one sample more is two
    assert [W for W, _ in long_form.plan_lengths([AL, AL + 1, 1, AL + long_form.AUDIO_STRIDE, AL + long_form.AUDIO_STRIDE + 1], cfg)] == [1, 2, 1, 2, 3]
    assert order.tolist() == [4, 1, 3, 0, 2] and active.tolist() == [5, 3, 1]
    for bad in ([], [0], [5, -1]):
        with pytest.raises(ValueError):
            long_form.plan_drop(bad, cfg)


def test_plan_drop_agrees_with_plan_lengths_on_random_lengths():
    cfg = synth.TED
    rng = np.random.Generator(np.random.PCG64(3))
    lens = rng.integers(1, cfg.audio_len + 6 * long_form.AUDIO_STRIDE, size=37)
    order, windows, active, offsets = long_form.plan_drop(lens, cfg)
    W = np.array([w for w, _ in long_form.plan_lengths(lens, cfg)])
    assert order.tolist() == np.argsort(-W, kind="stable").tolist() and windows.tolist() == W[order].tolist()
    assert active.tolist() == [int((W > w).sum()) for w in range(int(W.max()))] and offsets[-1] == W.sum()


@pytest.mark.parametrize("native", [True, False])
def test_ref_draws_windows_with_batches_is_one_call_per_window(native):
    cfg, _, diffusion = _parts("ted")
    diffusion.native_host_rng = native
    n_exec, D, rest, batches = 4, 512, (cfg.njoints, cfg.nfeats, cfg.nframes), [5, 3, 2]
    torch.manual_seed(11)
    x, eps, nz = ref_draws.RefDraws("cpu").windows(diffusion, 3, n_exec, (5,) + rest, D, batches=batches)
    state = torch.get_rng_state()
    torch.manual_seed(11)
    parts = [ref_draws.RefDraws("cpu").windows(diffusion, 1, n_exec, (n,) + rest, D) for n in batches]
    assert torch.equal(torch.get_rng_state(), state)              # the generator ends where the three calls leave it
    assert x.shape == (10,) + rest and torch.equal(x, torch.cat([p[0][0] for p in parts]))
    assert eps.shape == (10 * n_exec * 2 * D,) and torch.equal(eps, torch.cat([p[1].reshape(-1) for p in parts]))
    assert nz.shape == (10 * n_exec * int(np.prod(rest)),) and torch.equal(nz, torch.cat([p[2].reshape(-1) for p in parts]))
    assert parts[1][1].shape == (1, n_exec, 2, 3, D) and not torch.equal(parts[0][0][0, :2], parts[2][0][0])
    # without batches nothing changed
    torch.manual_seed(11)
    a = ref_draws.RefDraws("cpu").windows(diffusion, 2, n_exec, (3,) + rest, D)
    torch.manual_seed(11)
    b = ref_draws.RefDraws("cpu").windows(diffusion, 2, n_exec, (3,) + rest, D, batches=[3, 3])
    assert a[0].shape == (2, 3) + rest and a[1].shape == (2, n_exec, 2, 3, D)
    assert all(torch.equal(p.reshape(-1), q.reshape(-1)) for p, q in zip(a, b))
    with pytest.raises(ValueError):
        ref_draws.RefDraws("cpu").windows(diffusion, 3, n_exec, (5,) + rest, D, batches=[5, 3])


@pytest.mark.parametrize("ds", ["ted", "beat"])
def test_drop_finished_refusals_come_before_any_engine(ds, monkeypatch):
    _no_engine(monkeypatch)
    cfg, model, diffusion = _parts(ds)
    y = synth.make_long_cond(cfg, 2, 2)
    emo = {"emo": y["emo"]} if ds == "beat" else {}
    lens = lengths_for([2, 1], cfg)

    def call(**kw):
        return long_form.sample_long(diffusion, model, y["audio"], y["seed_poses"], y["vid_indices"], y["scale"], **emo, **kw)

    with pytest.raises(ValueError, match="audio_lengths"):
        call(drop_finished=True)
    with pytest.raises(ValueError):
        call(drop_finished=True, audio_lengths=lens, n_windows=2)
    for bad in (lens[:1], [0, 5], [5, y["audio"].shape[1] + 1]):
        with pytest.raises(ValueError):
            call(drop_finished=True, audio_lengths=bad)
    with pytest.raises(ValueError):
        call(drop_finished=True, audio_lengths=lens, sampler="plms")
    with pytest.raises(NotImplementedError):
        call(drop_finished=True, audio_lengths=lens, const_noise=True)
    diffusion.noise_source = "torch_device"
    with pytest.raises(NotImplementedError):
        call(drop_finished=True, audio_lengths=lens)
    diffusion.noise_source = "torch_cpu"
    with pytest.raises(TypeError):
        long_form.sample_long(diffusion, model.model, y["audio"], y["seed_poses"], y["vid_indices"], y["scale"], audio_lengths=lens,
                              drop_finished=True, **emo)


def test_library_exports_the_ragged_prepare_and_keeps_its_abi(tmp_path):
    lib = _lib.load_library()
    assert lib.ls_abi_version() == 5
    hdr = open(os.path.join(ROOT, "include", "ls_hip.h")).read()
    for name in ("ls_long_prepare_ragged", "ls_long_plan_drop"):
        assert name in _lib.EXPORTS and f"int {name}(" in hdr and hasattr(lib, name), name
    # no existing struct changed layout: the sizes the long-form ABI had before the ragged entry
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include "ls_hip.h"\nint main(void) {\n'
                   '    printf("%zu %zu %d\\n", sizeof(ls_long_cond), sizeof(ls_long_sample_args), LS_ABI_VERSION);\n    return 0;\n}\n')
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [64, 104, 5]
    assert ctypes.sizeof(_lib.LsLongCond) == 64 and ctypes.sizeof(_lib.LsLongSampleArgs) == 104
