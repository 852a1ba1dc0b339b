"""Host side of the scripted timeline edit (``long_form.edit_long(sag=, text_features=)`` -> ls_long_edit_sag): ``edit_start`` against
``torch.where`` on the masks ``edit_window`` gives, the refusals raised before an engine exists, and the ABI.  No GPU."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

from livelyspeaker_amd import _lib, long_form, synth
from livelyspeaker_amd.cfg_sampler import ClassifierFreeSampleModel
from livelyspeaker_amd.motionclip_module import Decoder_TRANSFORMER

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T, NPRE, S = 34, 4, 30
RANGES = np.array([(20, 50), (0, 0), (70, 80)])             # across the seam 33/34, an untouched clip, inside window 2


def _parts(ds):
    from types import SimpleNamespace
    from livelyspeaker_amd.model_util import create_model_and_diffusion
    cfg = synth.CONFIGS[ds]
    args = SimpleNamespace(mdm_condm="text", latent_dim=512, ff_size=1024, layers=8, cond_mask_prob=0.1, arch="trans_enc",
                           emb_trans_dec=False, dataset="humanml", lang_model=None, mlpact="silu", diffusion_steps=6,
                           noise_schedule="cosine", sigma_small=True, lambda_vel=1.0, lambda_rcxyz=0.0, lambda_fc=0.0, njoints=cfg.njoints)
    model, diffusion = create_model_and_diffusion(args, "", dataset=ds)
    return cfg, ClassifierFreeSampleModel(model), diffusion


def _no_engine(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("an engine was created before the arguments were checked")
    monkeypatch.setattr(_lib.Engine, "__init__", boom)
    monkeypatch.setattr(_lib.SagEngine, "__init__", boom)


@pytest.mark.parametrize("ds", ["ted", "beat"])
def test_edit_start_is_where_on_the_masks_of_edit_window(ds):
    cfg = synth.CONFIGS[ds]
    B, J, F, W = 3, cfg.njoints, cfg.nfeats, 3
    N = T + (W - 1) * S
    g = torch.Generator().manual_seed(3)
    timeline = torch.randn(B, J, F, N, generator=g)
    seed = torch.randn(B, J, F, NPRE, generator=g)
    joints = np.ones((B, J), bool)
    joints[2] = False
    joints[2, [1, J - 2]] = True
    assert long_form.edit_plan(RANGES, W, cfg) == [0, 1, 2]
    for w in range(W):
        _, mask, motion = long_form.edit_window(timeline, w, RANGES, joints, seed, cfg)
        sag_out = torch.randn(B, J, F, T, generator=g)
        start = long_form.edit_start(motion, mask, sag_out)
        assert start.shape == motion.shape and start.dtype == motion.dtype
        assert torch.equal(start, torch.where(mask, motion, sag_out))
        assert torch.equal(start[mask], motion[mask]) and torch.equal(start[~mask], sag_out[~mask])
        assert torch.equal(start[1], motion[1])                    # the clip that keeps everything starts from its slice, bit for bit
        assert bool(mask.any()) and not bool(mask.all())
        if w > 0:                                                  # a later window keeps its first n_pre frames: they start from the slice
            assert torch.equal(start[..., :NPRE], motion[..., :NPRE])
        assert torch.equal(start[2, 0], motion[2, 0])              # clip 2: a joint that is not selected starts from the slice
        if w == 2:                                                 # ... and a selected one from the decoder on frames 70..79 only
            assert torch.equal(start[2, 1, :, 10:20], sag_out[2, 1, :, 10:20]) and torch.equal(start[2, 1, :, 20:], motion[2, 1, :, 20:])
    # window 1 of clip 0: frames 4..19 are editable (34..49), the rest kept
    _, mask, motion = long_form.edit_window(timeline, 1, RANGES, joints, seed, cfg)
    sag_out = torch.full_like(motion, 7.0)
    start = long_form.edit_start(motion, mask, sag_out)
    assert bool((start[0, :, :, 4:20] == 7.0).all()) and torch.equal(start[0, :, :, :4], motion[0, :, :, :4]) and torch.equal(start[0, :, :, 20:], motion[0, :, :, 20:])
    with pytest.raises(ValueError):
        long_form.edit_start(motion, mask[:, :1], sag_out)
    with pytest.raises(ValueError):
        long_form.edit_start(motion, mask.float(), sag_out)


def _decoder(cfg, **over):
    kw = dict(njoints=cfg.njoints, nfeats=cfg.nfeats, latent_dim=512, n_pre_poses=4, use_style=False)
    kw.update(over)
    return Decoder_TRANSFORMER(**kw)


@pytest.mark.parametrize("ds", ["ted", "beat"])
def test_scripted_edit_refusals_come_before_any_engine(ds, monkeypatch):
    _no_engine(monkeypatch)
    cfg, model, diffusion = _parts(ds)
    B, Wn = 2, 2
    y = synth.make_long_cond(cfg, B, Wn)
    emo = {"emo": y["emo"]} if ds == "beat" else {}
    timeline = np.zeros((B, cfg.njoints, cfg.nfeats, T + S), np.float32)
    sag = _decoder(cfg)
    text = synth.make_text_features(B * Wn).reshape(B, Wn, 512)

    def call(**kw):
        return long_form.edit_long(diffusion, model, timeline, (10, 40), y["audio"], y["seed_poses"], y["vid_indices"], y["scale"], **emo, **kw)

    with pytest.raises(ValueError, match="text_features without sag"):
        call(text_features=text)
    with pytest.raises(ValueError, match="sag needs text_features"):
        call(sag=sag)
    for bad in (text[:, :1], text[:1], text[..., :511], text[:, :, None], text[0, 0], text[:, 0, :511], np.zeros((B + 1, 512), np.float32)):
        with pytest.raises(ValueError, match="text_features must be"):
            call(sag=sag, text_features=bad)
    other = "beat" if ds == "ted" else "ted"
    with pytest.raises(ValueError, match="do not match"):
        call(sag=_decoder(synth.CONFIGS[other]), text_features=text)
    with pytest.raises(ValueError, match="do not match"):
        call(sag=_decoder(cfg, n_pre_poses=3), text_features=text)
    # what edit_long refuses without a script it refuses with one
    with pytest.raises(ValueError, match="empty"):
        long_form.edit_long(diffusion, model, timeline, (7, 7), y["audio"], y["seed_poses"], y["vid_indices"], y["scale"], **emo, sag=sag,
                            text_features=text)
    # both forms are accepted up to the point where the engine would be bound: the bind itself fails, by the patch above, or, where
    # no GPU is visible, by the model's own refusal just ahead of it
    bind = dict(expected_exception=(AssertionError, _lib.EngineError), match="an engine was created|no MI355X visible")
    for ok in (text, text[:, 0], torch.from_numpy(text), torch.from_numpy(text[:, 0].copy())):
        with pytest.raises(**bind):
            call(sag=sag, text_features=ok)
    with pytest.raises(**bind):
        call()                                                              # ... where the unscripted edit arrives as well


def test_the_entry_is_exported_and_the_abi_is_unchanged(tmp_path):
    lib = _lib.load_library()
    assert lib.ls_abi_version() == 5
    hdr = open(os.path.join(ROOT, "include", "ls_hip.h")).read()
    assert "ls_long_edit_sag" in _lib.EXPORTS and "int ls_long_edit_sag(" in hdr and hasattr(lib, "ls_long_edit_sag")
    assert "int ls_long_edit(" in hdr and hasattr(lib, "ls_long_edit")
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "ls_hip.h"\nint main(void) {\n'
                   '    int (*entry)(ls_handle*, const ls_long_edit_args*, struct ls_sag*, const float*) = 0;\n'
                   '    if (0) entry = ls_long_edit_sag;       /* the declaration has this type */\n'
                   '    printf("%zu %zu %zu %d %d\\n", sizeof(ls_long_edit_args), sizeof(ls_long_cond), sizeof(ls_long_sample_args), LS_ABI_VERSION, entry == 0);\n'
                   '    return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-O1", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    sizes = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert sizes[:4] == [ctypes.sizeof(_lib.LsLongEditArgs), 64, 104, 5]
    assert ctypes.sizeof(_lib.LsLongEditArgs) == 144                       # as on the parent commit: no field was added for the decoder
    import inspect
    params = inspect.signature(_lib.Engine.long_edit).parameters
    assert "sag" in params and "text_features" in params and params["sag"].default is None
