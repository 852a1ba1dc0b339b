"""Host side of long-form synthesis (livelyspeaker_amd/long_form.py): the window plan, the audio windows, the exported symbols and
every refusal that is raised before an engine exists.  No GPU."""
import numpy as np
import pytest
import torch

from livelyspeaker_amd import _lib, long_form, synth
from livelyspeaker_amd.cfg_sampler import ClassifierFreeSampleModel
from livelyspeaker_amd.motionclip_module import Decoder_TRANSFORMER


@pytest.mark.parametrize("ds", ["ted", "beat"])
def test_plan_windows_table(ds):
    cfg = synth.CONFIGS[ds]
    AL = cfg.audio_len
    for L, W in ((AL, 1), (AL + 1, 2), (AL + 32000, 2), (AL + 32001, 3), (AL - 1000, 1), (1, 1), (AL + 29 * 32000, 30)):
        got = long_form.plan_windows(L, cfg)
        assert got == (W, AL + (W - 1) * 32000, 34 + (W - 1) * 30), (L, got)
        assert got[1] >= L or W == 1 and L <= AL                 # the padded waveform covers the given one
    with pytest.raises(ValueError):
        long_form.plan_windows(0, cfg)
    assert long_form.AUDIO_STRIDE == 32000 == 30 * 16000 // 15  # 30 frames at 15 fps of 16 kHz audio


@pytest.mark.parametrize("as_torch", [False, True])
def test_window_audio_is_the_slice_zero_padded(as_torch):
    cfg = synth.TED
    AL = cfg.audio_len
    L = AL + 2 * 32000 - 1000                                   # the third window runs 1000 samples past the end
    audio = np.random.Generator(np.random.PCG64(5)).standard_normal((3, L)).astype(np.float32)
    src = torch.from_numpy(audio) if as_torch else audio
    for w in range(3):
        got = np.asarray(long_form.window_audio(src, w, cfg))
        want = np.zeros((3, AL), np.float32)
        piece = audio[:, w * 32000:w * 32000 + AL]
        want[:, :piece.shape[1]] = piece
        assert got.shape == (3, AL) and np.array_equal(got, want), w
    assert np.array_equal(np.asarray(long_form.window_audio(src, 2, cfg))[:, -1000:], np.zeros((3, 1000), np.float32))
    assert np.asarray(long_form.window_audio(src, 5, cfg)).shape == (3, AL)          # wholly past the end: all padding
    assert not np.asarray(long_form.window_audio(src, 5, cfg)).any()


def test_make_long_cond_shapes():
    for ds in ("ted", "beat"):
        cfg = synth.CONFIGS[ds]
        y = synth.make_long_cond(cfg, 3, 3)
        assert y["audio"].shape == (3, cfg.audio_len + 2 * 32000) and y["seed_poses"].shape == (3, cfg.njoints, cfg.nfeats, 4)
        assert long_form.plan_windows(y["audio"].shape[1], cfg)[0] == 3
        assert ("emo" in y) == (ds == "beat") and (ds == "ted" or y["emo"].shape == (3, 3))
        again = synth.make_long_cond(cfg, 3, 3)
        assert all(np.array_equal(y[k], again[k]) for k in y)


def test_library_exports_the_long_form_symbols_and_keeps_its_abi():
    lib = _lib.load_library()
    assert lib.ls_abi_version() == 5
    for name in ("ls_long_prepare", "ls_long_sample"):
        assert name in _lib.EXPORTS and hasattr(lib, name)
    assert hasattr(_lib.Engine, "long_prepare") and hasattr(_lib.Engine, "long_sample")


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
def test_argument_refusals_come_before_any_engine(ds, monkeypatch):
    _no_engine(monkeypatch)
    cfg, model, diffusion = _parts(ds)
    y = synth.make_long_cond(cfg, 2, 2)
    emo = {"emo": y["emo"]} if ds == "beat" else {}

    def call(**over):
        kw = dict(audio=y["audio"], seed_poses=y["seed_poses"], vid_indices=y["vid_indices"], scale=y["scale"], **emo)
        kw.update(over)
        return long_form.sample_long(diffusion, model, kw.pop("audio"), kw.pop("seed_poses"), kw.pop("vid_indices"), kw.pop("scale"), **kw)

    bad = [dict(audio=y["audio"][0]), dict(audio=y["audio"][:, :, None]),                            # wrong ranks
           dict(vid_indices=y["vid_indices"][:, None]), dict(scale=y["scale"][:1]),
           dict(n_windows=0), dict(n_windows=-2),                                                    # W < 1
           dict(seed_poses=y["seed_poses"][..., :3]), dict(seed_poses=y["seed_poses"][:, :, :, :, None]),
           dict(seed_poses=np.zeros((2, cfg.njoints, cfg.nfeats, 34), np.float32)),                  # a whole origin_x is not the seed
           dict(text_features=np.zeros((2, 2, 512), np.float32)),                                    # text_features without sag
           dict(sampler="plms"), dict(skip_timesteps=6), dict(encoder_chunk=0)]
    if ds == "beat":
        bad += [dict(emo=None), dict(emo=y["emo"][:, :1]), dict(emo=y["emo"][:, :, None])]
    else:
        bad += [dict(emo=np.zeros(2, np.int64))]
    for over in bad:
        with pytest.raises(ValueError):
            call(**over)
    # the unsupported noise modes and keys: refused when the call is made
    for over in (dict(const_noise=True), dict(dump_steps=[0]), dict(inpainting_mask=np.ones((2, 1), bool)),
                 dict(inpainted_motion=np.zeros((2, 1), np.float32))):
        with pytest.raises(NotImplementedError):
            call(**over)
    diffusion.noise_source = "torch_device"
    with pytest.raises(NotImplementedError):
        call()
    diffusion.noise_source = "nonsense"
    with pytest.raises(ValueError):
        call()
    diffusion.noise_source = "torch_cpu"
    with pytest.raises(TypeError):
        call(no_such_option=1)
    with pytest.raises(TypeError):
        long_form.sample_long(diffusion, model.model, y["audio"], y["seed_poses"], y["vid_indices"], y["scale"], **emo)
    if ds == "ted":                                                                                  # sag: missing / misshapen text features
        sag = Decoder_TRANSFORMER(latent_dim=512, n_pre_poses=4, use_style=False)
        for tf in (None, np.zeros((2, 512), np.float32), np.zeros((2, 3, 512), np.float32)):
            with pytest.raises(ValueError):
                call(sag=sag, text_features=tf)
        with pytest.raises(ValueError):
            call(sag=Decoder_TRANSFORMER(latent_dim=512, n_pre_poses=2), text_features=np.zeros((2, 2, 512), np.float32))


@pytest.mark.parametrize("ds", ["ted", "beat"])
def test_oracle_chain_restates_the_reference_chain(ds):
    """Fixture G22 (tests/golden/make_golden_long.py: the reference's own loops and decoder, one call per window, W = 3, B = 2) against
    oracle.rag_oracle.sample_loop / SagDecoderOracle chained the same way.  1e-4 is the tolerance tests/test_oracle_golden.py uses for
    loops of this length; the generator measured at most 7.2e-6 on any window (profiles/r12_long_form.md)."""
    import os

    import long_form_restatement as lfr
    from conftest import GOLDEN, max_abs
    g = np.load(os.path.join(GOLDEN, f"{ds}_golden_long.npz"))
    cfg = synth.CONFIGS[ds]
    for case in lfr.CASES:
        timeline, wins = lfr.oracle_chain(cfg, case)
        want = g[f"G22_{case}_timeline"]
        assert timeline.shape == want.shape == (lfr.B, cfg.njoints, cfg.nfeats, 34 + 2 * 30)
        d = max_abs(timeline, want)
        print(f"{ds} G22_{case}: oracle chain vs reference {d:.3e}")
        assert d < 1e-4, (case, d)
        # window 1's prefix is window 0's tail: the stitched timeline holds every window's conditioning
        assert np.array_equal(wins[1][..., 4:], timeline[..., 34:64]) and np.array_equal(wins[0], timeline[..., :34])
