"""SAG encoder and the MOTIONCLIP encode-decode path: the float64 restatement vs the golden fixture G19 from the imported reference
(CPU), the drop-in modules' contracts (CPU), HIP vs fixture / restatement and the chained path (GPU).

Tolerances are the SAG decoder's (tests/test_sag.py): restatement vs reference < 2e-5 (the reference's own fp32 rounding against
float64 is 1.6e-6), HIP vs reference < 1e-4.  The fixture generator asserts that a dropped mask moves mu of the ragged rows by > 0.1
and a wrong query token by > 0.1, so neither can hide under these bounds."""
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, max_abs
from livelyspeaker_amd import synth
from sag_encoder_restatement import SagEncoderRestatement, motion_text_cosine as cosine_restated

DATASETS = {"ted": (synth.TED, "sag_enc_golden.npz"), "beat": (synth.BEAT, "sag_enc_beat_golden.npz")}
NEW_NAMES = ("ls_sag_enc_create", "ls_sag_enc_destroy", "ls_sag_enc_last_error", "ls_sag_enc_set_weight", "ls_sag_enc_commit_weights",
             "ls_sag_enc_encode", "ls_sag_enc_encode_async", "ls_sag_enc_last_encode_ms", "ls_sag_enc_stream")


def _g19(ds):
    return np.load(os.path.join(GOLDEN, DATASETS[ds][1]))


def _x(cfg, B=6):
    return synth.make_cond(cfg, B)["origin_x"]


def _restatement(cfg):
    return SagEncoderRestatement(synth.make_sag_encoder_state_dict(cfg), cfg.njoints, cfg.nfeats)


def _sag_cfg():
    return SimpleNamespace(n_pre_poses=4, use_style=False)


def _torch_sd(sd):
    import torch
    return {k: torch.from_numpy(v) for k, v in sd.items()}


# ---------------------------------------------------------------- CPU ----------------------------------------------------------------
@pytest.mark.parametrize("ds", ["ted", "beat"])
def test_restatement_matches_reference_fixture(ds):
    cfg, g = DATASETS[ds][0], _g19(ds)
    rest, x = _restatement(cfg), _x(cfg)
    for tag, mask in (("all", None), ("ragged", g["G19_mask_ragged"])):
        full, pruned = rest.encode(x, mask), rest.encode(x, mask, pruned=True)
        d_full, d_pruned, d_forms = max_abs(full, g[f"G19_mu_{tag}"]), max_abs(pruned, g[f"G19_mu_{tag}"]), max_abs(full, pruned)
        print(f"{ds} restatement vs reference mu_{tag}: full {d_full:.3e} pruned {d_pruned:.3e}; full vs pruned {d_forms:.3e}")
        assert d_full < 2e-5 and d_pruned < 2e-5
        assert d_forms < 1e-12
    # an explicit all-true mask is the same function as no mask
    assert np.array_equal(rest.encode(x, np.ones((6, 34), dtype=bool)), rest.encode(x, None))


@pytest.mark.parametrize("ds", ["ted", "beat"])
def test_restatement_chained_with_decoder_oracle(ds):
    from oracle import rag_oracle as orc
    cfg, g = DATASETS[ds][0], _g19(ds)
    x, mask = _x(cfg), g["G19_mask_ragged"]
    z = _restatement(cfg).encode(x, mask)
    dec = orc.SagDecoderOracle(synth.make_sag_state_dict(cfg), njoints=cfg.njoints, nfeats=cfg.nfeats)
    d = max_abs(dec.decode(x, z, mask), g["G19_ae_ragged"])
    print(f"{ds} restatement + decoder oracle vs reference MOTIONCLIP.forward: {d:.3e}")
    assert d < 2e-5


@pytest.mark.parametrize("ds", ["ted", "beat"])
def test_encoder_state_dict_contract(ds):
    from livelyspeaker_amd.motionclip_module import Encoder_TRANSFORMER
    cfg = DATASETS[ds][0]
    enc = Encoder_TRANSFORMER(njoints=cfg.njoints, nfeats=cfg.nfeats, latent_dim=512)
    want = synth.make_sag_encoder_state_dict(cfg)
    have = {k: tuple(v.shape) for k, v in enc.state_dict().items()}
    assert set(have) == set(want) | {"sequence_pos_encoder.pe"}
    assert all(have[k] == want[k].shape for k in want)
    assert not any(p.requires_grad for p in enc.parameters())
    with pytest.raises(NotImplementedError):
        Encoder_TRANSFORMER(latent_dim=512, activation="relu")


def test_get_sag_loads_checkpoint_layout():
    from livelyspeaker_amd.motionclip import MOTIONCLIP, get_SAG
    from livelyspeaker_amd.motionclip_module import Decoder_TRANSFORMER, Encoder_TRANSFORMER
    sag, text_encoder = get_SAG(_sag_cfg())
    assert text_encoder is None
    assert isinstance(sag, MOTIONCLIP) and isinstance(sag.encoder, Encoder_TRANSFORMER) and isinstance(sag.decoder, Decoder_TRANSFORMER)
    assert sag.promptLearner is None and sag.decoder.n_pre_poses == 4
    ckpt = synth.make_sag_checkpoint()
    assert all(k.startswith(("encoder.", "decoder.")) for k in ckpt)
    missing, unexpected = sag.load_state_dict(_torch_sd(ckpt), strict=False)
    assert not unexpected
    assert sorted(missing) == ["decoder.sequence_pos_encoder.pe", "encoder.sequence_pos_encoder.pe"]
    import torch
    assert torch.equal(sag.encoder.muQuery, torch.from_numpy(ckpt["encoder.muQuery"]))
    with pytest.raises(NotImplementedError):
        sag.compute_loss({}, None)


def test_seeded_construction_reproduces_reference_init():
    import torch
    from livelyspeaker_amd.motionclip_module import Encoder_TRANSFORMER
    g = _g19("ted")
    torch.manual_seed(0)
    enc = Encoder_TRANSFORMER(latent_dim=512)
    assert np.array_equal(enc.muQuery.numpy()[0, :8], g["G19_init_muQuery"])
    assert np.array_equal(enc.sigmaQuery.numpy()[0, :8], g["G19_init_sigmaQuery"])
    assert np.array_equal(enc.skelEmbedding.weight.numpy()[:4, :8], g["G19_init_skelEmbedding_weight"])
    # the last matrix drawn: the transformer layers consume the generator in the reference's order after the three above
    assert np.array_equal(enc.seqTransEncoder.layers[2].linear2.weight.numpy()[:4, :8], g["G19_init_last_linear2_weight"])


@pytest.mark.parametrize("ds", ["ted", "beat"])
def test_motion_text_cosine(ds):
    import torch
    from livelyspeaker_amd.motionclip import motion_text_cosine
    g = _g19(ds)
    text = synth.make_text_features(6)
    cos = motion_text_cosine(torch.from_numpy(g["G19_mu_all"]), torch.from_numpy(text))
    assert tuple(cos.shape) == (6,)
    d = max_abs(cos.numpy(), g["G19_cos"])
    print(f"{ds} motion_text_cosine vs reference: {d:.3e}")
    assert d < 1e-6
    assert max_abs(cosine_restated(g["G19_mu_all"], text), g["G19_cos"]) < 1e-6


def test_lengths_to_mask():
    import torch
    from livelyspeaker_amd.motionclip import MOTIONCLIP
    lengths = torch.tensor([34, 30, 20])
    got = MOTIONCLIP.lengths_to_mask(lengths)
    assert got.dtype == torch.bool and torch.equal(got, torch.arange(34)[None, :] < lengths[:, None])


def test_header_exports_and_abi():
    from livelyspeaker_amd import _lib
    with open(os.path.join(ROOT, "include", "ls_hip.h")) as f:
        declared = set(re.findall(r"\b(ls_[a-z_]+)\s*\(", f.read()))
    for name in NEW_NAMES:
        assert name in declared, name
        assert name in _lib.EXPORTS, name
    lib = _lib.load_library()
    assert lib.ls_abi_version() == 5
    for name in NEW_NAMES:
        assert hasattr(lib, name), name


# ---------------------------------------------------------------- GPU ----------------------------------------------------------------
def _engine(cfg):
    from livelyspeaker_amd import _lib
    eng = _lib.SagEncoderEngine(cfg.njoints, cfg.nfeats)
    eng.load_state_dict(synth.make_sag_encoder_state_dict(cfg))
    return eng


@pytest.mark.gpu
@pytest.mark.parametrize("ds", ["ted", "beat"])
def test_hip_encoder_vs_golden(ds):
    cfg, g = DATASETS[ds][0], _g19(ds)
    x, mask = _x(cfg), g["G19_mask_ragged"]
    eng = _engine(cfg)
    try:
        mu_all, mu_rag = eng.encode(x), eng.encode(x, mask)
        d_all, d_rag = max_abs(mu_all, g["G19_mu_all"]), max_abs(mu_rag, g["G19_mu_ragged"])
        print(f"{ds} SAG encoder vs reference: all {d_all:.3e} ragged {d_rag:.3e}")
        assert mu_all.shape == (6, 512) and mu_all.dtype == np.float32
        assert d_all < 1e-4 and d_rag < 1e-4
        assert np.array_equal(eng.encode(x, np.ones((6, 34), dtype=bool)), mu_all)
        # frames behind the mask are never read through a non-zero probability: rewriting them changes nothing, bit for bit
        x_over = x.copy()
        x_over[1, :, :, 30:] = 7.0
        x_over[4, :, :, 20:] = -3.0
        assert np.array_equal(eng.encode(x_over, mask), mu_rag)
        # ... and the mask is really applied: the ragged rows differ from the all-true result, the others do not
        moved = np.abs(mu_all - mu_rag).max(axis=1)
        print(f"{ds} mask effect per row: {np.array2string(moved, precision=3)}")
        assert moved[1] > 0.1 and moved[4] > 0.1
        assert np.array_equal(mu_all[[0, 2, 3, 5]], mu_rag[[0, 2, 3, 5]])
        assert eng.last_encode_ms() > 0.0
    finally:
        eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("ds", ["ted", "beat"])
def test_hip_encoder_caller_batch(ds):
    """B = 512 (the callers' batch): spot rows against the restatement, and batch-composition independence -- the same clips
    encoded as a batch of 3 run the full GEMMs at M = 108 and the pruned last layer's at M = 3 instead of 18432 and 512."""
    cfg = DATASETS[ds][0]
    B, pick = 512, [0, 255, 511]
    x = _x(cfg, B)
    mask = np.ones((B, 34), dtype=bool)
    mask[255, 17:] = False
    eng = _engine(cfg)
    try:
        big = eng.encode(x, mask)
        d = max_abs(big[pick], _restatement(cfg).encode(x[pick], mask[pick]))
        print(f"{ds} SAG encoder B = 512 rows {pick} vs restatement: {d:.3e}; encode {eng.last_encode_ms():.3f} ms")
        assert d < 1e-4
        assert np.array_equal(eng.encode(x[pick], mask[pick]), big[pick])
    finally:
        eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("ds", ["ted", "beat"])
def test_motionclip_forward(ds):
    import torch
    from livelyspeaker_amd import _lib
    from livelyspeaker_amd.motionclip import MOTIONCLIP, get_SAG
    from livelyspeaker_amd.motionclip_module import Decoder_TRANSFORMER, Encoder_TRANSFORMER
    cfg, g = DATASETS[ds][0], _g19(ds)
    dev = "cuda:0"
    if ds == "ted":
        sag, _ = get_SAG(_sag_cfg())
    else:           # get_SAG builds the variant's defaults; BEAT's shapes go through the constructors
        sag = MOTIONCLIP(Encoder_TRANSFORMER(njoints=cfg.njoints, nfeats=cfg.nfeats, latent_dim=512),
                         Decoder_TRANSFORMER(njoints=cfg.njoints, nfeats=cfg.nfeats, latent_dim=512, n_pre_poses=4, use_style=False),
                         None, _sag_cfg())
    missing, unexpected = sag.load_state_dict(_torch_sd(synth.make_sag_checkpoint(cfg)), strict=False)
    assert not unexpected and all(k.endswith(".pe") for k in missing)
    sag = sag.to(dev).eval()
    x = torch.from_numpy(_x(cfg)).to(dev)
    mask = torch.from_numpy(g["G19_mask_ragged"]).to(dev)
    batch = sag({"x": x, "mask": mask})
    assert batch["z"] is batch["mu"] and batch["output_xyz"] is batch["output"]
    assert torch.equal(batch["final_z"], batch["mu"])            # the decoder's z.clone(), taken on torch's stream
    assert batch["mu"].is_cuda and tuple(batch["mu"].shape) == (6, 512)
    got = batch["output_xyz"].cpu().numpy()
    d_mu, d_ae = max_abs(batch["mu"].cpu().numpy(), g["G19_mu_ragged"]), max_abs(got, g["G19_ae_ragged"])
    print(f"{ds} MOTIONCLIP.forward vs reference: mu {d_mu:.3e} output_xyz {d_ae:.3e}")
    assert d_mu < 1e-4 and d_ae < 1e-4
    # the decoder alone, given that z, produces the same bits
    alone = sag.decoder({"x": x, "mask": mask, "z": batch["mu"].clone()})["output"].cpu().numpy()
    assert np.array_equal(alone, got)
    # the enqueue-only chain: encode, order the decoder's stream behind the encoder's, decode -- no host wait until the read
    enc, dec = sag.encoder.engine(), sag.decoder.engine()
    mu = enc.encode(x, mask, wait=False)
    _lib.stream_order(enc.device, enc._stream, dec._stream)
    out = dec.decode(x, mu, mask, wait=False)
    _lib.stream_order(dec.device, dec._stream, torch.cuda.current_stream().cuda_stream)
    assert np.array_equal(out.cpu().numpy(), got)
    qbatch = sag({"x": x, "mask": mask}, wait=False)                        # MOTIONCLIP.forward with the decode left enqueued
    assert torch.equal(qbatch["final_z"], qbatch["mu"]) and torch.equal(qbatch["mu"], batch["mu"])      # torch's stream is behind the encode
    queued = qbatch["output_xyz"]
    _lib.stream_order(dec.device, dec._stream, torch.cuda.current_stream().cuda_stream)
    assert np.array_equal(queued.cpu().numpy(), got)
    assert enc.last_encode_ms() > 0.0


@pytest.mark.gpu
def test_encode_batch_history_and_async_timing():
    """B = 2, then 5, then 2 on one engine: the buffers grow and are reused, the first and last results are the same bits; an enqueued
    encode (wait=False) reports its span once asked for."""
    import torch
    x = _x(synth.TED, 5)
    eng = _engine(synth.TED)
    try:
        first = eng.encode(x[:2])
        eng.encode(x)
        assert np.array_equal(eng.encode(x[:2]), first) and np.abs(first).max() > 0
        mu = eng.encode(torch.from_numpy(x[:2]).cuda(), wait=False)
        assert eng.last_encode_ms() > 0.0            # waits for the enqueued encode
        assert np.array_equal(mu.cpu().numpy(), first)
    finally:
        eng.close()


@pytest.mark.gpu
def test_reload_with_layers_exchanged():
    """The encoder reads its weights through pointers resolved at commit.  A second load_state_dict -- the same keys and shapes, every
    weight of layer 0 exchanged with the last layer's (the one that runs on token 0 only) -- re-resolves all of them: same bits as an
    engine that only ever saw it."""
    sd = synth.make_sag_encoder_state_dict(synth.TED)
    a, b = "seqTransEncoder.layers.0.", "seqTransEncoder.layers.2."
    other = {k: sd[b + k[len(a):]] if k.startswith(a) else sd[a + k[len(b):]] if k.startswith(b) else v for k, v in sd.items()}
    x = _x(synth.TED, 2)
    eng, fresh = _engine(synth.TED), _engine(synth.TED)
    try:
        first = eng.encode(x)
        eng.load_state_dict(other)
        second = eng.encode(x)
        fresh.load_state_dict(other)
        assert np.array_equal(second, fresh.encode(x))
        assert not np.array_equal(second, first)
    finally:
        eng.close()
        fresh.close()


@pytest.mark.gpu
def test_error_paths_reach_no_kernel():
    from livelyspeaker_amd import _lib
    cfg = synth.TED
    sd = synth.make_sag_encoder_state_dict(cfg)
    x = _x(cfg)
    eng = _lib.SagEncoderEngine()
    try:
        with pytest.raises(_lib.EngineError, match="before ls_sag_enc_commit_weights"):
            eng.encode(x)
        short = {k: v for k, v in sd.items() if k != "seqTransEncoder.layers.2.norm2.bias"}
        with pytest.raises(_lib.EngineError, match=r"missing weight 'seqTransEncoder\.layers\.2\.norm2\.bias'"):
            eng.load_state_dict(short)
        with pytest.raises(_lib.EngineError, match="before ls_sag_enc_commit_weights"):
            eng.encode(x)
        bad = dict(sd)
        bad["skelEmbedding.weight"] = sd["skelEmbedding.weight"][:, :20]
        with pytest.raises(_lib.EngineError, match=r"weight 'skelEmbedding\.weight' has 10240 elements, expected 13824"):
            eng.load_state_dict(bad)
        assert eng.lib.ls_sag_enc_commit_weights(eng.h) < 0 and b"skelEmbedding.weight" in eng.lib.ls_sag_enc_last_error(eng.h)
        eng.load_state_dict(sd)
        with pytest.raises(ValueError, match="mask must be"):
            eng.encode(x, np.ones((6, 36), dtype=bool))
        with pytest.raises(ValueError, match="mask must be"):
            eng.encode(x, np.ones((5, 34), dtype=bool))
        with pytest.raises(ValueError, match="x must be"):
            eng.encode(x[:, :, :, :33])
        with pytest.raises(ValueError, match="x must be"):
            eng.encode(_x(synth.BEAT))
        with pytest.raises(_lib.EngineError, match="needs device tensors"):
            eng.encode(x, wait=False)
        assert eng.encode(x).shape == (6, 512)          # the handle is still good after every refusal
    finally:
        eng.close()
