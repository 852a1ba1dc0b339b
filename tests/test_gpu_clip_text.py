"""CLIP text encoder on the GPU: the HIP path against the float64 restatement (tests/clip_text_restatement.py), the bitwise claims
of the packing (pruned = full, any batch composition, garbage behind EOT), token placement, chaining into the SAG decoder, errors.

The parity bound is made from the yardstick, not from the code under test: e32 = max|torch fp32 CPU forward - float64| on the same
inputs is what fp32 arithmetic itself costs on this network, and the HIP path may be 16 times that (its MFMA sums run in another
order, and softmax / QuickGELU use the hardware's exp and reciprocal where torch uses libm).

The measured ratios are in test_parity's docstring and in profiles/r13_clip_text.md."""
import functools

import numpy as np
import pytest
import torch

from clip_text_restatement import LENGTHS, LENGTHS_12, ClipTextRestatement, TorchClipText, state
from livelyspeaker_amd import _lib, clip_text, synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@functools.lru_cache(maxsize=None)
def _case(layers):
    """(tokens, float64 reference, e32) of the parity shapes -- computed once, shared, left unchanged"""
    sd = state(layers)
    tok = synth.synth_clip_tokens(LENGTHS if layers == 2 else LENGTHS_12)
    ref = ClipTextRestatement(sd).encode(tok, prune=False)
    e32 = float(np.abs(TorchClipText(sd, torch.float32)(tok).double().numpy() - ref).max())
    ref.setflags(write=False)
    tok.setflags(write=False)
    return tok, ref, e32


@functools.lru_cache(maxsize=None)
def _model(layers):
    m = clip_text.CLIPTextEncoder(transformer_layers=layers)
    clip_text.load_clip_text(m, {k: torch.as_tensor(v) for k, v in state(layers).items()})
    return m.to(DEV).eval()


def _junk_behind_eot(tok, lengths, seed=5):
    junk = np.array(tok)
    r = np.random.default_rng(seed)
    for b, n in enumerate(lengths):
        junk[b, n:] = r.integers(0, 49407, junk.shape[1] - n)
    return junk


@pytest.mark.parametrize("layers", [2, 12])
def test_parity(layers):
    """HIP error <= 16 e32, both forms.  Measured on an MI355X: 2 layers e32 3.29e-6, HIP 4.78e-6 (ratio 1.45); 12 layers e32 2.60e-6,
    HIP 4.73e-6 (ratio 1.82), the same in both forms (they agree bitwise)."""
    tok, ref, e32 = _case(layers)
    m = _model(layers)
    for prune in (True, False):
        out = m.encode_text(torch.as_tensor(np.array(tok)), prune=prune)
        assert out.is_cuda and out.dtype == torch.float32 and tuple(out.shape) == ref.shape
        err = float(np.abs(out.double().cpu().numpy() - ref).max())
        print(f"{layers} layers prune={prune}: max|out| {np.abs(ref).max():.3f}  e32 {e32:.3e}  HIP {err:.3e}  ratio {err / e32:.2f}  "
              f"encode {m.engine().last_encode_ms():.3f} ms")
        assert err <= 16 * e32


def test_pruned_equals_full_and_garbage_behind_eot_is_ignored():
    tok, _, _ = _case(2)
    m = _model(2)
    t = torch.as_tensor(np.array(tok))
    full, pruned = m.encode_text(t, prune=False), m.encode_text(t, prune=True)
    assert torch.equal(pruned, full)
    junk = torch.as_tensor(_junk_behind_eot(tok, LENGTHS))
    assert not torch.equal(junk, t)
    assert torch.equal(m.encode_text(junk, prune=True), full)
    assert torch.equal(m.encode_text(junk, prune=False), full)


def test_batch_composition():
    """130 sentences of 2 .. 40 tokens: the packed rows cross several 128-row GEMM tiles, and a sentence's rows start anywhere in
    one.  Each picked sentence encoded alone gives the same bits."""
    lengths = [int(n) for n in np.random.default_rng(11).integers(2, 41, 130)]
    assert sum(lengths) > 3 * 128
    tok = torch.as_tensor(synth.synth_clip_tokens(lengths, seed=77))
    m = _model(1)
    big = m.encode_text(tok)
    assert torch.isfinite(big).all()
    for b in (0, 1, 63, 64, 129):
        assert torch.equal(m.encode_text(tok[b:b + 1])[0], big[b]), b
    pick = [5, 99, 17]
    assert torch.equal(m.encode_text(tok[pick]), big[pick])
    assert torch.equal(m.encode_text(tok, prune=False), big)


def test_token_placement_and_chaining():
    from livelyspeaker_amd.motionclip_module import Decoder_TRANSFORMER
    tok, _, _ = _case(2)
    m = _model(2)
    host = torch.as_tensor(np.array(tok))
    want = m.encode_text(host)
    got = m.encode_text(host.to(DEV))
    assert got.is_cuda and torch.equal(got, want)
    assert torch.equal(m.encode_text(host.to(DEV).int()), want)          # any integer dtype
    assert torch.equal(m.encode_text(np.array(tok)), want)               # numpy ids
    # tokens -> features -> SAG decoder with no host wait between the two engines
    cfg = synth.TED
    dec = Decoder_TRANSFORMER(latent_dim=512, n_pre_poses=4, use_style=False)
    missing, unexpected = dec.load_state_dict({k: torch.as_tensor(v) for k, v in synth.make_sag_state_dict(cfg).items()}, strict=False)
    assert not unexpected and all(k.endswith(".pe") for k in missing)
    dec = dec.to(DEV).eval()
    B = host.shape[0]
    x = torch.from_numpy(synth.make_init_image(cfg, B)).to(DEV)
    mask = torch.ones(B, 34, dtype=torch.bool, device=DEV)
    waited = dec({"x": x, "z": want, "mask": mask})["output"].clone()
    for t in (host, host.to(DEV)):
        z = m.encode_text(t, wait=False)
        _lib.stream_order(0, m.engine()._stream, dec.engine()._stream)
        out = dec({"x": x, "z": z, "mask": mask})["output"]
        assert torch.equal(out, waited)
        assert torch.equal(z, want)
    assert m.engine().last_encode_ms() > 0.0


def test_reload_with_layers_exchanged():
    """The encoder reads its weights through pointers resolved at commit.  A second load_state_dict -- the same keys and shapes, every
    weight of block 0 exchanged with the last block's -- re-resolves all of them: same bits as an engine that only ever saw it."""
    sd = state(2)
    a, b = "transformer.resblocks.0.", "transformer.resblocks.1."
    other = {k: sd[b + k[len(a):]] if k.startswith(a) else sd[a + k[len(b):]] if k.startswith(b) else v for k, v in sd.items()}
    tok = np.array(_case(2)[0][:2])
    eng, fresh = _lib.ClipTextEngine(layers=2), _lib.ClipTextEngine(layers=2)
    try:
        eng.load_state_dict(sd)
        first = eng.encode(tok)
        eng.load_state_dict(other)
        second = eng.encode(tok)
        fresh.load_state_dict(other)
        assert np.array_equal(second, fresh.encode(tok))
        assert not np.array_equal(second, first)
    finally:
        eng.close()
        fresh.close()


def test_errors():
    tok, _, _ = _case(2)
    m = _model(2)
    t = torch.as_tensor(np.array(tok))
    assert torch.equal(m.encode_text(t[4:5]), m.encode_text(t)[4:5])     # B = 1
    bad = t.clone()
    bad[3, 50] = 49408                                                   # behind EOT, and still an error
    for src in (bad, bad.to(DEV)):
        with pytest.raises(_lib.EngineError, match="outside"):
            m.encode_text(src)
        with pytest.raises(_lib.EngineError, match="outside"):
            m.encode_text(src, wait=False)
    assert torch.equal(m.encode_text(t[4:5]), m.encode_text(t)[4:5])     # the handle works on after a refused call
    with pytest.raises((ValueError, _lib.EngineError)):
        m.encode_text(t[:, :76])
    with pytest.raises(TypeError):
        m.encode_text(t.float())
    eng = _lib.ClipTextEngine(layers=2)
    try:
        sd = dict(state(2))
        del sd["transformer.resblocks.1.attn.out_proj.bias"]
        with pytest.raises(_lib.EngineError, match="out_proj.bias"):
            eng.load_state_dict(sd)
        with pytest.raises(_lib.EngineError):
            eng.encode(np.array(tok))                                    # not committed
        with pytest.raises(_lib.EngineError, match="expected"):
            eng.load_state_dict(dict(state(2), **{"text_projection": np.zeros((512, 256), np.float32)}))
    finally:
        eng.close()
