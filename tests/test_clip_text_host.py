"""CLIP text encoder, the part that needs no GPU: the float64 restatement (both forms) against torch's own layers, the claim the
packing rests on (nothing behind EOT reaches the result), the host plan against torch.argmax, the module's key layout and loader,
and the ABI additions."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from clip_text_restatement import LENGTHS, LENGTHS_12, ClipTextRestatement, TorchClipText, state
from livelyspeaker_amd import _lib, clip_text, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ls_clip_text_create", "ls_clip_text_destroy", "ls_clip_text_last_error", "ls_clip_text_set_weight", "ls_clip_text_commit_weights",
       "ls_clip_text_encode", "ls_clip_text_encode_async", "ls_clip_text_last_encode_ms", "ls_clip_text_stream", "ls_clip_text_plan")


@pytest.mark.parametrize("layers,lengths", [(2, LENGTHS), (12, LENGTHS_12)])
def test_restatement_matches_torch_float64(layers, lengths):
    """Bound: 1e-9 of the output's magnitude, about 1e6 float64 roundings -- far above what two orderings of the same sums differ
    by and far below any error of substance.  The two forms of the restatement differ by summation lengths alone: < 1e-12."""
    sd = state(layers)
    tok = synth.synth_clip_tokens(lengths)
    rest = ClipTextRestatement(sd)
    want = TorchClipText(sd, torch.float64)(tok).numpy()
    pruned, full = rest.encode(tok, prune=True), rest.encode(tok, prune=False)
    scale = np.abs(want).max()
    d_p, d_f, d_forms = np.abs(pruned - want).max(), np.abs(full - want).max(), np.abs(pruned - full).max()
    print(f"{layers} layers: max|out| {scale:.3f}; pruned vs torch {d_p:.3e}, full vs torch {d_f:.3e}, pruned vs full {d_forms:.3e}")
    assert d_p <= 1e-9 * scale and d_f <= 1e-9 * scale
    assert d_forms < 1e-12


def test_garbage_behind_eot_changes_nothing():
    """Ids below 49407 behind EOT: the argmax stays, the causal mask keeps them from every row up to EOT -- exactly, in both forms."""
    sd = state(2)
    tok = synth.synth_clip_tokens(LENGTHS)
    junk = tok.copy()
    r = np.random.default_rng(5)
    for b, n in enumerate(LENGTHS):
        junk[b, n:] = r.integers(0, 49407, 77 - n)
    assert (junk != tok).any()
    rest = ClipTextRestatement(sd)
    for prune in (True, False):
        assert np.array_equal(rest.encode(junk, prune), rest.encode(tok, prune))


def test_plan_matches_torch_argmax():
    tok = synth.synth_clip_tokens([2, 77, 9, 30, 12])
    tok[2, 20] = 49407                  # the maximum twice: the first position counts
    tok[3, :] = 7                       # a constant row: position 0
    assert tok[1, 76] == 49407          # EOT in the last position
    eot, row0, total = _lib.clip_text_plan(tok)
    want = torch.as_tensor(tok).argmax(-1).numpy()
    assert list(want) == [1, 76, 8, 0, 11]
    assert np.array_equal(eot, want)
    assert np.array_equal(row0, np.concatenate([[0], np.cumsum(want + 1)[:-1]])) and total == int((want + 1).sum())
    for bad in (49408, -1):
        t = tok.copy()
        t[4, 40] = bad                  # behind EOT: still found
        with pytest.raises(_lib.EngineError, match="outside"):
            _lib.clip_text_plan(t)
    assert _lib.clip_text_plan(tok[:, :40], vocab_size=49408)[2] == 2 + 1 + 9 + 1 + 12         # another context length: row 1 loses its EOT, its maximum is the start mark at 0


def _expected_keys(layers=12, W=512, E=512, V=49408, ctx=77):
    keys = {"token_embedding.weight": (V, W), "positional_embedding": (ctx, W), "ln_final.weight": (W,), "ln_final.bias": (W,),
            "text_projection": (W, E)}
    for i in range(layers):
        p = f"transformer.resblocks.{i}."
        keys.update({p + "ln_1.weight": (W,), p + "ln_1.bias": (W,), p + "attn.in_proj_weight": (3 * W, W), p + "attn.in_proj_bias": (3 * W,),
                     p + "attn.out_proj.weight": (W, W), p + "attn.out_proj.bias": (W,), p + "ln_2.weight": (W,), p + "ln_2.bias": (W,),
                     p + "mlp.c_fc.weight": (4 * W, W), p + "mlp.c_fc.bias": (4 * W,), p + "mlp.c_proj.weight": (W, 4 * W),
                     p + "mlp.c_proj.bias": (W,)})
    return keys


def test_key_layout_and_loader():
    model = clip_text.CLIPTextEncoder()
    assert {k: tuple(v.shape) for k, v in model.state_dict().items()} == _expected_keys()
    assert {k: v.shape for k, v in state(12).items()} == _expected_keys()
    assert not any(p.requires_grad for p in model.parameters())
    # a whole CLIP state dict in fp16, as the archive ships it
    small = clip_text.CLIPTextEncoder(transformer_layers=2)
    sd = {k: torch.as_tensor(v).half() for k, v in state(2).items()}
    whole = dict(sd, **{"visual.conv1.weight": torch.zeros(4, 3, 2, 2).half(), "visual.proj": torch.zeros(4, 4).half(),
                        "logit_scale": torch.tensor(4.6), "input_resolution": torch.tensor(224), "context_length": torch.tensor(77),
                        "vocab_size": torch.tensor(49408)})
    clip_text.load_clip_text(small, whole)
    got = small.state_dict()
    assert all(v.dtype == torch.float32 for v in got.values())
    assert all(torch.equal(got[k], sd[k].float()) for k in sd)
    missing = dict(whole)
    del missing["transformer.resblocks.1.mlp.c_proj.bias"]
    with pytest.raises(KeyError, match="c_proj.bias"):
        clip_text.load_clip_text(small, missing)
    with pytest.raises(KeyError, match="stray.weight"):
        clip_text.load_clip_text(small, dict(whole, **{"stray.weight": torch.zeros(1)}))


def test_get_clip_reads_sizes_off_the_state_dict(tmp_path):
    from livelyspeaker_amd import motionclip
    sd = {k: torch.as_tensor(v) for k, v in state(2).items()}
    sd["visual.proj"] = torch.zeros(2, 2)
    path = tmp_path / "clip_sd.pt"
    torch.save(sd, path)
    for src in (sd, str(path)):
        m = motionclip.get_clip(src, device="cpu")
        assert isinstance(m, clip_text.CLIPTextEncoder) and m.transformer_layers == 2 and not m.training
        assert torch.equal(m.state_dict()["text_projection"], sd["text_projection"])
    assert "get_clip" in motionclip.get_SAG.__doc__


def test_abi_additions(tmp_path):
    hdr = open(os.path.join(ROOT, "include", "ls_hip.h")).read()
    lib = ctypes.CDLL(_lib.library_path())
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in _lib.EXPORTS and hasattr(lib, name), name
    lib.ls_abi_version.restype = ctypes.c_int
    assert lib.ls_abi_version() == 5
    fields = [n for n, _ in _lib.LsClipTextConfig._fields_]
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ls_hip.h"\nint main(void) {\n'
                   '    printf("%zu", sizeof(ls_clip_text_config));\n' +
                   "".join(f'    printf(" %zu", offsetof(ls_clip_text_config, {n}));\n' for n in fields) +
                   '    printf(" %d\\n", LS_ABI_VERSION);\n    return 0;\n}\n')
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    A = _lib.LsClipTextConfig
    assert got == [ctypes.sizeof(A)] + [getattr(A, n).offset for n in fields] + [5]


@pytest.mark.parametrize("field,value", [("width", 256), ("heads", 4), ("context_length", 78), ("layers", 25), ("embed_dim", 768)])
def test_create_rejects_unsupported_shapes_without_a_gpu(field, value):
    """The configuration checks come before the device is touched: LS_EUNSUPPORTED (-5) on a machine without a GPU."""
    kw = dict(vocab_size=49408, context_length=77, width=512, heads=8, layers=12, embed_dim=512)
    kw[field] = value
    with pytest.raises(_lib.EngineError, match=r"\(-5\)"):
        _lib.ClipTextEngine(**kw)
