#!/usr/bin/env python3
"""GPU time of the CLIP text encoder for 512 sentences, three legs alternated call by call in one process so that they see the
same clocks: the packed form (prune), the full form (all 77 rows) and torch-ROCm's own forward of the tests' torch module
(tests/clip_text_restatement.py: nn.MultiheadAttention / nn.LayerNorm / nn.Linear, fp32, all 77 rows).

Length distribution (fixed): 512 lengths drawn uniformly from 6 .. 24 tokens, both marks included, by numpy's PCG64 seeded with 13 --
a sentence spoken inside a 2.3 s clip is about a dozen tokens.  Tokens are host tensors (what clip.tokenize returns), features stay
on the device; the engine's time is its HIP-event span (token upload included), torch's is a torch.cuda.Event span.

    python tools/clip_text_time.py [layers]          # default 12
Prints one line per leg, the R / (77 B) ratio of the run and the parity of the packed leg against the float64 restatement on eight
of the sentences in units of torch's own fp32 CPU error."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
from clip_text_restatement import ClipTextRestatement, TorchClipText
from livelyspeaker_amd import _lib, clip_text, synth

layers = int(sys.argv[1]) if len(sys.argv) > 1 else 12
B = 512
lengths = [int(n) for n in np.random.Generator(np.random.PCG64(13)).integers(6, 25, B)]
tok = torch.as_tensor(synth.synth_clip_tokens(lengths))
sd = synth.synth_clip_text_state(layers=layers)
model = clip_text.CLIPTextEncoder(transformer_layers=layers)
clip_text.load_clip_text(model, {k: torch.as_tensor(v) for k, v in sd.items()})
model = model.cuda().eval()
ref32 = TorchClipText(sd, torch.float32)
eng = model.engine()
_, _, R = _lib.clip_text_plan(tok)
print(f"layers {layers}  B {B}  packed rows R {R}  R / (77 B) = {R / (77 * B):.4f}")

pick = list(range(0, B, B // 8))
f64 = ClipTextRestatement(sd).encode(tok[pick].numpy(), prune=False)
e32 = float(np.abs(ref32(tok[pick]).double().numpy() - f64).max())
err = float(np.abs(model.encode_text(tok)[pick].double().cpu().numpy() - f64).max())
print(f"parity on sentences {pick}: e32 {e32:.3e}  HIP {err:.3e}  ratio {err / e32:.2f}")

ref32 = ref32.cuda()
tok_dev = tok.cuda()
# the shader clock needs a few hundred ms of load to reach its ceiling: heat it first, then time calls back to back
heat = torch.randn(4096, 4096, device="cuda")
for _ in range(60):
    heat = torch.mm(heat, heat) * 1e-3
torch.cuda.synchronize()
tp, tf, tt = [], [], []
for _ in range(30):
    model.encode_text(tok, prune=True)
    tp.append(eng.last_encode_ms())
    model.encode_text(tok, prune=False)
    tf.append(eng.last_encode_ms())
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    ref32(tok_dev)
    b.record()
    b.synchronize()
    tt.append(a.elapsed_time(b))
for name, t in (("packed (prune)", tp), ("full (77 rows)", tf), ("torch-ROCm fp32 module", tt)):
    print(f"{name}: median of last 20 = {np.median(t[10:]):.3f} ms  min {min(t):.3f} ms")
print(f"full / packed = {np.median(tf[10:]) / np.median(tp[10:]):.2f}   torch / packed = {np.median(tt[10:]) / np.median(tp[10:]):.2f}")
