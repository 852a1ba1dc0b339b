#!/usr/bin/env python3
"""GPU time of ls_sag_decode and ls_sag_enc_encode at B = 512 (HIP events on the handles' streams), steady state, the two alternated
call by call in one process so that they see the same clocks: python tools/sag_time.py [library.so] [ted|beat]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from livelyspeaker_amd import _lib, synth

args = sys.argv[1:]
cfg = synth.CONFIGS[args.pop()] if args and args[-1] in ("ted", "beat") else synth.TED
if args:
    _lib.use_library(args[0])
name = os.path.basename(args[0]) if args else "in-tree"
eng = _lib.SagEngine(cfg.njoints, cfg.nfeats)
eng.load_state_dict(synth.make_sag_state_dict(cfg))
enc = _lib.SagEncoderEngine(cfg.njoints, cfg.nfeats)
enc.load_state_dict(synth.make_sag_encoder_state_dict(cfg))
B = 512
xb = torch.from_numpy(synth.make_cond(cfg, B)["origin_x"]).cuda()
zb = torch.from_numpy(synth.make_text_features(B)).cuda()
mask = torch.ones(B, 34, dtype=torch.bool, device="cuda")
# The shader clock idles at ~100 MHz and needs a few hundred ms of load to reach its 2.4 GHz ceiling (rocm-smi while bench.py runs);
# 30 one-millisecond calls with a host sync each never get there.  Heat it with a GEMM loop first, then time calls back to back.
heat = torch.randn(4096, 4096, device="cuda")
for _ in range(60):
    heat = torch.mm(heat, heat) * 1e-3
torch.cuda.synchronize()
td, te = [], []
for _ in range(40):
    eng.decode(xb, zb)
    td.append(eng.last_decode_ms())
    enc.encode(xb, mask)
    te.append(enc.last_encode_ms())
dec_ms = float(np.median(td[20:]))
print(name, cfg.name, "sag decode ms: median of last 20 =", round(dec_ms, 4), "min", round(min(td), 4))
enc_ms = float(np.median(te[20:]))
print(name, cfg.name, "sag encode ms: median of last 20 =", round(enc_ms, 4), "min", round(min(te), 4), "| encode / decode =", round(enc_ms / dec_ms, 3))
