#!/usr/bin/env python3
"""In-kernel phase profile of ls::k_step (debug aid).  Uses a -DLS_DEBUG build of the library (variants/debug.so; build it in
the container with `python tools/phase_profile.py build`, it travels to the GPU box): there LS_PROF=<workgroup> makes lane 0
of each wave of that workgroup record s_memtime at phase boundaries.  The shipped library has no such code.
Prints mean cycles per phase (over waves and layers)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("LS_PROF", "300")
from livelyspeaker_amd import _lib, synth          # noqa: E402
from livelyspeaker_amd import build as _build      # noqa: E402

DEBUG_LIB = os.path.join(_build.ROOT, "variants", "debug.so")
if len(sys.argv) > 1 and sys.argv[1] == "build":
    os.makedirs(os.path.dirname(DEBUG_LIB), exist_ok=True)
    print(_build.build_library(defines=["LS_DEBUG"], out=DEBUG_LIB))
    sys.exit(0)
_lib.use_library(DEBUG_LIB)

ds = sys.argv[1] if len(sys.argv) > 1 else "ted"
B = int(sys.argv[2]) if len(sys.argv) > 2 else 512
cfg = synth.CONFIGS[ds]
PATH = os.environ.get("LS_PROF_PATH", "fused")          # "fused" (k_step, 8 waves) or "pass" (k_pass, 4 waves)
NWV = 4 if PATH == "pass" else 8
eng = _lib.Engine(cfg.njoints, cfg.nfeats, cfg.n_prefix_tokens, cfg.audio_len, n_emotions=cfg.n_emotions, path=PATH)
eng.load_state_dict(synth.make_state_dict(cfg))
if os.environ.get("LS_PROF_PRECISION"):
    eng.set_precision(os.environ["LS_PROF_PRECISION"])
eng.set_schedule(synth.schedule(8))
eng.prepare(synth.make_cond(cfg, B))
for _ in range(2):
    eng.sample(sampler=0, philox_seed=1)
raw = np.empty(8 * 96 * 2, np.float32)
n = eng.lib.ls_read(eng.h, b"prof", raw.ctypes.data_as(_lib.c_f32p), raw.size)
st = raw.view(np.uint64).reshape(8, 96).astype(np.float64)[:NWV]
L = 8
names = ["LN1 stats(+temb)", "LN1 store+bar", "token-mix", "LN2 stats", "LN2 store+bar", "GEMM pass0+epi", "GEMM pass1+epi", "(trace)"]
print(f"{ds} B={B} path={PATH}: total cycles (wave mean) = {np.mean(st[:, 4 + 8 * L] - st[:, 0]):.0f}")
print(f"  embed                : {np.mean(st[:, 1] - st[:, 0]):9.0f}")
prev = st[:, 1].copy()
# the split-fp32 form that stages LN2 per 48-row chunk stamps point 8 too: 6 -> 7 = tiles 0-2 (both channel halves), 7 -> 8 = barrier +
# store of chunk 1 + barrier, 8 -> 9 = tiles 3-4; every other form stamps 7 after its first channel half and never 8
chunked = bool(st[:, 8].any())
if chunked:
    names = names[:5] + ["chunk 0 (tiles 0-2)", "bar+store 1+bar", "chunk 1 (tiles 3-4)"]
pts = [2, 3, 4, 5, 6, 7, 8, 9] if chunked else [2, 3, 4, 5, 6, 7, 9]
acc = np.zeros(len(pts))
for l in range(L):
    for i, pnt in enumerate(pts):
        cur = st[:, pnt + 8 * l]
        acc[i] += np.mean(cur - prev)
        prev = cur
for i in range(len(pts)):
    print(f"  {names[i]:21s}: {acc[i] / L:9.0f} /layer")
print(f"  X->U + barrier       : {np.mean(st[:, 2 + 8 * L] - prev):9.0f}")
print(f"  out-proj MFMA        : {np.mean(st[:, 3 + 8 * L] - st[:, 2 + 8 * L]):9.0f}")
print(f"  OUT + combine        : {np.mean(st[:, 4 + 8 * L] - st[:, 3 + 8 * L]):9.0f}")
print("  per-wave totals:", (st[:, 4 + 8 * L] - st[:, 0]).astype(int).tolist())
if chunked and NWV == 8:
    # Per wave, not per mean: how long the fastest and the slowest wave take for each phase, separately for waves 0-3 and 4-7 (wave w and
    # w + 4 share a SIMD), and how long a wave then stands at the barrier that follows the stamp.  A wave's wait is the time from its own
    # stamp to the last wave's: exact where the barrier follows the stamp directly (7), a lower bound where work lies between (1: temb
    # add and LN1 partial sums, 4: LN2 partial sums, 5: the store of chunk 0).
    halves = [("waves 0-3", slice(0, 4)), ("waves 4-7", slice(4, 8))]
    dur = np.zeros((len(pts), NWV))
    prev = st[:, 1].copy()
    for l in range(L):
        for i, pnt in enumerate(pts):
            cur = st[:, pnt + 8 * l]
            dur[i] += (cur - prev) / L
            prev = cur
    print("  per phase and layer: mean | earliest wave .. latest wave (its number), by SIMD half")
    for i in range(len(pts)):
        row = f"  {names[i]:21s}:"
        for hname, hs in halves:
            d = dur[i, hs]
            row += f"   {hname} {d.mean():8.0f} | {d.min():8.0f} (w{hs.start + int(d.argmin())}) .. {d.max():8.0f} (w{hs.start + int(d.argmax())})"
        print(row)
    bars = [(1, "layer end -> LN1 barrier"), (4, "token-mix end -> LN2 barrier"), (5, "LN2 stats -> chunk-0 barrier"), (7, "chunk 0 end -> mid barrier")]
    print("  arrival at the barriers, per layer: spread = latest - earliest wave; wait = latest wave's stamp - own stamp")
    for pnt, bname in bars:
        arr = np.stack([st[:, pnt + 8 * l] for l in range(1 if pnt == 1 else 0, L)])          # [layers][waves]; the first layer's 1 follows the embedding
        wait = arr.max(axis=1, keepdims=True) - arr
        spread = (arr.max(axis=1) - arr.min(axis=1)).mean()
        pair = np.abs(arr[:, :4] - arr[:, 4:]).mean()                                         # |stamp(w) - stamp(w + 4)|: skew between SIMD partners
        lead = (arr[:, 4:] - arr[:, :4]).mean()                                               # > 0: the younger half arrives later
        print(f"  {bname:29s}: spread {spread:7.0f}   mean wait " + "  ".join(f"{hname} {wait[:, hs].mean():7.0f}" for hname, hs in halves)
              + f"   partner skew {pair:7.0f} (w+4 later by {lead:+.0f})   last to arrive: " + ",".join(f"w{int(x)}" for x in arr.argmax(axis=1)))
if os.environ.get("LS_PROF_RAW"):
    l = 3
    base = st[:, 1 + 8 * l].min()
    print("per-wave stamps of layer 3 (cycles since earliest previous-layer end):")
    for wv in range(NWV):
        print(f"  wave {wv}:", [int(st[wv, p + 8 * l] - base) for p in [1] + pts])
