"""Recorder of tests/golden/layer_overlap_parent.npz: what the fused step kernel's split-fp32 channel mixing (k_step PREC 2) computed BEFORE
a layer's movable vector work -- the SiLU epilogues of its passes, the bf16 split of chunk 1 -- was placed beside its bf16 MFMAs instead
of after them and after the mid-layer barriers.  Run once on the GPU with that earlier build of the library:

    python tests/golden/make_layer_overlap_golden.py --lib /path/to/the/earlier/libls_hip.so [OUT.npz]

(the layer trace goes into OUT_trace.npz beside it).

Only API that the earlier build has is used.  tests/test_gpu_layer_overlap.py imports `cases()` from here and demands bitwise equality:
the placement changes WHEN an epilogue or a split is computed, never its terms or their order.

The shapes are the smallest at which a moved epilogue, split or layer head can go wrong (fused path, precision 'fp32', Philox seed SEED):
  layers = 1   no next layer: work done early for it would add temb twice or leave stale partial sums, and the layer's last pass has
               no MFMAs after it to carry an epilogue
  layers = 2   one layer boundary
  layers = 3   a middle layer that both receives early work and issues it
each for
  ted_b1_cfg      TED,  B = 1, scale 1.5   rows 35 + 35: 6 ragged rows, tile 4's lanes partly masked in the split and in the epilogues
  ted_b3_single   TED,  B = 3, scale 1.0   single pass: a paired workgroup plus the odd tail
  beat_b2_cfg     BEAT, B = 2, scale 1.5   R = 72, 8 ragged rows
and for each of those one forward at t = 500 (cond and uncond outputs) and a 3-step DDPM loop; one forward also with the layer trace."""
import dataclasses
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SEED = 20261021
STEPS = 3                # the DDPM loops
FWD_STEPS = 50           # schedule of the engines that run the single forwards (as in make_weight_ring_golden.py)
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "layer_overlap_parent.npz")
OUT_TRACE = OUT[:-4] + "_trace.npz"          # the layer trace alone, in a file of its own: together they would pass 1 MiB
SHAPES = {"ted_b1_cfg": ("ted", 1, 1.5), "ted_b3_single": ("ted", 3, 1.0), "beat_b2_cfg": ("beat", 2, 1.5)}
LAYERS = (1, 2, 3)
TRACE = ("ted_b1_cfg", 3)          # the traced forward: every layer boundary of the deepest model, ragged rows


def _engine(ds, layers, batch, scale, steps=STEPS):
    from livelyspeaker_amd import _lib, synth
    cfg = dataclasses.replace(synth.CONFIGS[ds], layers=layers)
    eng = _lib.Engine(cfg.njoints, cfg.nfeats, cfg.n_prefix_tokens, cfg.audio_len, n_emotions=cfg.n_emotions, layers=layers, path="fused")
    eng.load_state_dict(synth.make_state_dict(cfg))
    eng.set_precision("fp32")
    eng.set_schedule(synth.schedule(steps))
    eng.prepare(synth.make_cond(cfg, batch, scale=scale))
    return cfg, eng


def loop(ds, layers, batch, scale, use_graph=True):
    """Final samples of the STEPS-step DDPM loop."""
    _, eng = _engine(ds, layers, batch, scale)
    try:
        out = np.array(eng.sample(sampler=0, philox_seed=SEED, use_graph=use_graph))
        assert eng.timing()["step_path"] == 0, "the fused kernel did not run"
        return out
    finally:
        eng.close()


def forward(ds, layers, batch, scale, t=500, trace=False):
    """(cond, uncond) outputs of one forward; with trace, also X before every layer and after the last: [B][layers + 1][R][512]."""
    cfg, eng = _engine(ds, layers, batch, scale, FWD_STEPS)
    try:
        g = np.random.Generator(np.random.PCG64(SEED + t))
        x = g.standard_normal((batch, cfg.njoints, cfg.nfeats, cfg.nframes)).astype(np.float32)
        eps = g.standard_normal((2, batch, 512)).astype(np.float32)
        res = eng.forward(x, np.full((batch,), t), eps[0], eps[1], trace=trace)
        return (np.array(res[0]), np.array(res[1])) + ((np.array(res[3]),) if trace else ())
    finally:
        eng.close()


def cases():
    """name -> callable returning the arrays of that case (a tuple for the forwards)."""
    out = {}
    for layers in LAYERS:
        for shape, (ds, batch, scale) in SHAPES.items():
            out[f"L{layers}_{shape}_fwd"] = lambda ds=ds, layers=layers, batch=batch, scale=scale: forward(ds, layers, batch, scale)
            out[f"L{layers}_{shape}_loop"] = lambda ds=ds, layers=layers, batch=batch, scale=scale: loop(ds, layers, batch, scale)
    shape, layers = TRACE
    ds, batch, scale = SHAPES[shape]
    out[f"L{layers}_{shape}_trace"] = lambda: forward(ds, layers, batch, scale, trace=True)
    return out


def keys(name):
    if name.endswith("_trace"):
        return [f"{name}.cond", f"{name}.uncond", f"{name}.trace"]
    if name.endswith("_fwd"):
        return [f"{name}.cond", f"{name}.uncond"]
    return [name]


def flatten(name, val):
    return dict(zip(keys(name), val if isinstance(val, tuple) else (val,)))


def main():
    argv = sys.argv[1:]
    if argv[:1] == ["--lib"]:                    # an earlier build of the library, bound before the first engine exists
        from livelyspeaker_amd import _lib
        _lib.use_library(argv[1])
        argv = argv[2:]
    out = argv[0] if argv else OUT
    rec = {}
    for name, fn in cases().items():
        for k, v in flatten(name, fn()).items():
            assert np.isfinite(v).all(), k
            rec[k] = v
            print(k, v.shape, float(np.abs(v).sum()))
    out_trace = out[:-4] + "_trace.npz"
    np.savez_compressed(out, **{k: v for k, v in rec.items() if not k.endswith(".trace")})
    np.savez_compressed(out_trace, **{k: v for k, v in rec.items() if k.endswith(".trace")})
    for f in (out, out_trace):
        print("wrote", f, os.path.getsize(f), "bytes")


if __name__ == "__main__":
    main()
