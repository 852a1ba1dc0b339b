"""Recorder of tests/golden/weight_ring_parent.npz: what the fused step kernel's split-fp32 channel mixing (k_step PREC 2) computed BEFORE
its weight fragments went through a register ring that runs across the pass boundaries of a layer.  Run once on the GPU with that
earlier build of the library:

    python tests/golden/make_weight_ring_golden.py --lib /path/to/the/earlier/libls_hip.so [OUT.npz]

Only API that the earlier build has is used.  tests/test_gpu_weight_ring.py imports `cases()` from here and demands bitwise equality: the
ring changes when a weight fragment is fetched, never which one multiplies what, so every accumulator sees the same sequence of additions.

The shapes are the smallest at which a ring can fetch the wrong thing (fused path, precision 'fp32', Philox seed SEED):
  layers = 1   there is no other layer: a ring that ran past its slice would leave the image, on every launch
  layers = 2   the synthetic state dict draws every layer's weights afresh: a ring that crossed into the wrong layer's, wave's or channel
               half's slice multiplies different numbers
each for
  ted_b1_cfg      TED,  B = 1, scale 1.5   one workgroup, rows 35 + 35, 6 ragged rows
  ted_b3_cfg      TED,  B = 3, scale 1.5   several workgroups
  ted_b3_single   TED,  B = 3, scale 1.0   single pass: a paired workgroup plus an odd tail
  beat_b2_cfg     BEAT, B = 2, scale 1.5   R = 72, 8 ragged rows
and for each of those one forward at t = 500 (cond and uncond outputs) and a 3-step DDPM loop."""
import dataclasses
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SEED = 20261020
STEPS = 3                # the DDPM loops
FWD_STEPS = 50           # schedule of the engines that run the single forwards (as in make_split_shared_golden.py)
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "weight_ring_parent.npz")
SHAPES = {"ted_b1_cfg": ("ted", 1, 1.5), "ted_b3_cfg": ("ted", 3, 1.5), "ted_b3_single": ("ted", 3, 1.0), "beat_b2_cfg": ("beat", 2, 1.5)}
LAYERS = (1, 2)


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


def forward(ds, layers, batch, scale, t=500):
    """(cond, uncond) outputs of one forward."""
    cfg, eng = _engine(ds, layers, batch, scale, FWD_STEPS)
    try:
        g = np.random.Generator(np.random.PCG64(SEED + t))
        x = g.standard_normal((batch, cfg.njoints, cfg.nfeats, cfg.nframes)).astype(np.float32)
        eps = g.standard_normal((2, batch, 512)).astype(np.float32)
        oc, ou, _ = eng.forward(x, np.full((batch,), t), eps[0], eps[1])
        return np.array(oc), np.array(ou)
    finally:
        eng.close()


def cases():
    """name -> callable returning the arrays of that case (a tuple for the forwards)."""
    out = {}
    for layers in LAYERS:
        for shape, (ds, batch, scale) in SHAPES.items():
            out[f"L{layers}_{shape}_fwd"] = lambda ds=ds, layers=layers, batch=batch, scale=scale: forward(ds, layers, batch, scale)
            out[f"L{layers}_{shape}_loop"] = lambda ds=ds, layers=layers, batch=batch, scale=scale: loop(ds, layers, batch, scale)
    return out


def flatten(name, val):
    if isinstance(val, tuple):
        return {f"{name}.cond": val[0], f"{name}.uncond": val[1]}
    return {name: val}


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
    np.savez_compressed(out, **rec)
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
