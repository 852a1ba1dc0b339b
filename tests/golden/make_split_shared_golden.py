"""Recorder of tests/golden/split_shared_parent.npz: what the fused step kernel's split-fp32 channel mixing (k_step PREC 2) computed
BEFORE its LayerNorm-2 operand was split once per 48-row chunk in LDS.  Run once on the GPU with that earlier build of the library:

    python tests/golden/make_split_shared_golden.py [OUT.npz]

Only API that the earlier build has is used.  tests/test_gpu_split_shared.py imports `cases()` from here and demands bitwise equality:
the parts, the terms and their order are the same, so every accumulator sees the same sequence of additions.

Cases (fused path, precision 'fp32', synth.schedule(50), Philox seed SEED):
  a  TED,  B = 3, scale 1.5  CFG rows 35 + 35: the 47 / 48 chunk seam falls inside the uncond pass, 6 ragged rows
  b  TED,  B = 3, scale 1.0  single-pass (two samples per workgroup) with an odd batch
  c  BEAT, B = 2, scale 1.5  R = 72, 8 ragged rows
  d  TED and BEAT, B = 3     one forward each at t = 500, cond and uncond outputs"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SEED = 20261019
STEPS = 50
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "split_shared_parent.npz")


def _engine(ds, batch, scale):
    from livelyspeaker_amd import _lib, synth
    cfg = synth.CONFIGS[ds]
    eng = _lib.Engine(cfg.njoints, cfg.nfeats, cfg.n_prefix_tokens, cfg.audio_len, n_emotions=cfg.n_emotions, path="fused")
    eng.load_state_dict(synth.make_state_dict(cfg))
    eng.set_precision("fp32")
    eng.set_schedule(synth.schedule(STEPS))
    eng.prepare(synth.make_cond(cfg, batch, scale=scale))
    return cfg, eng


def loop(ds, batch, scale, use_graph=True):
    """Final samples of the STEPS-step DDPM loop."""
    _, eng = _engine(ds, batch, scale)
    try:
        out = np.array(eng.sample(sampler=0, philox_seed=SEED, use_graph=use_graph))
        assert eng.timing()["step_path"] == 0, "the fused kernel did not run"
        return out
    finally:
        eng.close()


def forward(ds, batch=3, t=500):
    """(cond, uncond) outputs of one forward."""
    cfg, eng = _engine(ds, batch, 1.5)
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
    return {
        "a_ted_b3_cfg": lambda: loop("ted", 3, 1.5),
        "b_ted_b3_single": lambda: loop("ted", 3, 1.0),
        "c_beat_b2_cfg": lambda: loop("beat", 2, 1.5),
        "d_ted_fwd": lambda: forward("ted"),
        "d_beat_fwd": lambda: forward("beat"),
    }


def flatten(name, val):
    if isinstance(val, tuple):
        return {f"{name}.cond": val[0], f"{name}.uncond": val[1]}
    return {name: val}


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else OUT
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
