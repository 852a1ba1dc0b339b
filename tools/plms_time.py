"""Per-evaluation loop time of the PLMS sampler (order 4) against the DDIM loop of the same handle, alternated in one process:

    python tools/plms_time.py                 # the table of profiles/r08_plms.md (TED B = 4 / 32 / 512, BEAT B = 256; Philox, hipGraph replay)
    python tools/plms_time.py call            # the LivelySpeaker-shaped comparison: 512 clips, ddim100, skip_timesteps = 80
    python tools/plms_time.py trace           # a few PLMS loops at every shape and nothing else: run it under
                                              # rocprofv3 --kernel-trace --stats -d <dir> -- python tools/plms_time.py trace
                                              # and read k_plms_update's durations from the kernel stats

A handle keeps ONE captured loop, so each block below is one capturing call followed by timed replays; DDIM and PLMS blocks alternate and
the spread of the DDIM figure over its blocks is printed next to it (the step kernel is power-bound: its clock moves from run to run).
loop_ms is the handle's own event pair around the loop (ls_timing)."""
import sys

import numpy as np

sys.path.insert(0, ".")
from livelyspeaker_amd import _lib, synth  # noqa: E402

SHAPES = (("ted", 4), ("ted", 32), ("ted", 512), ("beat", 256))
SKIP, ROUNDS, REPLAYS = 60, 4, 6            # 40 executed steps per loop


def engine(ds, B):
    cfg = synth.CONFIGS[ds]
    eng = _lib.Engine(cfg.njoints, cfg.nfeats, cfg.n_prefix_tokens, cfg.audio_len, n_emotions=cfg.n_emotions, path="auto")
    eng.load_state_dict(synth.make_state_dict(cfg))
    eng.set_schedule(synth.schedule(1000, "ddim100"))
    eng.prepare(synth.make_cond(cfg, B))
    return cfg, eng


def block(eng, replays, **kw):
    """One capture + `replays` timed replays: loop_ms of each replay."""
    eng.sample(philox_seed=1, **kw)
    out = []
    for _ in range(replays):
        eng.sample(philox_seed=1, **kw)
        t = eng.timing()
        assert t["graph_replayed"] == 1
        out.append(t["loop_ms"])
    return out


def table():
    n_exec = 100 - SKIP
    print(f"# ddim100 tables, skip_timesteps = {SKIP} ({n_exec} executed steps), CFG 1.5, Philox, hipGraph replay; {ROUNDS} alternated blocks of {REPLAYS} replays")
    print("| shape | DDIM ms / evaluation (median, min .. max over blocks) | PLMS-4 ms / evaluation (median, min .. max) | difference, us |")
    print("|---|---|---|---|")
    for ds, B in SHAPES:
        cfg, eng = engine(ds, B)
        dd, pl = [], []
        for _ in range(ROUNDS):
            dd.append(np.median(block(eng, REPLAYS, sampler=_lib.LS_SAMPLER_DDIM, skip_timesteps=SKIP)) / n_exec)
            pl.append(np.median(block(eng, REPLAYS, sampler=_lib.LS_SAMPLER_PLMS, plms_order=4, skip_timesteps=SKIP)) / (n_exec + 1))
        t = eng.timing()
        print(f"| {ds} B = {B} (family {t['step_path']}) | {np.median(dd):.4f} ({min(dd):.4f} .. {max(dd):.4f}) | {np.median(pl):.4f} ({min(pl):.4f} .. {max(pl):.4f}) | "
              f"{(np.median(pl) - np.median(dd)) * 1e3:+.1f} |", flush=True)
        eng.close()


def call():
    cfg, eng = engine("ted", 512)
    init = synth.make_init_image(cfg, 512)
    x_T = eng.philox_x_init(512, seed=7)
    ref = None
    print("# 512 clips, ddim100, init_image, given x_T, Philox style draws; loop_ms per call (median of 6 replays), max-abs distance to 20-step DDIM")
    print("| sampler | executed steps | model evaluations | ms per call | max-abs distance to 20-step DDIM |")
    print("|---|---|---|---|---|")
    for name, kw, n_exec in (("DDIM", dict(sampler=_lib.LS_SAMPLER_DDIM), 20), ("PLMS order 4", dict(sampler=_lib.LS_SAMPLER_PLMS, plms_order=4), 20),
                             ("PLMS order 4", dict(sampler=_lib.LS_SAMPLER_PLMS, plms_order=4), 12), ("PLMS order 4", dict(sampler=_lib.LS_SAMPLER_PLMS, plms_order=4), 8)):
        kw = dict(kw, skip_timesteps=100 - n_exec, init_image=init, x_init=x_T)
        ms = np.median(block(eng, 6, **kw))
        out = eng.sample(philox_seed=1, **kw)
        if ref is None:
            ref = out
        print(f"| {name} | {n_exec} | {eng.timing()['n_step_launches']} | {ms:.2f} | {float(np.abs(out - ref).max()):.3f} |", flush=True)
    eng.close()


def trace():
    for ds, B in SHAPES:
        _, eng = engine(ds, B)
        for _ in range(3):
            eng.sample(philox_seed=1, sampler=_lib.LS_SAMPLER_PLMS, plms_order=4, skip_timesteps=SKIP)
        print(f"{ds} B = {B}: 3 PLMS loops", flush=True)
        eng.close()


if __name__ == "__main__":
    {"table": table, "call": call, "trace": trace}[sys.argv[1] if len(sys.argv) > 1 else "table"]()
