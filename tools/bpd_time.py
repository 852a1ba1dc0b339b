"""Per-column time of the likelihood loop (ls_bpd, calc_bpd_loop) against the DDIM loop of the same handle over the same 100 schedule
indices, alternated in one process:

    python tools/bpd_time.py                  # the table of profiles/r10_bpd.md (TED B = 512 / 32 / 4; Philox, hipGraph replay)
    python tools/bpd_time.py trace            # a few bpd loops at every shape and nothing else: run it under
                                              # rocprofv3 --kernel-trace --stats -d <dir> -- python tools/bpd_time.py trace
                                              # and read k_vb_terms / k_q_sample / k_q_sample_philox from the kernel stats

A handle keeps ONE captured loop, so each block below is one capturing call followed by timed replays; DDIM and bpd blocks alternate and
the spread of the DDIM figure over its blocks is printed next to it (the step kernel is power-bound: its clock moves from run to run).
loop_ms is the handle's own event pair around the loop (ls_timing).  A column is q_sample (in Philox
mode the same launch draws the column's noise plane) + one model evaluation + k_vb_terms; the surplus over a DDIM step is what the two
extra launches cost."""
import sys

import numpy as np

sys.path.insert(0, ".")
from livelyspeaker_amd import _lib, synth  # noqa: E402

SHAPES = (("ted", 512), ("ted", 32), ("ted", 4))
ROUNDS, REPLAYS, T = 4, 6, 100


def engine(ds, B):
    cfg = synth.CONFIGS[ds]
    eng = _lib.Engine(cfg.njoints, cfg.nfeats, cfg.n_prefix_tokens, cfg.audio_len, n_emotions=cfg.n_emotions, path="auto")
    eng.load_state_dict(synth.make_state_dict(cfg))
    eng.set_schedule(synth.schedule(1000, "ddim100"))
    eng.prepare(synth.make_cond(cfg, B))
    return cfg, eng


def block(run, eng, replays):
    """One capture + `replays` timed replays: loop_ms of each replay."""
    run()
    out = []
    for _ in range(replays):
        run()
        t = eng.timing()
        assert t["graph_replayed"] == 1 and t["n_step_launches"] == T
        out.append(t["loop_ms"])
    return out


def runners(cfg, eng, B):
    import torch
    dev = torch.device("cuda", eng.device)
    x0 = torch.from_numpy(synth.make_init_image(cfg, B)).to(dev)
    outs = tuple(torch.empty(B, T, device=dev) for _ in range(3))
    g = torch.Generator(device=dev).manual_seed(1)
    nz = torch.randn((T, B, cfg.njoints, cfg.nfeats, cfg.nframes), device=dev, generator=g)
    eps = torch.randn((T, 2, B, 512), device=dev, generator=g)
    return (lambda: eng.sample(philox_seed=1, sampler=_lib.LS_SAMPLER_DDIM, device_out=True),
            lambda: eng.bpd(x0, outs, philox_seed=1),
            lambda: eng.bpd(x0, outs, noise_tape=nz, eps_tape=eps))


def table():
    print(f"# ddim100 tables, all {T} schedule indices, CFG 1.5, hipGraph replay; {ROUNDS} alternated blocks of {REPLAYS} replays; ms per step / column")
    print("| shape | DDIM step (median, min .. max over blocks) | bpd column, Philox | surplus, us | bpd column, device tapes | surplus, us |")
    print("|---|---|---|---|---|---|")
    for ds, B in SHAPES:
        cfg, eng = engine(ds, B)
        ddim, philox, tape = runners(cfg, eng, B)
        dd, bp, bt = [], [], []
        for _ in range(ROUNDS):
            dd.append(np.median(block(ddim, eng, REPLAYS)) / T)
            bp.append(np.median(block(philox, eng, REPLAYS)) / T)
            bt.append(np.median(block(tape, eng, REPLAYS)) / T)
        t = eng.timing()
        fmt = lambda v: f"{np.median(v):.4f} ({min(v):.4f} .. {max(v):.4f})"      # noqa: E731
        print(f"| {ds} B = {B} (family {t['step_path']}) | {fmt(dd)} | {fmt(bp)} | {(np.median(bp) - np.median(dd)) * 1e3:+.1f} | {fmt(bt)} | "
              f"{(np.median(bt) - np.median(dd)) * 1e3:+.1f} |", flush=True)
        eng.close()


def trace():
    for ds, B in SHAPES:
        cfg, eng = engine(ds, B)
        _, philox, tape = runners(cfg, eng, B)
        for _ in range(3):
            philox()
        tape()
        print(f"{ds} B = {B}: 3 Philox bpd loops, 1 tape loop", flush=True)
        eng.close()


if __name__ == "__main__":
    {"table": table, "trace": trace}[sys.argv[1] if len(sys.argv) > 1 else "table"]()
