"""The session pool (long_form.open_pool) against one open_stream per speaker, alternated in one process:

    python tools/long_pool_time.py               # S = 4 and 8 speakers (profiles/r23_long_pool.md)
    python tools/long_pool_time.py 4             # one pool size
    python tools/long_pool_time.py --keyed       # a keyed pool (noise_keys='clip') against an unkeyed one at 1, 4, 8 and 32 speakers
                                                 # (profiles/r28_pool_keys.md); sizes may follow
    python tools/long_pool_time.py --pins        # a pinned round against a plain round of the same pool at 1, 4 and 8 speakers
                                                 # (profiles/r33_pool_pins.md); sizes may follow

TED, Philox noise, guidance 1.5, device-resident inputs, hipGraph replay, ddim100 skip 80 (20 steps per window).  S speakers talk at the
same rate but started at different times: speaker s is s * 32000 / S samples ahead of speaker 0, so their windows complete at staggered
times.  Audio arrives in TICKS: every tick brings every speaker the same number of new samples,

  * 32000 per tick: every speaker completes one window in every tick (the pool runs one round at batch S);
  * 32000 / S per tick: exactly one speaker completes a window in every tick (the pool runs one round at batch 1).

The pool takes a tick as ONE push on one model; the baseline is what the interface offered before it: S models with the same weights,
one open_stream at batch 1 each, pushed in turn.  Per tick the two are timed back to back (host clock around calls that end in the
engine's own wait), pool first on even ticks and baseline first on odd ones; WARM ticks warm up, TICKS ticks are timed; median and
worst per tick, and per completed window.  The shader clock is sampled alongside (long_form_time.ClockSampler).

--keyed: two pools with the same weights on two models, one opened with noise_keys='clip', fed the same ticks and timed the same way,
keyed first on even ticks.  What the keys add to a round: the upload of its rows of the key table, one draw launch per ring refill
(csrc/ls_philox_rows.hip) and the step kernels reading their draws from the ring in place of computing them.

--pins: ONE pool opened with pins=64, every speaker fed 32000 samples per tick, so every tick is one round at batch S.  Ahead of every
other tick each speaker's coming window is pinned (one whole pose, ten frames ahead of the frames returned), which makes that tick's
round an inpainting call at batch S; the ticks between are plain calls at the same batch, in the same process, on the same handle.
Timed per tick: the push, and on pinned ticks the S pin calls ahead of it (each ends in a host wait).  Reported: median / worst of a
plain push and of a pinned push, their difference, the plain pushes' own spread (worst - best, and the median absolute deviation), and
the pin calls.  What a pinned round adds: k_pool_pin_gather, and per step the denoiser alone plus the inpainting update in place of
the fused step with its update."""
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, ".")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from livelyspeaker_amd import long_form, synth                                        # noqa: E402
from long_form_time import DEV, ClockSampler, build                                   # noqa: E402

WARM, TICKS, STRIDE, SKIP = 4, 24, 32000, 80


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def run(S, per_tick, cfg, pool_model, stream_models, diffusion, clocks):
    AL = cfg.audio_len
    n_ticks = WARM + TICKS
    lead = [s * STRIDE // S for s in range(S)]                       # samples speaker s is ahead by
    total = AL + max(lead) + n_ticks * per_tick
    y = {k: torch.from_numpy(v).to(DEV) for k, v in synth.make_long_cond(cfg, S, -(-total // STRIDE) + 1).items()}
    pool = long_form.open_pool(diffusion, pool_model, S, sampler="ddim", skip_timesteps=SKIP)
    streams = []
    for s in range(S):
        assert pool.join(y["seed_poses"][s], y["vid_indices"][s], y["scale"][s]) == s
        streams.append(long_form.open_stream(diffusion, stream_models[s], y["seed_poses"][s:s + 1], y["vid_indices"][s:s + 1], y["scale"][s:s + 1],
                                             sampler="ddim", skip_timesteps=SKIP))
    # before the clock starts: window 0 of every speaker, and each speaker's lead
    fed = [AL + lead[s] for s in range(S)]
    head = torch.zeros(S, max(fed), device=DEV)
    for s in range(S):
        head[s, :fed[s]] = y["audio"][s, :fed[s]]
    pool.push(head, fed)
    for s in range(S):
        streams[s].push(y["audio"][s:s + 1, :fed[s]])
    torch.cuda.synchronize()
    clocks.take()
    pool_ms, base_ms, windows = [], [], 0
    for t in range(n_ticks):
        chunk = torch.stack([y["audio"][s, fed[s]:fed[s] + per_tick] for s in range(S)]).contiguous()

        def tick_pool():
            return pool.push(chunk, [per_tick] * S)[1]

        def tick_base():
            return [int(streams[s].push(chunk[s:s + 1]).shape[3]) for s in range(S)]

        if t % 2 == 0:
            ms_p, counts = timed(tick_pool)
            ms_b, each = timed(tick_base)
        else:
            ms_b, each = timed(tick_base)
            ms_p, counts = timed(tick_pool)
        assert counts.tolist() == each, (counts, each)                # the same windows completed on both sides
        fed = [n + per_tick for n in fed]
        if t >= WARM:
            pool_ms.append(ms_p)
            base_ms.append(ms_b)
            windows += sum(1 for c in each if c)
    tm = pool_model.model.engine().timing()
    med_p, med_b = statistics.median(pool_ms), statistics.median(base_ms)
    print(f"S={S:2d}, {per_tick:5d} samples per tick ({windows / TICKS:.2f} windows per tick): pool push {med_p:8.2f} / {max(pool_ms):8.2f}   "
          f"{S} streams in turn {med_b:8.2f} / {max(base_ms):8.2f}   ratio of medians {med_p / med_b:.3f}   per completed window: pool "
          f"{sum(pool_ms) / windows:.2f}, streams {sum(base_ms) / windows:.2f} ms   | last pool push: "
          f"graph replayed {tm['graph_replayed']} of {tm['n_segments']}, step path {tm['step_path']} | {clocks.take()}", flush=True)
    pool.close()
    for st in streams:
        st.close()


def run_keyed(S, per_tick, cfg, models, diffusion, clocks):
    AL = cfg.audio_len
    n_ticks = WARM + TICKS
    lead = [s * STRIDE // S for s in range(S)]
    total = AL + max(lead) + n_ticks * per_tick
    y = {k: torch.from_numpy(v).to(DEV) for k, v in synth.make_long_cond(cfg, S, -(-total // STRIDE) + 1).items()}
    pools = [long_form.open_pool(diffusion, m, S, sampler="ddim", skip_timesteps=SKIP, noise_keys=nk) for m, nk in zip(models, ("clip", None))]
    fed = [AL + lead[s] for s in range(S)]
    head = torch.zeros(S, max(fed), device=DEV)
    for s in range(S):
        head[s, :fed[s]] = y["audio"][s, :fed[s]]
    for pool in pools:
        for s in range(S):
            assert pool.join(y["seed_poses"][s], y["vid_indices"][s], y["scale"][s]) == s
        pool.push(head, fed)
    torch.cuda.synchronize()
    clocks.take()
    ms, windows = ([], []), 0
    for t in range(n_ticks):
        chunk = torch.stack([y["audio"][s, fed[s]:fed[s] + per_tick] for s in range(S)]).contiguous()
        order = (0, 1) if t % 2 == 0 else (1, 0)
        got = {}
        for i in order:
            got[i] = timed(lambda: pools[i].push(chunk, [per_tick] * S)[1])
        assert got[0][1].tolist() == got[1][1].tolist()
        fed = [n + per_tick for n in fed]
        if t >= WARM:
            for i in (0, 1):
                ms[i].append(got[i][0])
            windows += sum(1 for c in got[0][1] if c)
    tm = models[0].model.engine().timing()
    med_k, med_u = statistics.median(ms[0]), statistics.median(ms[1])
    print(f"S={S:2d}, {per_tick:5d} samples per tick ({windows / TICKS:.2f} windows per tick): keyed push {med_k:8.2f} / {max(ms[0]):8.2f}   "
          f"unkeyed push {med_u:8.2f} / {max(ms[1]):8.2f}   ratio of medians {med_k / med_u:.3f}   per completed window: keyed "
          f"{sum(ms[0]) / windows:.3f}, unkeyed {sum(ms[1]) / windows:.3f} ms   | last keyed push: graph replayed {tm['graph_replayed']} of "
          f"{tm['n_segments']}, step path {tm['step_path']} | {clocks.take()}", flush=True)
    for pool in pools:
        pool.close()


def run_pins(S, cfg, model, diffusion, clocks):
    AL, per_tick, n_ticks = cfg.audio_len, STRIDE, WARM + 2 * TICKS
    total = AL + n_ticks * per_tick
    y = {k: torch.from_numpy(v).to(DEV) for k, v in synth.make_long_cond(cfg, S, -(-total // STRIDE) + 1).items()}
    pool = long_form.open_pool(diffusion, model, S, sampler="ddim", skip_timesteps=SKIP, pins=64)
    for s in range(S):
        assert pool.join(y["seed_poses"][s], y["vid_indices"][s], y["scale"][s]) == s
    pose = (torch.rand(cfg.njoints, cfg.nfeats, 1, generator=torch.Generator().manual_seed(33)) * 2 - 1).to(DEV)
    pool.push(y["audio"][:, :AL].contiguous(), [AL] * S)            # before the clock starts: window 0 of every speaker
    torch.cuda.synchronize()
    clocks.take()
    fed, ms, pin_ms = AL, {False: [], True: []}, []
    for t in range(n_ticks):
        chunk = y["audio"][:, fed:fed + per_tick].contiguous()
        pinned = t % 2 == 1
        if pinned:
            at = int(pool.slots["frames_out"][0]) + 10              # owned by the window this tick completes
            ms_pin, _ = timed(lambda: [pool.pin(s, [at], pose) for s in range(S)])
        ms_push, counts = timed(lambda: pool.push(chunk, [per_tick] * S)[1])
        assert counts.tolist() == [30] * S and pool.slots["pins"].tolist() == [0] * S
        fed += per_tick
        if t >= WARM:
            ms[pinned].append(ms_push)
            if pinned:
                pin_ms.append(ms_pin)
    tm = model.model.engine().timing()
    plain, pins = ms[False], ms[True]
    med_p, med_i = statistics.median(plain), statistics.median(pins)
    mad = statistics.median(abs(v - med_p) for v in plain)
    print(f"S={S:2d}, one round at batch {S} per tick, {len(plain)} plain and {len(pins)} pinned ticks: plain push {med_p:7.3f} / {max(plain):7.3f}   "
          f"pinned push {med_i:7.3f} / {max(pins):7.3f}   pinned - plain {med_i - med_p:+.3f} ms ({med_i / med_p:.3f}x)   plain spread: worst - best "
          f"{max(plain) - min(plain):.3f}, median abs deviation {mad:.3f}   {S} pin calls {statistics.median(pin_ms):.3f} / {max(pin_ms):.3f}   | last push: "
          f"graph replayed {tm['graph_replayed']} of {tm['n_segments']}, step path {tm['step_path']} | {clocks.take()}", flush=True)
    pool.close()


def main_pins(sizes):
    cfg, model, diffusion = build()
    diffusion.noise_source, diffusion.philox_seed = "philox", 1
    clocks = ClockSampler()
    clocks.start()
    print(f"# TED ddim100 skip {SKIP}, CFG 1.5, philox, device inputs, graph replay; one pool with pins=64, {WARM} warm-up ticks, then plain and "
          f"pinned ticks in turn ({TICKS} each); ms per push, median / worst")
    for S in sizes or [1, 4, 8]:
        run_pins(S, cfg, model, diffusion, clocks)
    clocks.on = False


def main_keyed(sizes):
    cfg, model_k, diffusion = build()
    model_u = build()[1]
    diffusion.noise_source, diffusion.philox_seed = "philox", 1
    clocks = ClockSampler()
    clocks.start()
    print(f"# TED ddim100 skip {SKIP}, CFG 1.5, philox, device inputs, graph replay; {TICKS} ticks after {WARM} warm-up ticks, a push of a keyed "
          f"pool alternated with the same push of an unkeyed one; ms per tick, median / worst")
    for S in sizes or [1, 4, 8, 32]:
        for per_tick in sorted({STRIDE, STRIDE // S}, reverse=True):
            run_keyed(S, per_tick, cfg, (model_k, model_u), diffusion, clocks)
    clocks.on = False


def main():
    if "--keyed" in sys.argv[1:]:
        return main_keyed([int(a) for a in sys.argv[1:] if a != "--keyed"])
    if "--pins" in sys.argv[1:]:
        return main_pins([int(a) for a in sys.argv[1:] if a != "--pins"])
    sizes = [int(sys.argv[1])] if len(sys.argv) > 1 else [4, 8]
    cfg, pool_model, diffusion = build()
    stream_models = [build()[1] for _ in range(max(sizes))]
    diffusion.noise_source, diffusion.philox_seed = "philox", 1
    clocks = ClockSampler()
    clocks.start()
    print(f"# TED ddim100 skip {SKIP}, CFG 1.5, philox, device inputs, graph replay; {TICKS} ticks after {WARM} warm-up ticks, one pool push "
          f"alternated with S open_stream pushes at batch 1; ms per tick, median / worst")
    for S in sizes:
        for per_tick in (STRIDE, STRIDE // S):
            run(S, per_tick, cfg, pool_model, stream_models, diffusion, clocks)
    clocks.on = False


if __name__ == "__main__":
    main()
