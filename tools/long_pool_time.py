"""The session pool (long_form.open_pool) against one open_stream per speaker, alternated in one process:

    python tools/long_pool_time.py               # S = 4 and 8 speakers (profiles/r23_long_pool.md)
    python tools/long_pool_time.py 4             # one pool size

TED, Philox noise, guidance 1.5, device-resident inputs, hipGraph replay, ddim100 skip 80 (20 steps per window).  S speakers talk at the
same rate but started at different times: speaker s is s * 32000 / S samples ahead of speaker 0, so their windows complete at staggered
times.  Audio arrives in TICKS: every tick brings every speaker the same number of new samples,

  * 32000 per tick: every speaker completes one window in every tick (the pool runs one round at batch S);
  * 32000 / S per tick: exactly one speaker completes a window in every tick (the pool runs one round at batch 1).

The pool takes a tick as ONE push on one model; the baseline is what the interface offered before it: S models with the same weights,
one open_stream at batch 1 each, pushed in turn.  Per tick the two are timed back to back (host clock around calls that end in the
engine's own wait), pool first on even ticks and baseline first on odd ones; WARM ticks warm up, TICKS ticks are timed; median and
worst per tick, and per completed window.  The shader clock is sampled alongside (long_form_time.ClockSampler)."""
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


def main():
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
