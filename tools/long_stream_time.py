"""Streaming long-form synthesis (long_form.open_stream) against the one-window call of the interface that existed before it
(long_form.sample_long(n_windows=1)), alternated in one process:

    python tools/long_stream_time.py               # B = 1, 8, 32 at ddim100 skip 80 and at the full ddim100 (profiles/r22_long_stream.md)
    python tools/long_stream_time.py 8             # one batch size

TED, Philox noise, guidance 1.5, device-resident inputs, hipGraph replay.  Two models with the same weights, one engine each: the stream
lives on one, the yardstick on the other (a sample_long on the stream's engine would replace its conditioning and end the stream).

Per-window latency: the wall time (host clock around a call that ends in the engine's own wait) of a push of 32000 samples that completes
exactly one window, i.e. from the arrival of a window's last sample to its 30 frames; 3 warm-up windows, then WINDOWS windows, each
followed by one yardstick call on a waveform of audio_len samples; median and worst of both, and the ratio of the medians.  The REAL-TIME
MARGIN is that latency against the 2.0 s of audio a window consumes (32000 samples at 16 kHz).

Whole stream: SECONDS of speech fed in CHUNK-second pushes plus the close, end to end, against one sample_long of the same waveform on the
other engine; median of REPS alternated repetitions.  The shader clock is sampled alongside (long_form_time.ClockSampler)."""
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, ".")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from livelyspeaker_amd import long_form, synth                                        # noqa: E402
from long_form_time import DEV, ClockSampler, build                                   # noqa: E402

WARM, WINDOWS, SECONDS, CHUNK, REPS, STRIDE = 3, 25, 60.0, 0.37, 3, 32000


def timed(fn):
    """ms of a call that waits for its own device work (push / sample_long both end in the engine's synchronise)."""
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def main():
    batches = [int(sys.argv[1])] if len(sys.argv) > 1 else [1, 8, 32]
    cfg, model_s, diffusion = build()
    _, model_y, _ = build()
    diffusion.noise_source, diffusion.philox_seed = "philox", 1
    AL = cfg.audio_len
    clocks = ClockSampler()
    clocks.start()
    print(f"# TED ddim100, CFG 1.5, philox, device inputs, graph replay; per-window latency over {WINDOWS} windows after {WARM} warm-up windows, "
          f"stream push (32000 samples completing one window) alternated with sample_long(n_windows=1); ms, median / worst")
    for skip in (80, 0):
        for B in batches:
            n_win = WARM + WINDOWS                                  # windows 0 .. WARM - 1 warm up, the rest are timed
            y = {k: torch.from_numpy(v).to(DEV) for k, v in synth.make_long_cond(cfg, B, n_win).items()}
            audio = y["audio"]
            first = audio[:, :AL].contiguous()

            def yard():
                return long_form.sample_long(diffusion, model_y, first, y["seed_poses"], y["vid_indices"], y["scale"], n_windows=1,
                                             sampler="ddim", skip_timesteps=skip)

            st = long_form.open_stream(diffusion, model_s, y["seed_poses"], y["vid_indices"], y["scale"], sampler="ddim", skip_timesteps=skip)
            assert st.push(first).shape[3] == 34
            yard()
            torch.cuda.synchronize()
            clocks.take()
            push_ms, yard_ms = [], []
            for w in range(1, n_win):
                chunk = audio[:, AL + (w - 1) * STRIDE:AL + w * STRIDE]
                ms, new = timed(lambda: st.push(chunk))
                assert new.shape[3] == 30
                ms_y, _ = timed(yard)
                if w >= WARM:
                    push_ms.append(ms)
                    yard_ms.append(ms_y)
            t = model_s.model.engine().timing()
            assert len(push_ms) == WINDOWS >= 20
            med_p, med_y = statistics.median(push_ms), statistics.median(yard_ms)
            print(f"skip {skip:2d} ({100 - skip:3d} steps) B={B:3d}: push {med_p:8.2f} / {max(push_ms):8.2f} [min {min(push_ms):.2f}]   "
                  f"sample_long(1) {med_y:8.2f} / {max(yard_ms):8.2f} [min {min(yard_ms):.2f}]   ratio of medians {med_p / med_y:.3f}   "
                  f"real-time margin: worst push = {max(push_ms) / 2000.0:.4f} of the 2.0 s a window consumes   | window loop "
                  f"{t['total_ms']:.2f} ms on the device, graph replayed {t['graph_replayed']} of {t['n_segments']}, step path {t['step_path']} | "
                  f"{clocks.take()}", flush=True)
            st.close()
            # ---- the whole stream, end to end
            L = int(round(SECONDS * 16000))
            W = long_form.plan_windows(L, cfg)[0]
            yl = {k: torch.from_numpy(v).to(DEV) for k, v in synth.make_long_cond(cfg, B, W).items()}
            speech = yl["audio"][:, :L].contiguous()
            n = int(round(CHUNK * 16000))

            def whole_stream():
                s = long_form.open_stream(diffusion, model_s, yl["seed_poses"], yl["vid_indices"], yl["scale"], sampler="ddim", skip_timesteps=skip)
                parts = [s.push(speech[:, lo:lo + n]) for lo in range(0, L, n)]
                parts.append(s.close())
                return torch.cat(parts, dim=3)

            def whole_call():
                return long_form.sample_long(diffusion, model_y, speech, yl["seed_poses"], yl["vid_indices"], yl["scale"], sampler="ddim",
                                             skip_timesteps=skip)

            a, b = whole_stream(), whole_call()                     # warm-up of both; the same key: the same bits
            same = bool(torch.equal(a, b))
            ws, wc = [], []
            for _ in range(REPS):
                torch.cuda.synchronize()
                ws.append(timed(whole_stream)[0])
                torch.cuda.synchronize()
                wc.append(timed(whole_call)[0])
            print(f"            whole {SECONDS:g} s ({W} windows) B={B:3d}: stream in {CHUNK:g} s chunks ({-(-L // n)} pushes + close) "
                  f"{statistics.median(ws):9.2f} [{min(ws):.2f} .. {max(ws):.2f}]   one sample_long {statistics.median(wc):9.2f} "
                  f"[{min(wc):.2f} .. {max(wc):.2f}]   ratio {statistics.median(ws) / statistics.median(wc):.3f}   outputs equal: {same}   | "
                  f"{clocks.take()}", flush=True)
    clocks.on = False


if __name__ == "__main__":
    main()
