"""One push of the post-processing stream (postprocess.open_post_stream) against the two ways the timeline entries can serve a live
stream, alternated in one process:

    python tools/post_stream_time.py               # S = 1, 8, 32; TED and BEAT (J = 47)      (profiles/r27_post_stream.md)

Per slot count S, k = 30 new frames per slot and push (one long-form window), device-resident input, 100 timed pushes after 5 warm-up
rounds.  Each round times, in this order,
  push     one PostStream.push of the chunk [S, J, F, 30]: every output plus the beats that became decidable
  chunk    the timeline entry on the same 30-frame chunk alone: the cost of the same frames before this stream existed, and wrong at
           every seam (no frame to the left, the beat range and the clamps end with the chunk)
  growing  the timeline entry on the whole series so far, 34 + 30 w frames in round w: the only correct alternative, until 4096 frames
TED: ted_postprocess_timeline; BEAT: beat_postprocess_timeline + beat_metrics_timeline(want=('beat_mask',)).  Times are a host clock
around calls that end in their own device wait; mean, median and worst in microseconds.  Also: ls_post_stream_info's device_bytes at
S = 32 before and after 1000 pushes.  The shader clock is sampled alongside (long_form_time.ClockSampler)."""
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from livelyspeaker_amd import beat_metrics as bm, postprocess as pp          # noqa: E402
from long_form_time import DEV, ClockSampler                                 # noqa: E402

WARM, ROUNDS, K = 5, 100, 30


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e6


def series(rng, S, J, F, N):
    x = np.cumsum(rng.standard_normal((S, J, F, N)).astype(np.float32) * 0.02, axis=3)
    if F == 6:
        x[:, :, 0] += 1.0
        x[:, :, 4] += 1.0
    return torch.from_numpy(x).to(DEV)


def line(name, us):
    return f"{name} {statistics.mean(us):8.1f} / {statistics.median(us):8.1f} / {max(us):8.1f}"


def main():
    clocks = ClockSampler()
    clocks.start()
    rng = np.random.default_rng(27)
    print(f"# one push of k = {K} frames per slot, device input; {ROUNDS} rounds after {WARM} warm-up rounds, push / chunk / growing alternated; "
          f"microseconds, mean / median / worst")
    for ds, J, F in (("ted", 9, 3), ("beat", 47, 6)):
        for S in (1, 8, 32):
            N = 34 + K * (WARM + ROUNDS)
            x = series(rng, S, J, F, N)
            if ds == "ted":
                whole = lambda t: pp.ted_postprocess_timeline(t)                                                        # noqa: E731
            else:
                whole = lambda t: bm.beat_metrics_timeline(pp.beat_postprocess_timeline(t)["pred_euler"], want=("beat_mask",))      # noqa: E731
            ps = pp.open_post_stream(ds, S)
            ps.push(x[..., :34].contiguous())
            t_push, t_chunk, t_grow, first_bytes = [], [], [], ps.device_bytes()
            for w in range(WARM + ROUNDS):
                lo = 34 + K * w
                chunk, so_far = x[..., lo:lo + K].contiguous(), x[..., :lo + K].contiguous()
                torch.cuda.synchronize()
                a = timed(lambda: ps.push(chunk))
                b = timed(lambda: whole(chunk))
                c = timed(lambda: whole(so_far))
                if w >= WARM:
                    t_push.append(a), t_chunk.append(b), t_grow.append(c)
            half = ROUNDS // 2
            print(f"{ds:4s} S={S:2d}: {line('push', t_push)}   {line('chunk', t_chunk)}   {line('growing', t_grow)}   | push, first half of the "
                  f"stream {statistics.median(t_push[:half]):.1f}, second half {statistics.median(t_push[half:]):.1f}; growing {statistics.median(t_grow[:half]):.1f} "
                  f"-> {statistics.median(t_grow[half:]):.1f} | {clocks.take()}", flush=True)
            if S == 32:
                for _ in range(1000):
                    ps.push(chunk)
                print(f"{ds:4s} S=32: device_bytes {first_bytes} after the first push, {ps.device_bytes()} after {int(ps.frames_in[0])} frames per slot "
                      f"({WARM + ROUNDS + 1001} pushes)", flush=True)
            ps.close()
    clocks.on = False


if __name__ == "__main__":
    main()
