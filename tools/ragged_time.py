"""Time of one ragged call of the onset chain and of each timeline entry, next to the two things a caller had before it:

    python tools/ragged_time.py                  # the figures of profiles/r16_ragged.md
    python tools/ragged_time.py --rounds 15

  (a) loop     one equal-length call per clip at the clip's own length: the correct alternative
  (b) padded   one equal-length call on the batch padded to the longest clip: WRONG numbers at every clip's end, cost only

The batch: B = 32 speeches whose lengths spread 8x (12.5 s .. 100 s of 16 kHz audio; 184 .. 1504 gesture frames), device-resident,
warm.  A call time is a host clock around work that ends in a device synchronise (every entry point waits for its kernels).  The three
variants of an entry are ALTERNATED round by round in one process, so that clock and thermal drift hits all three alike; the figure is
the median over the rounds, with the spread (min .. max) next to it."""
import sys
import time

import numpy as np

sys.path.insert(0, ".")
from livelyspeaker_amd import audio_onsets as ao, beat_metrics as bm, postprocess as pp  # noqa: E402

B, J, SR = 32, 47, 16000


def main():
    import torch
    rounds = int(sys.argv[sys.argv.index("--rounds") + 1]) if "--rounds" in sys.argv else 25
    g = np.random.default_rng(0)
    seconds = np.linspace(12.5, 100.0, B)
    g.shuffle(seconds)
    lengths = (seconds * SR).astype(np.int64)
    frames = (34 + 30 * np.maximum(0, -(-(lengths - 36267) // 32000))).astype(np.int64)       # long_form.plan_windows
    L, N = int(lengths.max()), int(frames.max())
    print(f"B = {B}; audio {lengths.min()} .. {L} samples (sum {lengths.sum()}, padded {B * L}); frames {frames.min()} .. {N} "
          f"(sum {frames.sum()}, padded {B * N}); {rounds} alternated rounds, median (min .. max) in ms")

    audio = torch.from_numpy((0.05 * g.standard_normal((B, L))).astype(np.float32)).cuda()
    audio[:, ::6400] += 0.9
    ted = torch.from_numpy(np.cumsum(0.05 * g.standard_normal((B, 9, 3, N)), axis=3).astype(np.float32)).cuda()
    beat = torch.from_numpy((np.array([1, 0, 0, 0, 1, 0], np.float32)[None, None, :, None]
                             + np.cumsum(0.08 * g.standard_normal((B, J, 6, N)), axis=3)).astype(np.float32)).cuda()
    euler = pp.beat_postprocess_timeline(beat)["pred_euler"]
    target = euler + 1.2 * torch.randn_like(euler)
    onsets = [np.sort(g.uniform(0, f / 15.0, size=max(3, int(2.4 * f / 15)))).astype(np.float32) for f in frames]
    # the per-clip inputs of the loop, made contiguous ahead of the clock (a caller with ragged speeches holds them this way)
    audio_b = [audio[b:b + 1, :n].contiguous() for b, n in enumerate(lengths)]
    ted_b = [ted[b:b + 1, ..., :n].contiguous() for b, n in enumerate(frames)]
    beat_b = [beat[b:b + 1, ..., :n].contiguous() for b, n in enumerate(frames)]
    euler_b = [euler[b:b + 1, :n].contiguous() for b, n in enumerate(frames)]
    target_b = [target[b:b + 1, :n].contiguous() for b, n in enumerate(frames)]
    want_on = ("count", "onset_raw", "onset_bt_rms")

    entries = {
        "audio_onsets": (
            lambda: ao.audio_onsets(audio, SR, want=want_on, lengths=lengths),
            lambda: [ao.audio_onsets(a, SR, want=want_on) for a in audio_b],
            lambda: ao.audio_onsets(audio, SR, want=want_on)),
        "ted_postprocess_timeline": (
            lambda: pp.ted_postprocess_timeline(ted, frames=frames),
            lambda: [pp.ted_postprocess_timeline(t) for t in ted_b],
            lambda: pp.ted_postprocess_timeline(ted)),
        "beat_postprocess_timeline": (
            lambda: pp.beat_postprocess_timeline(beat, frames=frames),
            lambda: [pp.beat_postprocess_timeline(t) for t in beat_b],
            lambda: pp.beat_postprocess_timeline(beat)),
        "beat_metrics_timeline": (
            lambda: bm.beat_metrics_timeline(euler, target, None, onsets, frames=frames),
            lambda: [bm.beat_metrics_timeline(e, t, None, [o]) for e, t, o in zip(euler_b, target_b, onsets)],
            lambda: bm.beat_metrics_timeline(euler, target, None, onsets)),
    }
    for name, fns in entries.items():
        ms = [[], [], []]
        for r in range(rounds + 3):                       # three warm rounds, not recorded
            for i, fn in enumerate(fns):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                if r >= 3:
                    ms[i].append((time.perf_counter() - t0) * 1e3)
        med = [float(np.median(m)) for m in ms]
        for label, m, md in zip(("ragged", "(a) loop", "(b) padded"), ms, med):
            print(f"{name:27s} {label:10s} {md:8.3f} ({min(m):.3f} .. {max(m):.3f})")
        print(f"{name:27s} loop / ragged = {med[1] / med[0]:.2f}, padded / ragged = {med[2] / med[0]:.2f}")


if __name__ == "__main__":
    main()
