"""The audio front end measured (livelyspeaker_amd.audio_io); the figures of profiles/r30_resample.md:

    python tools/resample_time.py [--out FILE] [quality] [oneshot] [push]

1. Filter quality, from the library's own taps (CPU, the float64 restatement of tests/resample_restatement.py): per input rate the
   amplitude of a 1 s unit tone after resampling to 16 kHz -- 100 Hz, 4 kHz, 7 kHz (passband) and 8.4, 9, 12 kHz (leak: what aliases
   into the output); read off the middle half of the output as sqrt(2) * rms.  A tone at or above the input's Nyquist is left out.
2. One-shot time: 1, 8 and 64 clips of 60 s float32 mono at 48 and 44.1 kHz, device-resident, host clock around ``resample`` (which ends
   in its own device wait), median (min .. max) of RUNS runs after a warm-up; beside it ``scipy.signal.resample_poly`` with the same taps
   on the host for ONE clip (it scales with the clips), and the host-to-device copy of the same input from pageable memory -- the floor
   a caller who resamples on the host pays as well (for the 16 kHz result: a third of it).
3. Push time: ``open_stream(input_sr=48000, input_channels=2)`` fed int16 stereo chunks of 96000 frames against the same stream fed the
   32000 float32 samples at 16 kHz, one engine each, alternated push by push: every push completes exactly one window (TED, ddim100
   skip 80, philox, device inputs; the setting of profiles/r22_long_stream.md).  The difference is what the front end costs per window."""
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, ".")
sys.path.insert(0, "tests")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from livelyspeaker_amd import audio_io  # noqa: E402

RUNS, WARM, WINDOWS = 7, 3, 25
LINES = []


def say(line=""):
    print(line, flush=True)
    LINES.append(line)


def fmt(v):
    return f"{statistics.median(v):.3f} ({min(v):.3f} .. {max(v):.3f})"


def quality():
    import resample_restatement as rr
    say("## 1. Filter quality (zeros 32, beta 12, rolloff 0.95; amplitude of a unit tone after resampling to 16 kHz)")
    say()
    tones = (100, 4000, 7000, 8400, 9000, 12000)
    say("| input | taps | DC gain − 1 | " + " | ".join(f"{f} Hz" for f in tones) + " |")
    say("|---|---|---|" + "---|" * len(tones))
    for sr in (48000, 44100, 22050, 8000):
        h64, _, r = audio_io.resample_taps(sr)
        t = np.arange(sr) / sr
        cells = []
        for f in tones:
            if 2 * f >= sr:
                cells.append("—")
                continue
            y, _ = rr.resample(np.sin(2 * np.pi * f * t), r["up"], r["down"], r["half"], h64)
            mid = y[len(y) // 4: 3 * len(y) // 4]
            amp = float(np.sqrt(2 * np.mean(mid * mid)))
            cells.append(f"1 − {1 - amp:.1e}" if 0.9999 < amp < 1 else f"{amp:.3g}")
        say(f"| {sr} | {r['n_taps']} | {h64.sum() / r['up'] - 1:.1e} | " + " | ".join(cells) + " |")
    say()


def oneshot():
    import torch
    import scipy.signal as ss
    say(f"## 2. One-shot: clips of 60 s float32 mono -> 16 kHz (ms; median (min .. max) of {RUNS} runs)")
    say()
    say("| input | clips | `resample` on the device | H2D copy of the input | scipy `resample_poly`, ONE clip, host |")
    say("|---|---|---|---|---|")
    for sr in (48000, 44100):
        h64, _, r = audio_io.resample_taps(sr)
        one = np.random.default_rng(sr).uniform(-1, 1, size=60 * sr).astype(np.float32)
        host_ms = []
        for _ in range(3):
            t0 = time.perf_counter()
            ref = ss.resample_poly(one.astype(np.float64), r["up"], r["down"], window=h64 / r["up"])
            host_ms.append((time.perf_counter() - t0) * 1e3)
        for B in (1, 8, 64):
            x = np.ascontiguousarray(np.broadcast_to(one, (B, one.size)))
            copy_ms = []
            for _ in range(RUNS):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                xd = torch.from_numpy(x).cuda()
                torch.cuda.synchronize()
                copy_ms.append((time.perf_counter() - t0) * 1e3)
            y, n = audio_io.resample(xd, sr)                                 # warm-up
            err = float(np.abs(y[0, :n[0]].cpu().numpy() - ref).max())
            dev_ms = []
            for _ in range(RUNS):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                audio_io.resample(xd, sr)
                dev_ms.append((time.perf_counter() - t0) * 1e3)
            say(f"| {sr} | {B} | {fmt(dev_ms)} | {fmt(copy_ms)} | {fmt(host_ms)} (max abs difference to the device's output {err:.1e}) |")
            del xd, y
    say()


def push():
    import torch
    from livelyspeaker_amd import long_form, synth
    from long_form_time import DEV, build
    say(f"## 3. Push that completes one window: stream fed 48 kHz int16 stereo against the stream fed 16 kHz float32 (ms; {WINDOWS} windows after "
        f"{WARM}, alternated; TED ddim100 skip 80, philox, device inputs)")
    say()
    say("| B | push at 16 kHz, median / worst | push at 48 kHz, median / worst | difference of medians |")
    say("|---|---|---|---|")
    cfg, model_a, diffusion = build()
    _, model_b, _ = build()
    diffusion.noise_source, diffusion.philox_seed = "philox", 1
    AL, STRIDE = cfg.audio_len, 32000
    for B in (1, 8, 32):
        n_win = WARM + WINDOWS
        y = {k: torch.from_numpy(v).to(DEV) for k, v in synth.make_long_cond(cfg, B, n_win).items()}
        rng = np.random.default_rng(B)
        mic = torch.from_numpy((3000 * rng.standard_normal((B, 3 * (AL + (n_win - 1) * STRIDE) + 1200, 2))).astype(np.int16)).to(DEV)
        audio, _ = audio_io.resample(mic, 48000)
        args = (y["seed_poses"], y["vid_indices"], y["scale"])
        a = long_form.open_stream(diffusion, model_a, *args, sampler="ddim", skip_timesteps=80)
        b = long_form.open_stream(diffusion, model_b, *args, sampler="ddim", skip_timesteps=80, input_sr=48000, input_channels=2,
                                  resample={"max_chunk": 3 * STRIDE})
        fa = [a.push(audio[:, :AL])]
        # the resampler decides an output only once the samples behind it are in: feed 48 kHz frames until window 0 is complete
        pos = 3 * AL + 3 * 200
        fb = [b.push(mic[:, :3 * STRIDE]), b.push(mic[:, 3 * STRIDE:pos])]
        assert fa[0].shape[3] == 34 and sum(f.shape[3] for f in fb) == 34
        ms_a, ms_b = [], []
        for w in range(1, n_win):
            chunk = audio[:, AL + (w - 1) * STRIDE:AL + w * STRIDE]
            t0 = time.perf_counter()
            fa.append(a.push(chunk))
            t1 = time.perf_counter()
            fb.append(b.push(mic[:, pos:pos + 3 * STRIDE]))
            t2 = time.perf_counter()
            pos += 3 * STRIDE
            assert fa[-1].shape[3] == 30 and fb[-1].shape[3] == 30
            if w >= WARM:
                ms_a.append((t1 - t0) * 1e3)
                ms_b.append((t2 - t1) * 1e3)
        same = bool(torch.equal(torch.cat(fa, dim=3), torch.cat(fb, dim=3)))
        say(f"| {B} | {statistics.median(ms_a):.2f} / {max(ms_a):.2f} | {statistics.median(ms_b):.2f} / {max(ms_b):.2f} | "
            f"{statistics.median(ms_b) - statistics.median(ms_a):+.2f} (frames equal: {same}) |")
    say()


def main():
    argv = sys.argv[1:]
    out = None
    if "--out" in argv:
        out = argv[argv.index("--out") + 1]
        del argv[argv.index("--out"):argv.index("--out") + 2]
    parts = argv or ["quality", "oneshot", "push"]
    say("# The audio front end: filter quality, one-shot time, push time (tools/resample_time.py)")
    say()
    for name in parts:
        {"quality": quality, "oneshot": oneshot, "push": push}[name]()
    if out:
        with open(out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
