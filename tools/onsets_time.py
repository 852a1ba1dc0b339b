"""Time of the audio-onset chain (ls_onsets, audio_onsets.audio_onsets) at the shape of one TED evaluation batch:

    python tools/onsets_time.py               # B = 512 clips of 36267 samples, device-resident, warm; the figures of profiles/r14_onsets.md

Each kernel is timed alone by the event pair ls_onsets records around it (ls_onsets_args.kernel_ms); the call is timed by a host clock
around work that ends in a device synchronise, so it includes the table upload, the temporaries and the one host wait for the counts.
The spectrum kernel reads every sample four times (hop 512 of a 2048-sample frame), which the caches serve; its algorithmic HBM traffic
is the audio once plus the dB planes it writes."""
import sys
import time

import numpy as np

sys.path.insert(0, ".")
from livelyspeaker_amd import audio_onsets as ao  # noqa: E402

B, L, RUNS = 512, 36267, 20
HBM_BYTES_PER_S = 8.0e12        # MI355X peak HBM3E rate


def main():
    import torch
    g = np.random.default_rng(0)
    audio = torch.from_numpy((0.1 * g.standard_normal((B, L))).astype(np.float32)).cuda()
    F = 1 + L // ao.HOP
    want = ("oenv", "count", "onset_raw", "onset_bt", "onset_bt_rms")
    for _ in range(3):
        ao.audio_onsets(audio, 16000, want=want)
    spec, pick, call = [], [], []
    for _ in range(RUNS):
        ms = []
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = ao.audio_onsets(audio, 16000, want=want, timing=ms)
        torch.cuda.synchronize()
        call.append((time.perf_counter() - t0) * 1e3)
        spec.append(ms[0])
        pick.append(ms[1])
    in_bytes, db_bytes = B * L * 4, B * F * 128 * 4
    fmt = lambda v: f"{np.median(v):.3f} ({min(v):.3f} .. {max(v):.3f})"      # noqa: E731
    print(f"B = {B}, L = {L} ({F} frames per clip), {RUNS} warm runs, median (min .. max) in ms; onsets per clip {got['counts'].mean():.1f}")
    print(f"k_onset_spectrum  {fmt(spec)}")
    print(f"k_onset_pick      {fmt(pick)}")
    print(f"whole call        {fmt(call)}")
    t = np.median(spec) * 1e-3
    print(f"audio {in_bytes / 1e6:.1f} MB read once + {db_bytes / 1e6:.1f} MB of dB planes written: {(in_bytes + db_bytes) / t / 1e9:.0f} GB/s = "
          f"{(in_bytes + db_bytes) / t / HBM_BYTES_PER_S:.3f} of the HBM rate; the audio alone {in_bytes / t / 1e9:.0f} GB/s = "
          f"{in_bytes / t / HBM_BYTES_PER_S:.3f}")
    flops = B * F * (5 * 1024 * 10 + 1025 * 12 + 2 * 2045)        # radix-4 FFT ~ 5 N log2 N, post-pass and power, mel gathers
    print(f"arithmetic: about {flops / 1e9:.2f} GFLOP, {flops / t / 1e12:.2f} TFLOP/s")


if __name__ == "__main__":
    main()
