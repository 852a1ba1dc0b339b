#!/usr/bin/env python3
"""Times ``ingest.ted_ingest`` for 64 recordings of 60 s (25 fps poses, 16 kHz audio) against the numpy restatement of the reference's
pipeline (tests/ingest_restatement.py) on the same machine's CPU.  Reported, not gated (profiles/r18_ingest.md).

    python tools/ingest_time.py [recordings] [seconds] [repeats]

Device time: the recordings are resident CUDA tensors, as a loader that keeps raw clips on the device would hold them; one warm-up,
then the median and the spread of ``repeats`` calls, each closed by torch.cuda.synchronize() (the call itself waits for its kernels
and for the one boolean index).  The host-pointer figure includes the upload of the recordings and the download of every window.
The restatement runs once over the same recordings, one thread."""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ingest_restatement as R                                        # noqa: E402
from livelyspeaker_amd import ingest                                  # noqa: E402
from livelyspeaker_amd.postprocess import TED_DIR_VEC_PAIRS, TED_MEAN_DIR_VEC      # noqa: E402


def main():
    n_rec = int(sys.argv[1]) if len(sys.argv) > 1 else 64
    seconds = float(sys.argv[2]) if len(sys.argv) > 2 else 60.0
    repeats = int(sys.argv[3]) if len(sys.argv) > 3 else 7
    rng = np.random.Generator(np.random.PCG64(18))
    mean_pose = np.zeros((10, 3))
    for j, (a, b, ln) in enumerate(TED_DIR_VEC_PAIRS):
        mean_pose[b] = mean_pose[a] + ln * TED_MEAN_DIR_VEC[3 * j:3 * j + 3]
    n = int(seconds * 25)
    t = np.linspace(0, seconds, n)[:, None, None]
    sk, au = [], []
    for _ in range(n_rec):
        pose = np.repeat(mean_pose[None], n, 0)
        pose[:, 4:] += 0.1 * np.sin(2 * np.pi * rng.uniform(0.4, 1.0, (1, 6, 3)) * t + rng.uniform(0, 6.28, (1, 6, 3)))
        sk.append(pose.astype(np.float32))
        au.append((0.1 * rng.standard_normal(int(seconds * 16000))).astype(np.float32))
    s, e = [0.0] * n_rec, [seconds] * n_rec
    args = (s, e, mean_pose.astype(np.float32), TED_MEAN_DIR_VEC)

    def timed(fn, reps):
        out = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = fn()
            torch.cuda.synchronize()
            out.append((time.perf_counter() - t0) * 1e3)
        return out, r

    d_sk, d_au = [torch.from_numpy(v).cuda() for v in sk], [torch.from_numpy(v).cuda() for v in au]
    timed(lambda: ingest.ted_ingest(d_sk, d_au, *args), 1)
    dev, got = timed(lambda: ingest.ted_ingest(d_sk, d_au, *args), repeats)
    host, _ = timed(lambda: ingest.ted_ingest(sk, au, *args), 3)
    t0 = time.perf_counter()
    n_ref = sum(len(R.ted_ingest(sk[b], au[b], s[b], e[b], mean_pose, TED_MEAN_DIR_VEC)) for b in range(n_rec))
    cpu_ms = (time.perf_counter() - t0) * 1e3
    W = int(got["keep"].numel())
    assert n_ref == W
    print(json.dumps({"recordings": n_rec, "seconds": seconds, "windows": W, "kept": int(got["keep"].sum()),
                      "device_resident_ms_median": float(np.median(dev)), "device_resident_ms_min": min(dev), "device_resident_ms_max": max(dev),
                      "host_pointers_ms_median": float(np.median(host)), "numpy_restatement_cpu_ms": cpu_ms,
                      "windows_per_s_device": W / (float(np.median(dev)) * 1e-3), "repeats": repeats}))


if __name__ == "__main__":
    main()
