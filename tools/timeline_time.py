"""Time of the timeline post-processing and scores at one minute of gesture (N = 934 frames = 31 chained windows):

    python tools/timeline_time.py                 # TED B = 512, BEAT B = 32, device-resident, warm; the figures of profiles/r15_timeline_post.md
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/timeline_time.py --runs 5      # the kernel times, in a run of its own

Call times are a host clock around work that ends in a device synchronise (every entry point waits for its kernels).  Next to each
timeline call runs what a user had before it: the 34-frame entry point called once per window of the chain (31 slices of 34 frames every 30
frames, each made contiguous first), which yields the windows' numbers, not the timeline's (beats and velocities reset at every seam).
The bytes are the algorithmic traffic computed from the shapes: every input read once, every output written once."""
import sys
import time

import numpy as np

sys.path.insert(0, ".")
from livelyspeaker_amd import beat_metrics as bm, postprocess as pp  # noqa: E402

N, W = 934, 31
B_TED, B_BEAT, J = 512, 32, 47


def timed(fn, runs):
    import torch
    for _ in range(3):
        fn()
    ms = []
    for _ in range(runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return f"{np.median(ms):8.3f} ({min(ms):.3f} .. {max(ms):.3f})"


def main():
    import torch
    runs = int(sys.argv[sys.argv.index("--runs") + 1]) if "--runs" in sys.argv else 20
    g = np.random.default_rng(0)
    ted = torch.from_numpy(np.cumsum(0.05 * g.standard_normal((B_TED, 9, 3, N)), axis=3).astype(np.float32)).cuda()
    beat = torch.from_numpy((np.array([1, 0, 0, 0, 1, 0], np.float32)[None, None, :, None]
                             + np.cumsum(0.08 * g.standard_normal((B_BEAT, J, 6, N)), axis=3)).astype(np.float32)).cuda()
    n_on = 150                                                      # about 2.4 onsets per second of speech
    slab = torch.from_numpy(np.sort(g.integers(0, 1946, size=(B_TED, n_on)), axis=1).astype(np.int32)).cuda()
    count = torch.full((B_TED,), n_on, dtype=torch.int32).cuda()
    onsets = [np.sort(g.uniform(0, N / 15.0, size=n_on)).astype(np.float32) for _ in range(B_BEAT)]
    win_onsets = [np.sort(g.uniform(0, 34 / 15.0, size=5)).astype(np.float32) for _ in range(B_BEAT)]
    mask = pp.ted_postprocess_timeline(ted)["beat_mask"]
    euler = pp.beat_postprocess_timeline(beat)["pred_euler"]
    target = euler + 1.2 * torch.randn_like(euler)

    def ted_slices():
        for w in range(W):
            pp.ted_postprocess(ted[..., 30 * w:30 * w + 34].contiguous())

    def beat_post_slices():
        for w in range(W):
            pp.beat_postprocess(beat[..., 30 * w:30 * w + 34].contiguous())

    def beat_metrics_slices():
        for w in range(W):
            bm.beat_metrics(euler[:, 30 * w:30 * w + 34].contiguous(), target[:, 30 * w:30 * w + 34].contiguous(), None, win_onsets)

    print(f"N = {N} frames ({W} windows), {runs} warm runs, median (min .. max) in ms")
    print(f"TED  B = {B_TED}: ted_postprocess_timeline          {timed(lambda: pp.ted_postprocess_timeline(ted), runs)}")
    print(f"TED  B = {B_TED}: ted_postprocess per window x {W}    {timed(ted_slices, runs)}")
    print(f"TED  B = {B_TED}: ted_beat_align ({n_on} onsets/clip)  {timed(lambda: pp.ted_beat_align(mask, slab, count), runs)}")
    print(f"BEAT B = {B_BEAT}:  beat_postprocess_timeline         {timed(lambda: pp.beat_postprocess_timeline(beat), runs)}")
    print(f"BEAT B = {B_BEAT}:  beat_postprocess per window x {W}   {timed(beat_post_slices, runs)}")
    print(f"BEAT B = {B_BEAT}:  beat_metrics_timeline             {timed(lambda: bm.beat_metrics_timeline(euler, target, None, onsets), runs)}")
    print(f"BEAT B = {B_BEAT}:  beat_metrics per window x {W}       {timed(beat_metrics_slices, runs)}")
    ted_bytes = B_TED * N * (27 * 4 + 27 * 4 + 30 * 4 + 4 + 1)
    post_bytes = B_BEAT * N * J * (6 * 4 + 6 * 4 + 3 * 4)
    met_bytes = B_BEAT * (N * J * (2 * 3 * 4 + 1) + 2 * 6 * N * 3 * 4 + 6 * (N - 1) * 5)
    red_bytes = B_BEAT * (N * J + (N - 1) + n_on * 4)
    print(f"algorithmic bytes: k_ted_timeline {ted_bytes / 1e6:.1f} MB, k_beat_post_timeline {post_bytes / 1e6:.1f} MB, "
          f"k_beat_metrics_timeline {met_bytes / 1e6:.1f} MB, k_beat_reduce_timeline {red_bytes / 1e6:.2f} MB, "
          f"k_ted_align {B_TED * (N + n_on * 4 + 16) / 1e6:.2f} MB")


if __name__ == "__main__":
    main()
