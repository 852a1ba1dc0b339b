"""Times of the score stream (postprocess.open_score_stream, long_form.score_talk); the figures of profiles/r29_score_stream.md:

    python tools/score_stream_time.py

1. The finish at F = 4096 audio frames and N = 4096 pose frames for S in {1, 8, 32} slots, against what the whole-clip entries take for
   the same data in the same process, alternated run by run: ``audio_onsets(want=count, onset_raw)``'s pick kernel (its event pair,
   ``kernel_ms[1]``) plus ``ted_beat_align`` (host clock).  The finish is timed by a host clock around the call, which ends in its own
   device waits: per slot nine launches of the tiled pick, two of the alignment sum, a wait and the copies out.
2. The spectrum part of a push: 2 s of audio per slot at S in {1, 8, 32}, against ``audio_onsets(want=('mel_db',))`` on the same
   samples (device input, host clock around work that ends in a device synchronise).
3. The finish and ``device_bytes`` of one slot at 15 and 60 minutes of audio.
4. ``score_talk`` for 15 minutes (13 500 pose frames, 14.4 M samples), against nothing: the whole-clip entries refuse it."""
import sys
import time

import numpy as np

sys.path.insert(0, ".")
sys.path.insert(0, "tests")
from livelyspeaker_amd import audio_onsets as ao, long_form, postprocess as pp  # noqa: E402

SR, RUNS = 16000, 7


def clock(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def fmt(v):
    return f"{np.median(v):.3f} ({min(v):.3f} .. {max(v):.3f})"


def speech(n, seed):
    import onsets_restatement as R
    return np.concatenate([R.test_clip(seed + i, 36267) for i in range(-(-n // 36267))])[:n]


def fill(ss, audio, masks, step=32000):
    """audio [S, L] (device), masks [S, N] (host bool): everything a finish needs, in pushes of ``step`` samples."""
    S, L = audio.shape
    for c0 in range(0, L, step):
        ss.push(audio=audio[:, c0:c0 + step])
    for t0 in range(0, masks.shape[1], 4096):
        m = masks[:, t0:t0 + 4096]
        ss.push(beats={"beat_mask": m, "beat_first": np.full(S, t0), "beat_count": np.full(S, m.shape[1])})


def finish_at_the_limit():
    import torch
    print("## 1. finish at F = 4096, N = 4096 (ms, median (min .. max) of %d alternated runs)" % RUNS)
    L, N = 4095 * 512, 4096
    for S in (1, 8, 32):
        rng = np.random.default_rng(S)
        audio = torch.from_numpy(np.stack([speech(L, 100 * s) for s in range(S)])).cuda()
        masks = rng.uniform(size=(S, N)) < 0.15
        dmask = torch.from_numpy(masks).cuda()
        ss = pp.open_score_stream("ted", S, max(L / SR, N / 15.0) + 1, max_chunk=32000)
        mine, pick, align = [], [], []
        for run in range(RUNS + 2):
            fill(ss, audio, masks)
            t, res = clock(lambda: ss._finish(range(S)))
            ms = []
            on = ao.audio_onsets(audio, SR, want=("count", "onset_raw"), timing=ms)
            ta, (total, beats) = clock(lambda: pp.ted_beat_align(dmask, on["onset_raw"], on["count"]))
            assert all(res[s]["align_sum"] == total[s] and res[s]["count"] == on["counts"][s] for s in range(S))
            if run >= 2:
                mine.append(t), pick.append(ms[1]), align.append(ta)
        parent = np.array(pick) + np.array(align)
        print(f"S = {S:2d}: finish {fmt(mine)}; parent pick kernel {fmt(pick)} + ted_beat_align call {fmt(align)} = {fmt(parent)}; "
              f"ratio {np.median(mine) / np.median(parent):.2f}; device_bytes {ss.device_bytes / 1e6:.1f} MB")
        ss.close()


def spectrum_of_a_push():
    import torch
    print("## 2. the spectrum part of a push: 2 s of audio per slot (ms)")
    n = 2 * SR
    for S in (1, 8, 32):
        audio = torch.from_numpy(np.stack([speech(8 * n, 7 * s) for s in range(S)])).cuda()
        ss = pp.open_score_stream("ted", S, 8 * n / SR + 1, max_chunk=n)
        mine, whole = [], []
        for run in range(8):
            piece = audio[:, run * n:(run + 1) * n].contiguous()
            t, _ = clock(lambda: ss.push(audio=piece))
            tw, _ = clock(lambda: ao.audio_onsets(piece, SR, want=("mel_db",)))
            if run >= 2:
                mine.append(t), whole.append(tw)
        print(f"S = {S:2d}: push {fmt(mine)}; audio_onsets(want=mel_db) on the same samples {fmt(whole)}; ratio {np.median(mine) / np.median(whole):.2f}")
        ss.close()


def long_talks():
    import torch
    print("## 3. one slot at 15 and 60 minutes of audio")
    for minutes in (15, 60):
        L = minutes * 60 * SR
        audio = torch.from_numpy(speech(L, 5)[None]).cuda()
        masks = np.random.default_rng(minutes).uniform(size=(1, minutes * 60 * 15)) < 0.15
        ss = pp.open_score_stream("ted", 1, minutes * 60 + 1, max_chunk=1 << 20)
        times = []
        for run in range(3):
            t_fill, _ = clock(lambda: fill(ss, audio, masks, 1 << 20))
            t, res = clock(lambda: ss._finish([0]))
            times.append(t)
        r = res[0]
        print(f"{minutes} min: {r['n_frames']} audio frames, {r['count']} onsets, {r['n_beats']} motion beats; finish {fmt(times)} ms; "
              f"feeding it in 65 s pushes {t_fill:.1f} ms; device_bytes {ss.device_bytes / 1e6:.1f} MB")
        ss.close()


def a_quarter_of_an_hour():
    import torch
    print("## 4. score_talk, 15 minutes")
    N, L = 13500, 900 * SR
    rng = np.random.default_rng(3)
    z = np.cumsum(rng.standard_normal((27, N)) * 0.02, axis=1).astype(np.float32)
    x = torch.from_numpy((z - z.mean(1, keepdims=True)).reshape(1, 9, 3, N)).cuda()
    y = torch.from_numpy(speech(L, 11)[None]).cuda()
    times = []
    for run in range(3):
        t, res = clock(lambda: long_form.score_talk(x, y, "ted"))
        times.append(t)
    print(f"score_talk(ted, N = {N}, L = {L}): {fmt(times)} ms; bc {res['bc']:.4f}, {int(res['onset_count'][0])} onsets, "
          f"{len(res['motion_beat_times'][0])} motion beats")


if __name__ == "__main__":
    finish_at_the_limit()
    spectrum_of_a_push()
    long_talks()
    a_quarter_of_an_hour()
