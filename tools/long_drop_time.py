"""Time of sample_long(audio_lengths=, drop_finished=True) next to the same call with drop_finished=False, which runs every clip for
the windows of the longest one:

    python tools/long_drop_time.py               # the figures of profiles/r17_drop_finished.md
    python tools/long_drop_time.py --rounds 9 --only readme,spread32

The batches: the README's three speeches (20, 45.5 and 8 s) and speeches spread evenly over 12.5 .. 100 s (tools/ragged_time.py's
spread: one to four windows) at B = 32 and B = 512, shuffled.  TED, ddim100, skip_timesteps = 80 (20 steps per window), guidance
scale 2.5, device-resident inputs, noise_source 'philox' and 'torch_cpu' (whose host draws are inside the clock: they are part of the
call).  A call time is a host clock around the call and a device synchronise.  The two variants are ALTERNATED round by round in one
process, so that clock and thermal drift hits both alike; the figure is the median over the rounds, with the spread (min .. max)
next to it, and the share of clip-windows the dropping call samples, sum B_w / (B * W_max), for comparison."""
import os
import sys
import time
from types import SimpleNamespace

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from livelyspeaker_amd import long_form, synth                                        # noqa: E402
from livelyspeaker_amd.cfg_sampler import ClassifierFreeSampleModel                   # noqa: E402
from livelyspeaker_amd.model_util import create_model_and_diffusion, load_model_wo_clip   # noqa: E402

SR = 16000


def build():
    import torch
    args = SimpleNamespace(mdm_condm="text", latent_dim=512, ff_size=1024, layers=8, cond_mask_prob=0.1, arch="trans_enc",
                           emb_trans_dec=False, dataset="humanml", lang_model=None, mlpact="silu", diffusion_steps=1000,
                           noise_schedule="cosine", sigma_small=True, lambda_vel=1.0, lambda_rcxyz=0.0, lambda_fc=0.0, njoints=9)
    model, diffusion = create_model_and_diffusion(args, "ddim100")
    load_model_wo_clip(model, {k: torch.from_numpy(v) for k, v in synth.make_state_dict(synth.TED).items()})
    model = ClassifierFreeSampleModel(model).to("cuda:0")
    model.eval()
    return model, diffusion


def batches():
    g = np.random.default_rng(0)
    out = {"readme": np.array([20.0, 45.5, 8.0])}
    for B in (32, 512):
        seconds = np.linspace(12.5, 100.0, B)
        g.shuffle(seconds)
        out[f"spread{B}"] = seconds
    return out


def main():
    import torch
    rounds = int(sys.argv[sys.argv.index("--rounds") + 1]) if "--rounds" in sys.argv else 15
    only = sys.argv[sys.argv.index("--only") + 1].split(",") if "--only" in sys.argv else None
    cfg = synth.TED
    model, diffusion = build()
    print(f"TED ddim100 skip 80; {rounds} alternated rounds, median (min .. max) in ms")
    for name, seconds in batches().items():
        if only and name not in only:
            continue
        B = len(seconds)
        lengths = np.maximum(1, np.round(seconds * SR)).astype(np.int64)
        active = long_form.plan_drop(lengths, cfg)[2]
        W = len(active)
        share = float(active.sum()) / (B * W)
        audio = 0.1 * torch.randn((B, int(lengths.max())), device="cuda:0", generator=torch.Generator("cuda:0").manual_seed(1))
        y = {k: torch.from_numpy(v).cuda() for k, v in synth.make_long_cond(cfg, B, 1, scale=2.5).items() if k != "audio"}
        print(f"{name}: B = {B}, W_max = {W}, clips per window {active.tolist()}: {int(active.sum())} of {B * W} clip-windows "
              f"(share {share:.3f})")
        for source in ("philox", "torch_cpu"):
            diffusion.noise_source = source
            call = lambda drop: long_form.sample_long(diffusion, model, audio, y["seed_poses"], y["vid_indices"], y["scale"],      # noqa: E731
                                                      sampler="ddim", skip_timesteps=80, audio_lengths=lengths, drop_finished=drop)
            slow = source == "torch_cpu" and B >= 512           # the host draws of such a call take seconds
            n, warm = (max(3, rounds // 3), 1) if slow else (rounds, 2)
            ms = [[], []]
            try:
                for r in range(n + warm):                     # warm rounds are not recorded
                    for i, drop in enumerate((True, False)):
                        torch.manual_seed(5)
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        call(drop)
                        torch.cuda.synchronize()
                        if r >= warm:
                            ms[i].append((time.perf_counter() - t0) * 1e3)
            except ValueError as e:                           # one window's tape beyond tape_segment_bytes
                print(f"  {source:9s} refused: {e}")
                continue
            med = [float(np.median(m)) for m in ms]
            for label, m, md in zip(("drop_finished", "all windows"), ms, med):
                print(f"  {source:9s} {label:13s} {md:9.2f} ({min(m):.2f} .. {max(m):.2f})")
            print(f"  {source:9s} drop / all = {med[0] / med[1]:.3f} (clip-window share {share:.3f}), {n} rounds")


if __name__ == "__main__":
    main()
