"""Long-form synthesis (long_form.sample_long: one engine call for W chained windows) against the loop a user of the per-clip API writes
(one ddim_sample_loop call per window, origin_x rebuilt from the previous sample in between), alternated in one process:

    python tools/long_form_time.py                 # long call vs per-window loop at three shapes (profiles/r12_long_form.md)
    python tools/long_form_time.py torch_cpu       # the same with the reference's CPU draws instead of Philox
    python tools/long_form_time.py trace           # a few long calls per shape and nothing else: run it under
                                                   # rocprofv3 --kernel-trace --stats -d <dir> -- python tools/long_form_time.py trace
                                                   # and read k_chain_window from the kernel stats (its bytes per launch are printed here)

TED, ddim100, skip_timesteps = 80 (20 steps per window), guidance 1.5, device-resident inputs, hipGraph replay.  The per-window loop
runs today's per-clip code paths unchanged.  Each call is timed by a host clock around work that ends in a device synchronise; the two
forms alternate ROUNDS times after a warm-up of both, the median of a round's calls is that round's figure, and the table gives the
median over rounds with their min .. max.  The shader clock (hwmon freq1_input of the card whose power moves most) is sampled alongside."""
import glob
import statistics
import sys
import threading
import time
from types import SimpleNamespace

import torch

sys.path.insert(0, ".")
from livelyspeaker_amd import long_form, synth                                        # noqa: E402
from livelyspeaker_amd.cfg_sampler import ClassifierFreeSampleModel                   # noqa: E402
from livelyspeaker_amd.model_util import create_model_and_diffusion, load_model_wo_clip   # noqa: E402

SHAPES = ((1, 30), (32, 8), (512, 4))
ROUNDS, SKIP, DEV = 5, 80, "cuda:0"


def build():
    cfg = synth.TED
    args = SimpleNamespace(mdm_condm="text", latent_dim=512, ff_size=1024, layers=8, cond_mask_prob=0.1, arch="trans_enc",
                           emb_trans_dec=False, dataset="humanml", lang_model=None, mlpact="silu", diffusion_steps=1000,
                           noise_schedule="cosine", sigma_small=True, lambda_vel=1.0, lambda_rcxyz=0.0, lambda_fc=0.0, njoints=9)
    model, diffusion = create_model_and_diffusion(args, "ddim100")
    load_model_wo_clip(model, {k: torch.from_numpy(v) for k, v in synth.make_state_dict(cfg).items()})
    return cfg, ClassifierFreeSampleModel(model).to(DEV).eval(), diffusion


def per_window(diffusion, model, cfg, y, W):
    B = y["audio"].shape[0]
    shape = (B, cfg.njoints, cfg.nfeats, cfg.nframes)
    prefix, wins = y["seed_poses"], []
    for w in range(W):
        origin_x = torch.zeros(shape, device=DEV)
        origin_x[..., :cfg.n_pre_seq] = prefix
        yy = {"audio_input": long_form.window_audio(y["audio"], w, cfg).contiguous(), "origin_x": origin_x,
              "vid_indices": y["vid_indices"], "scale": y["scale"]}
        s = diffusion.ddim_sample_loop(model, shape, clip_denoised=False, model_kwargs={"y": yy}, skip_timesteps=SKIP, progress=False,
                                       dump_steps=None, noise=None, const_noise=False)
        wins.append(s)
        prefix = s[..., cfg.nframes - cfg.n_pre_seq:]
    return torch.cat([wins[0]] + [s[..., cfg.n_pre_seq:] for s in wins[1:]], dim=-1)


def long_call(diffusion, model, cfg, y, W):
    return long_form.sample_long(diffusion, model, y["audio"], y["seed_poses"], y["vid_indices"], y["scale"], n_windows=W, sampler="ddim",
                                 skip_timesteps=SKIP)


def timed(fn, *a):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn(*a)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


class ClockSampler(threading.Thread):
    """sclk (MHz) of every amdgpu hwmon at ~50 Hz; the card whose power moves most is the one this process runs on."""

    def __init__(self):
        super().__init__(daemon=True)
        self.cards = []
        for hw in sorted(glob.glob("/sys/class/drm/card*/device/hwmon/hwmon*")):
            pw = sorted(glob.glob(hw + "/power1_average") + glob.glob(hw + "/power1_input"))
            ck = sorted(glob.glob(hw + "/freq1_input"))
            if pw and ck:
                self.cards.append((pw[0], ck[0], []))
        self.on = True

    @staticmethod
    def _read(path):
        try:
            with open(path) as f:
                return int(f.read().split()[0])
        except Exception:      # noqa: BLE001
            return None

    def run(self):
        while self.on:
            for pw, ck, rows in self.cards:
                w, hz = self._read(pw), self._read(ck)
                if w is not None and hz is not None:
                    rows.append((w / 1e6, hz / 1e6))
            time.sleep(0.02)

    def take(self):
        """'p10 / p50 / p90 MHz' of the busiest card since the last take."""
        best = max(self.cards, key=lambda c: (max(r[0] for r in c[2]) - min(r[0] for r in c[2])) if c[2] else -1.0, default=None)
        if best is None or len(best[2]) < 5:
            return "sclk not readable"
        clk = sorted(r[1] for r in best[2])
        text = f"sclk MHz p10 {clk[len(clk) // 10]:.0f} p50 {clk[len(clk) // 2]:.0f} p90 {clk[len(clk) * 9 // 10]:.0f} ({len(clk)} samples)"
        for c in self.cards:
            c[2].clear()
        return text


def chain_bytes(cfg, B, W):
    """Algorithmic bytes of the W + 1 k_chain_window launches of one call (csrc/ls_chain.hip), fp32."""
    JF, T, npre = cfg.jf, cfg.nframes, cfg.n_pre_seq
    KPP = (JF + 1 + 31) // 32 * 32
    cond = npre * (KPP + JF)                                    # feat_u prefix rows + origin_x prefix columns
    total = B * (npre * JF + cond)                              # window 0: seed poses in
    total += B * (W - 1) * (T * JF + cond + (T - npre) * JF)    # middle launches: sample in, conditioning + new frames out
    total += B * (T * JF + (T if W == 1 else T - npre) * JF)    # last launch: frames out only
    if W > 1:
        total += B * npre * JF                                  # window 0 leaves all T frames
    return 4 * total


def main():
    mode = sys.argv[1] if len(sys.argv) > 1 else "philox"
    cfg, model, diffusion = build()
    diffusion.noise_source = "torch_cpu" if mode == "torch_cpu" else "philox"
    diffusion.philox_seed = 1
    if mode == "trace":
        for B, W in SHAPES:
            y = {k: torch.from_numpy(v).to(DEV) for k, v in synth.make_long_cond(cfg, B, W).items()}
            for _ in range(4):
                long_call(diffusion, model, cfg, y, W)
            torch.cuda.synchronize()
            print(f"B={B} W={W}: {W + 1} k_chain_window launches per call, {chain_bytes(cfg, B, W)} algorithmic bytes per call "
                  f"({chain_bytes(cfg, B, W) / (W + 1):.0f} per launch)")
        return
    clocks = ClockSampler()
    clocks.start()
    print(f"# TED ddim100 skip {SKIP} (20 steps per window), CFG 1.5, noise {diffusion.noise_source}, device inputs; ms per call, "
          f"median over {ROUNDS} alternated rounds [min .. max of the rounds]")
    for B, W in SHAPES:
        reps = 3 if B >= 512 else 5
        y = {k: torch.from_numpy(v).to(DEV) for k, v in synth.make_long_cond(cfg, B, W).items()}
        for _ in range(2):                                          # warm-up of both forms: allocations, graph capture, clocks
            a = timed(per_window, diffusion, model, cfg, y, W)[1]
            b = timed(long_call, diffusion, model, cfg, y, W)[1]
        same = bool(torch.equal(a, b))                              # philox: per-call keys differ between the forms, so only torch_cpu can agree
        clocks.take()
        rounds = {"loop": [], "long": []}
        for _ in range(ROUNDS):
            for name, fn in (("loop", per_window), ("long", long_call)):
                if mode == "torch_cpu":
                    torch.manual_seed(1)
                rounds[name].append(statistics.median(timed(fn, diffusion, model, cfg, y, W)[0] for _ in range(reps)))
        t = model.model.engine().timing()
        med = {k: statistics.median(v) for k, v in rounds.items()}
        print(f"B={B:4d} W={W:3d} ({34 + (W - 1) * 30} frames): per-window loop {med['loop']:9.2f} [{min(rounds['loop']):.2f} .. {max(rounds['loop']):.2f}]  "
              f"long call {med['long']:9.2f} [{min(rounds['long']):.2f} .. {max(rounds['long']):.2f}]  ratio {med['loop'] / med['long']:.2f}x  "
              f"| long call: prepare {t['prepare_ms']:.2f} ms, windows {t['total_ms']:.2f} ms, graph replayed for {t['graph_replayed']} of {W} windows, "
              f"step path {t['step_path']} | {clocks.take()}" + (f" | outputs equal: {same}" if mode == "torch_cpu" else ""), flush=True)
    clocks.on = False


if __name__ == "__main__":
    main()
