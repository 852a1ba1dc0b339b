"""noise_source='torch_device' against the other noise sources, per sampling call of a whole loop (DDPM, CFG 1.5, synthetic weights):
  torch_device  the reference's GPU-run draws generated on the device inside the captured loop (csrc/ls_torch_philox.hip)
  tape_device   TAPE mode on a pre-drawn device-resident tape of the same draws (engine level: the loop with no generator in it)
  philox        the project's own keyed stream (throughput mode)
  torch_cpu     the reference's CPU-run draws (host stream, page-locked segments)
Prints one JSON line per (config, mode): the engine's loop_ms (first step launch .. last step done), the wall time of the call and
pose-frames/s = B * nframes / wall seconds.
python tools/device_rng_time.py [ted|beat] [B] [steps] [modes, comma-separated] [reps]"""
import json
import sys
import time
from types import SimpleNamespace

sys.path.insert(0, ".")
import torch  # noqa: E402

from livelyspeaker_amd import synth  # noqa: E402
from livelyspeaker_amd.cfg_sampler import ClassifierFreeSampleModel  # noqa: E402
from livelyspeaker_amd.model_util import create_model_and_diffusion  # noqa: E402

ds = sys.argv[1] if len(sys.argv) > 1 else "ted"
B = int(sys.argv[2]) if len(sys.argv) > 2 else 512
steps = int(sys.argv[3]) if len(sys.argv) > 3 else 1000
modes = sys.argv[4].split(",") if len(sys.argv) > 4 else ["torch_device", "tape_device", "philox", "torch_cpu"]
reps = int(sys.argv[5]) if len(sys.argv) > 5 else 3
dev = torch.device("cuda", 0)

cfg = synth.CONFIGS[ds]
args = SimpleNamespace(mdm_condm="text", latent_dim=512, ff_size=1024, layers=8, cond_mask_prob=0.1, arch="trans_enc", emb_trans_dec=False,
                       dataset="humanml", lang_model=None, mlpact="silu", diffusion_steps=steps, noise_schedule="cosine", sigma_small=True,
                       lambda_vel=1.0, lambda_rcxyz=0.0, lambda_fc=0.0, njoints=cfg.njoints)
rag, diffusion = create_model_and_diffusion(args, "", dataset=ds)
rag.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_state_dict(cfg).items()}, strict=False)
rag.to(dev).eval()
model = ClassifierFreeSampleModel(rag)
y = {k: torch.from_numpy(v).to(dev) for k, v in synth.make_cond(cfg, B).items()}
shape = (B, cfg.njoints, cfg.nfeats, cfg.nframes)
eng = diffusion._bind_schedule(rag._engine_prepared(y))

for mode in modes:
    if mode == "tape_device":
        torch.manual_seed(1)
        x_T = torch.randn(*shape, device=dev)
        eps = torch.randn(steps, 2, B, 512, device=dev)
        nz = torch.randn((steps,) + shape, device=dev)

        def call():
            return eng.sample(x_init=x_T, eps_tape=eps, noise_tape=nz)
    else:
        diffusion.noise_source = mode

        def call():
            return diffusion.p_sample_loop(model, shape, clip_denoised=False, model_kwargs={"y": y}, progress=False)
    torch.cuda.manual_seed(233)
    call()                                  # warm-up: graph capture, allocations, the once-per-process self-check
    torch.cuda.synchronize()
    loop, wall = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = call()
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
        loop.append(eng.timing()["loop_ms"])
        del out
    if mode == "tape_device":
        del x_T, eps, nz
        torch.cuda.empty_cache()
    w = min(wall)
    print(json.dumps({"config": f"{ds} B={B} DDPM {steps} steps", "mode": mode, "loop_ms": [round(v, 2) for v in loop],
                      "wall_ms": [round(v, 2) for v in wall], "loop_ms_per_step": round(min(loop) / steps, 4),
                      "pose_frames_per_s": round(B * cfg.nframes / (w / 1e3), 1),
                      "native": bool(getattr(diffusion, "last_device_rng_native", False)) if mode == "torch_device" else None}), flush=True)
