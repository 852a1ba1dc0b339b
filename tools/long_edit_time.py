"""Editing a long-form timeline (long_form.edit_long: only the windows a frame range touches are sampled) against sampling the whole
timeline again (long_form.sample_long of the same W), alternated in one process:

    python tools/long_edit_time.py                 # 60 s of speech, 64 clips (profiles/r19_long_edit.md)
    python tools/long_edit_time.py 20 8            # seconds, clips
    python tools/long_edit_time.py --sag [20 8]    # the SCRIPTED edit two ways (profiles/r26_long_edit_sag.md)
    python tools/long_edit_time.py --compact [--sag] [20 8]    # the dense against the COMPACT edit (profiles/r31_edit_compact.md)
    python tools/long_edit_time.py --mask [20 8]   # two stretches as ONE mask call against TWO range calls (profiles/r32_edit_mask.md)

TED, ddim100, skip_timesteps = 80 (20 steps per window), guidance 1.5, Philox noise, device-resident inputs, hipGraph replay, warm
handles.  Three forms: the full call, an edit inside one window, and an edit that spans W // 2 windows.  Each call is timed by a host
clock around work that ends in a device synchronise; the forms alternate ROUNDS times after a warm-up of all three, the median of a
round's calls is that round's figure, and the table gives the median over rounds with their min .. max, next to the engine's own
event times of the last call of each form (prepare: ls_long_prepare, the same for all three; windows: the sampling alone).  The shader
clock is sampled alongside (long_form_time.ClockSampler).

What to check (derived, not measured): the windows' time scales with |Wset| / W; each step costs about one elementwise launch more
than in the full call (the inpainting branch runs the denoiser and the update as two launches); prepare is unchanged.

--sag times the script-guided edit of the `one` and `half` ranges two ways, alternated in the same manner: edit_long(sag=,
text_features=) -- one engine call -- and the host loop it replaces, "for w in edit_plan: edit_window -> decoder -> edit_start ->
ddim_sample_loop(init_image=) -> write-back", through the public per-clip API (which encodes a window's audio when it samples it,
where edit_long encodes all W windows ahead; both are part of what a caller waits for and both are inside the timed call).

--compact alternates edit_long(compact=False) and edit_long(compact=True) of the same ranges, round by round, in three cases: (a) one
clip in one window, (b) 8 clips each in a window of its own, (c) every clip in W // 2 windows, where the compact plan is the dense one
and the results are checked to be the same bits.  With --sag the edits are scripted, and (a) is timed against the host loop too.

--mask alternates, round by round, two stretches of clip 0 (ten frames each, in two windows a quarter of the timeline apart) edited as
ONE call of edit_long(mask=) and as TWO calls of edit_long(frames=) -- the second on the first one's result --, each in the compact and
in the dense form.  The mask lives on the device, as the timeline does.  Under Philox the two ways draw the same streams, so the tool
checks, form by form, that they give the same bits before it times them."""
import os
import statistics
import sys

import torch

sys.path.insert(0, ".")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from livelyspeaker_amd import long_form, synth                                        # noqa: E402
from long_form_time import DEV, ROUNDS, SKIP, ClockSampler, build, timed              # noqa: E402


def host_loop(diffusion, model, sag, text, cfg, y, timeline, frames, W):
    """The scripted edit through the public API: one sampling call per window of edit_plan."""
    tl = timeline.clone()
    B, T, S = tl.shape[0], cfg.nframes, cfg.nframes - cfg.n_pre_seq
    shape = (B, cfg.njoints, cfg.nfeats, T)
    ones = torch.ones(B, T, device=DEV).bool()
    for w in long_form.edit_plan(frames, W, cfg):
        origin_x, mask, motion = long_form.edit_window(tl, w, frames, None, y["seed_poses"], cfg)
        init = long_form.edit_start(motion, mask, sag({"x": origin_x.clone(), "z": text[:, w].contiguous(), "mask": ones})["output"])
        yy = {"audio_input": long_form.window_audio(y["audio"], w, cfg).contiguous(), "origin_x": origin_x, "vid_indices": y["vid_indices"],
              "scale": y["scale"], "inpainting_mask": mask, "inpainted_motion": motion}
        s = diffusion.ddim_sample_loop(model, shape, clip_denoised=False, model_kwargs={"y": yy}, skip_timesteps=SKIP, init_image=init,
                                       progress=False, dump_steps=None, noise=None, const_noise=False)
        tl[..., w * S:w * S + T] = torch.where(mask, motion, s)
    return tl


def main_sag(seconds, B):
    from livelyspeaker_amd.motionclip_module import Decoder_TRANSFORMER
    cfg, model, diffusion = build()
    diffusion.noise_source, diffusion.philox_seed = "philox", 1
    sag = Decoder_TRANSFORMER(njoints=cfg.njoints, nfeats=cfg.nfeats, latent_dim=512, n_pre_poses=cfg.n_pre_seq, use_style=False)
    sag.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_sag_state_dict(cfg).items()}, strict=False)
    sag.to(DEV).eval()
    W, _, n_frames = long_form.plan_windows(int(round(seconds * 16000)), cfg)
    y = {k: torch.from_numpy(v).to(DEV) for k, v in synth.make_long_cond(cfg, B, W).items()}
    text = torch.from_numpy(synth.make_text_features(B * W).reshape(B, W, 512)).to(DEV)
    S = cfg.nframes - cfg.n_pre_seq
    mid, half_lo = W // 2, (W // 4) * S + 10
    ranges = {"one": (mid * S + 10, mid * S + 20), "half": (half_lo, half_lo + (W // 2 - 1) * S + 5)}
    timeline = long_form.sample_long(diffusion, model, y["audio"], y["seed_poses"], y["vid_indices"], y["scale"], n_windows=W, sampler="ddim",
                                     skip_timesteps=SKIP, sag=sag, text_features=text)

    def call(frames):
        return long_form.edit_long(diffusion, model, timeline, frames, y["audio"], y["seed_poses"], y["vid_indices"], y["scale"], sampler="ddim",
                                   skip_timesteps=SKIP, sag=sag, text_features=text)

    forms = []
    for name, frames in ranges.items():
        forms.append((name, "loop", lambda frames=frames: host_loop(diffusion, model, sag, text, cfg, y, timeline, frames, W)))
        forms.append((name, "call", lambda frames=frames: call(frames)))
    clocks = ClockSampler()
    clocks.start()
    for _ in range(2):                                               # warm-up of all forms: allocations, graph capture, clocks
        for _, _, fn in forms:
            timed(fn)
    clocks.take()
    reps = 3
    rounds, engine = {(n, k): [] for n, k, _ in forms}, {}
    for _ in range(ROUNDS):
        for name, kind, fn in forms:
            rounds[name, kind].append(statistics.median(timed(fn)[0] for _ in range(reps)))
            if kind == "call":
                engine[name] = model.model.engine().timing()
    print(f"# scripted edit; TED ddim100 skip {SKIP} (20 steps per window), CFG 1.5, philox, device inputs; {seconds:g} s of speech = {W} "
          f"windows ({n_frames} frames), {B} clips; ms per call, median over {ROUNDS} alternated rounds [min .. max of the rounds]")
    for name, frames in ranges.items():
        lp, cl, t = rounds[name, "loop"], rounds[name, "call"], engine[name]
        n_run = len(long_form.edit_plan(frames, W, cfg))
        print(f"{name:5s} {n_run:3d} of {W} windows: host loop {statistics.median(lp):9.2f} [{min(lp):.2f} .. {max(lp):.2f}]  edit_long(sag=) "
              f"{statistics.median(cl):9.2f} [{min(cl):.2f} .. {max(cl):.2f}]  ratio {statistics.median(lp) / statistics.median(cl):.2f}x  | edit_long: "
              f"prepare {t['prepare_ms']:.2f} ms, windows {t['total_ms']:.2f} ms ({t['total_ms'] / n_run:.3f} per window), graph replayed for "
              f"{t['graph_replayed']} of {t['n_segments']} windows, step path {t['step_path']}", flush=True)
    print(f"# {clocks.take()}")
    clocks.on = False


def main_compact(seconds, B, scripted):
    """The dense and the compact form of the same edit, alternated round by round (profiles/r31_edit_compact.md): (a) one clip, one
    window; (b) 8 clips, each in a window of its own; (c) every clip in W // 2 windows (the identity plan).  scripted: with the SAG
    decoder, and (a) against the host loop of main_sag as well."""
    import numpy as np
    cfg, model, diffusion = build()
    diffusion.noise_source, diffusion.philox_seed = "philox", 1
    W, _, n_frames = long_form.plan_windows(int(round(seconds * 16000)), cfg)
    y = {k: torch.from_numpy(v).to(DEV) for k, v in synth.make_long_cond(cfg, B, W).items()}
    S = cfg.nframes - cfg.n_pre_seq
    mid, half_lo, n8 = W // 2, (W // 4) * S + 10, min(8, B, W)
    a = np.zeros((B, 2), np.int64)
    a[0] = (mid * S + 10, mid * S + 20)
    b = np.zeros((B, 2), np.int64)
    for k in range(n8):                                              # clip k inside the frames window first + k owns
        w = max(0, mid - n8 // 2) + k
        b[k] = (w * S + 10, w * S + 20)
    c = np.tile(np.array([(half_lo, half_lo + (W // 2 - 1) * S + 5)], np.int64), (B, 1))
    cases = {"a": a, "b": b, "c": c}
    kw, sag, text = {}, None, None
    if scripted:
        from livelyspeaker_amd.motionclip_module import Decoder_TRANSFORMER
        sag = Decoder_TRANSFORMER(njoints=cfg.njoints, nfeats=cfg.nfeats, latent_dim=512, n_pre_poses=cfg.n_pre_seq, use_style=False)
        sag.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_sag_state_dict(cfg).items()}, strict=False)
        sag.to(DEV).eval()
        text = torch.from_numpy(synth.make_text_features(B * W).reshape(B, W, 512)).to(DEV)
        kw = dict(sag=sag, text_features=text)
    timeline = long_form.sample_long(diffusion, model, y["audio"], y["seed_poses"], y["vid_indices"], y["scale"], n_windows=W, sampler="ddim",
                                     skip_timesteps=SKIP, **kw)

    def call(frames, compact):
        return long_form.edit_long(diffusion, model, timeline, frames, y["audio"], y["seed_poses"], y["vid_indices"], y["scale"], sampler="ddim",
                                   skip_timesteps=SKIP, compact=compact, **kw)

    forms = []
    for name, frames in cases.items():
        if scripted and name == "a":
            forms.append((name, "loop", lambda frames=frames: host_loop(diffusion, model, sag, text, cfg, y, timeline, frames, W)))
        forms.append((name, "dense", lambda frames=frames: call(frames, False)))
        forms.append((name, "compact", lambda frames=frames: call(frames, True)))
    # the identity plan gives the dense call's bits; elsewhere the compact form changes the same elements and no other
    assert torch.equal(call(c, True), call(c, False))
    for frames in (a, b):
        got, ref = call(frames, True), call(frames, False)
        assert torch.equal(got != timeline, ref != timeline) and bool(torch.isfinite(got).all())
    clocks = ClockSampler()
    clocks.start()
    for _ in range(2):                                               # warm-up of all forms: allocations, graph capture, clocks
        for _, _, fn in forms:
            timed(fn)
    clocks.take()
    reps = 3
    rounds, engine = {(n, k): [] for n, k, _ in forms}, {}
    for _ in range(ROUNDS):
        for name, kind, fn in forms:
            rounds[name, kind].append(statistics.median(timed(fn)[0] for _ in range(reps)))
            if kind != "loop":
                engine[name, kind] = model.model.engine().timing()
    print(f"# dense against compact edit_long{' (scripted)' if scripted else ''}; TED ddim100 skip {SKIP} (20 steps per window), CFG 1.5, philox, "
          f"device inputs; {seconds:g} s of speech = {W} windows ({n_frames} frames), {B} clips; ms per call, median over {ROUNDS} alternated "
          f"rounds [min .. max of the rounds]; prepare / windows: the engine's event times of the last call")
    for name, frames in cases.items():
        plan = long_form.edit_plan_compact(frames, W, cfg)
        pairs = sum(len(rows) for _, rows in plan)
        print(f"case {name}: {len(plan)} windows, {pairs} clip-windows of {len(plan) * B} dense ({W * B} encoded by the dense form)")
        for kind in ("loop", "dense", "compact"):
            if (name, kind) not in rounds:
                continue
            r = rounds[name, kind]
            line = f"  {kind:8s} {statistics.median(r):9.2f} [{min(r):.2f} .. {max(r):.2f}]"
            if kind != "loop":
                t = engine[name, kind]
                line += (f"  | prepare {t['prepare_ms']:.2f} ms, windows {t['total_ms']:.2f} ms, {t['n_step_launches']} steps, graph replayed for "
                         f"{t['graph_replayed']} of {t['n_segments']} windows, step path {t['step_path']}")
            print(line, flush=True)
        d, cpt = rounds[name, "dense"], rounds[name, "compact"]
        print(f"  dense / compact {statistics.median(d) / statistics.median(cpt):.2f}x; compact faster in {sum(p < q for p, q in zip(cpt, d))} of"
              f"{ROUNDS} rounds; dense spread {max(d) - min(d):.2f} ms, median difference {statistics.median(cpt) - statistics.median(d):+.2f} ms")
    print(f"# {clocks.take()}")
    clocks.on = False


def main_mask(seconds, B):
    """Two stretches of one clip as one mask call against two range calls, compact and dense (profiles/r32_edit_mask.md)."""
    import numpy as np
    cfg, model, diffusion = build()
    diffusion.noise_source, diffusion.philox_seed = "philox", 1
    W, _, n_frames = long_form.plan_windows(int(round(seconds * 16000)), cfg)
    y = {k: torch.from_numpy(v).to(DEV) for k, v in synth.make_long_cond(cfg, B, W).items()}
    S = cfg.nframes - cfg.n_pre_seq
    w1, w2 = W // 4, (3 * W) // 4
    stretches = [(w1 * S + 10, w1 * S + 20), (w2 * S + 10, w2 * S + 20)]
    ranges = []
    for lo, hi in stretches:
        r = np.zeros((B, 2), np.int64)
        r[0] = (lo, hi)
        ranges.append(r)
    host_mask = np.zeros((B, n_frames), bool)
    for lo, hi in stretches:
        host_mask[0, lo:hi] = True
    mask = torch.from_numpy(host_mask).to(DEV)
    timeline = long_form.sample_long(diffusion, model, y["audio"], y["seed_poses"], y["vid_indices"], y["scale"], n_windows=W, sampler="ddim",
                                     skip_timesteps=SKIP)

    def call(tl, compact, **what):
        return long_form.edit_long(diffusion, model, tl, what.get("frames"), y["audio"], y["seed_poses"], y["vid_indices"], y["scale"], sampler="ddim",
                                   skip_timesteps=SKIP, compact=compact, mask=what.get("mask"))

    def one_call(compact):
        return call(timeline, compact, mask=mask)

    def two_calls(compact):
        return call(call(timeline, compact, frames=ranges[0]), compact, frames=ranges[1])

    forms = [("compact", "mask", lambda: one_call(True)), ("compact", "ranges", lambda: two_calls(True)),
             ("dense", "mask", lambda: one_call(False)), ("dense", "ranges", lambda: two_calls(False))]
    plan = long_form.edit_plan_compact(None, W, cfg, mask=host_mask)
    assert plan == [(w1, [0]), (w2, [0])] and w1 != w2, plan
    for compact in (True, False):                                    # the same keys, the same windows at the same batch: the same bits
        ref = two_calls(compact)
        assert torch.equal(one_call(compact), ref) and not torch.equal(ref, timeline), compact
    clocks = ClockSampler()
    clocks.start()
    for _ in range(2):                                               # warm-up of all forms: allocations, graph capture, clocks
        for _, _, fn in forms:
            timed(fn)
    clocks.take()
    reps = 3
    rounds, engine = {(f, k): [] for f, k, _ in forms}, {}
    for _ in range(ROUNDS):
        for form, kind, fn in forms:
            rounds[form, kind].append(statistics.median(timed(fn)[0] for _ in range(reps)))
            engine[form, kind] = model.model.engine().timing()
    print(f"# one mask call against two range calls; TED ddim100 skip {SKIP} (20 steps per window), CFG 1.5, philox, device inputs and a device "
          f"mask; {seconds:g} s of speech = {W} windows ({n_frames} frames), {B} clips; clip 0 on frames {stretches}: windows {w1} and {w2}; ms, "
          f"median over {ROUNDS} alternated rounds [min .. max of the rounds]; prepare / windows: the engine's event times of the LAST call "
          f"(of two range calls: the second, one window)")
    for form in ("compact", "dense"):
        for kind in ("mask", "ranges"):
            r, t = rounds[form, kind], engine[form, kind]
            print(f"  {form:8s} {'one mask call  ' if kind == 'mask' else 'two range calls'} {statistics.median(r):9.2f} [{min(r):.2f} .. {max(r):.2f}]  | "
                  f"prepare {t['prepare_ms']:.2f} ms, windows {t['total_ms']:.2f} ms, {t['n_step_launches']} steps, graph replayed for "
                  f"{t['graph_replayed']} of {t['n_segments']} windows, step path {t['step_path']}", flush=True)
        m, r = rounds[form, "mask"], rounds[form, "ranges"]
        print(f"  {form}: two calls - one call = {statistics.median(r) - statistics.median(m):+.2f} ms ({statistics.median(r) / statistics.median(m):.2f}x); "
              f"the mask call faster in {sum(p < q for p, q in zip(m, r))} of {ROUNDS} rounds; spread of the mask call {max(m) - min(m):.2f} ms")
    print(f"# {clocks.take()}")
    clocks.on = False


def main():
    if "--mask" in sys.argv:
        sys.argv.remove("--mask")
        return main_mask(float(sys.argv[1]) if len(sys.argv) > 1 else 60.0, int(sys.argv[2]) if len(sys.argv) > 2 else 64)
    if "--compact" in sys.argv:
        sys.argv.remove("--compact")
        scripted = "--sag" in sys.argv
        if scripted:
            sys.argv.remove("--sag")
        return main_compact(float(sys.argv[1]) if len(sys.argv) > 1 else 60.0, int(sys.argv[2]) if len(sys.argv) > 2 else 64, scripted)
    if "--sag" in sys.argv:
        sys.argv.remove("--sag")
        return main_sag(float(sys.argv[1]) if len(sys.argv) > 1 else 60.0, int(sys.argv[2]) if len(sys.argv) > 2 else 64)
    seconds = float(sys.argv[1]) if len(sys.argv) > 1 else 60.0
    B = int(sys.argv[2]) if len(sys.argv) > 2 else 64
    cfg, model, diffusion = build()
    diffusion.noise_source, diffusion.philox_seed = "philox", 1
    W, _, n_frames = long_form.plan_windows(int(round(seconds * 16000)), cfg)
    y = {k: torch.from_numpy(v).to(DEV) for k, v in synth.make_long_cond(cfg, B, W).items()}
    S = cfg.nframes - cfg.n_pre_seq
    mid = W // 2
    one = (mid * S + 10, mid * S + 20)                               # inside the frames window `mid` owns
    half_lo = (W // 4) * S + 10
    half = (half_lo, half_lo + (W // 2 - 1) * S + 5)                 # the frames W // 2 consecutive windows own
    plans = {"one": long_form.edit_plan(one, W, cfg), "half": long_form.edit_plan(half, W, cfg)}
    assert len(plans["one"]) == 1 and len(plans["half"]) == max(1, W // 2), plans

    def full():
        return long_form.sample_long(diffusion, model, y["audio"], y["seed_poses"], y["vid_indices"], y["scale"], n_windows=W, sampler="ddim",
                                     skip_timesteps=SKIP)

    timeline = full()

    def edit(frames):
        return long_form.edit_long(diffusion, model, timeline, frames, y["audio"], y["seed_poses"], y["vid_indices"], y["scale"], sampler="ddim",
                                   skip_timesteps=SKIP)

    forms = (("full", full), ("one", lambda: edit(one)), ("half", lambda: edit(half)))
    clocks = ClockSampler()
    clocks.start()
    for _ in range(2):                                               # warm-up of all forms: allocations, graph capture, clocks
        for _, fn in forms:
            timed(fn)
    clocks.take()
    reps = 3
    rounds, engine = {k: [] for k, _ in forms}, {}
    for _ in range(ROUNDS):
        for name, fn in forms:
            rounds[name].append(statistics.median(timed(fn)[0] for _ in range(reps)))
            engine[name] = model.model.engine().timing()
    print(f"# TED ddim100 skip {SKIP} (20 steps per window), CFG 1.5, philox, device inputs; {seconds:g} s of speech = {W} windows "
          f"({n_frames} frames), {B} clips; ms per call, median over {ROUNDS} alternated rounds [min .. max of the rounds]")
    med = {k: statistics.median(v) for k, v in rounds.items()}
    for name, _ in forms:
        t = engine[name]
        n_run = W if name == "full" else len(plans[name])
        print(f"{name:5s} {n_run:3d} of {W} windows: {med[name]:9.2f} [{min(rounds[name]):.2f} .. {max(rounds[name]):.2f}]  "
              f"({med[name] / med['full']:.3f} of the full call; |Wset| / W = {n_run / W:.3f})  | prepare {t['prepare_ms']:.2f} ms, "
              f"windows {t['total_ms']:.2f} ms ({t['total_ms'] / n_run:.3f} per window), {t['n_step_launches']} steps, graph replayed for "
              f"{t['graph_replayed']} of {t['n_segments']} windows, step path {t['step_path']}", flush=True)
    print(f"# {clocks.take()}")
    clocks.on = False


if __name__ == "__main__":
    main()
