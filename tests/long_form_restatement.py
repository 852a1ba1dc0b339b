"""Long-form synthesis restated on the CPU oracles: oracle.rag_oracle.sample_loop (and SagDecoderOracle) chained window by window,
origin_x rebuilt from the previous window's last n_pre_seq poses, the timeline stitched as long_form.sample_long stitches it.  Shared
by tests/test_long_form_host.py (against fixture G22), tests/test_gpu_long_form.py and tests/golden/make_golden_long.py."""
import numpy as np

from livelyspeaker_amd import long_form, synth
from oracle import rag_oracle as orc

B, W = 2, 3
#: name -> (diffusion_steps, respacing, ddim?, skip_timesteps, SAG chain?)
CASES = {"ddim100_skip95": (1000, "ddim100", True, 95, False), "ddpm6": (6, "", False, 0, False),
         "sag_ddim100_skip95": (1000, "ddim100", True, 95, True)}


def inputs(cfg, case):
    """(y, tapes [one synth.NoiseTape per window], text features [B, W, 512] or None) of a G22 case."""
    steps, resp, _, skip, sag = CASES[case]
    n_exec = orc.Schedule(steps, resp).num_timesteps - skip
    tapes = [synth.NoiseTape(cfg, B, n_exec, seed=synth.SEED_NOISE + 10 + w) for w in range(W)]
    text = synth.make_text_features(B * W).reshape(B, W, 512) if sag else None
    return synth.make_long_cond(cfg, B, W), tapes, text


def window_cond(cfg, y, w, prefix):
    """model_kwargs['y'] of window w: its audio, origin_x = [prefix poses | zeros], the per-clip keys, the window's emotion id."""
    origin_x = np.zeros((prefix.shape[0], cfg.njoints, cfg.nfeats, cfg.nframes), np.float32)
    origin_x[..., :cfg.n_pre_seq] = prefix
    yy = {"audio_input": np.ascontiguousarray(long_form.window_audio(y["audio"], w, cfg)), "origin_x": origin_x,
          "vid_indices": y["vid_indices"], "scale": y["scale"]}
    if "emo" in y:
        yy["emo"] = np.repeat(y["emo"][:, w:w + 1], cfg.nframes, axis=1)
    return yy


def stitch(cfg, windows):
    return np.concatenate([windows[0]] + [s[..., cfg.n_pre_seq:] for s in windows[1:]], axis=-1)


def chain(cfg, case, one_window):
    """The chain over W windows; one_window(w, yy, tape, init_image or None) -> sample [B, J, F, T].  Returns (timeline, windows)."""
    y, tapes, text = inputs(cfg, case)
    sag = orc.SagDecoderOracle(synth.make_sag_state_dict(cfg), njoints=cfg.njoints, nfeats=cfg.nfeats) if text is not None else None
    prefix, wins = y["seed_poses"], []
    for w in range(W):
        yy = window_cond(cfg, y, w, prefix)
        init = sag.decode(yy["origin_x"], text[:, w], np.ones((B, cfg.nframes), bool)) if sag is not None else None
        s = np.ascontiguousarray(one_window(w, yy, tapes[w], init), dtype=np.float32)
        wins.append(s)
        prefix = s[..., cfg.nframes - cfg.n_pre_seq:]
    return stitch(cfg, wins), wins


def oracle_chain(cfg, case):
    steps, resp, ddim, skip, _ = CASES[case]
    oracle = orc.RagOracle(synth.make_state_dict(cfg), cfg.njoints, cfg.nfeats, cfg.n_prefix_tokens)
    sch = orc.Schedule(steps, resp)
    return chain(cfg, case, lambda w, yy, tape, init: orc.sample_loop(oracle, sch, yy, tape.x_init, tape.eps, tape.noise, ddim=ddim,
                                                                      skip_timesteps=skip, init_image=init))
