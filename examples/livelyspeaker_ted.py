#!/usr/bin/env python3
"""End-to-end LivelySpeaker inference on one MI355X with the drop-in modules, mirroring
scripts/test_LivelySpeaker_ted.py:57-113 + :176-224 of the reference on SYNTHETIC inputs (no dataset / checkpoints here):

    CLIP text feature z (stand-in)  ->  SAG decoder (script-guided motion)  ->  init_image
    RAG + classifier-free guidance, ddim100, skip_timesteps=80 (20 refinement steps conditioned on audio / speaker / prefix poses)
    ->  post-processing (aligned motions, poses, motion beats)  ->  FGD / diversity against the "real" clips, and the
        beat-consistency score against the onsets detected in the clips' audio on the device

    python examples/livelyspeaker_ted.py [batch]
    python examples/livelyspeaker_ted.py [batch] --from-motion [--raw-poses]
    python examples/livelyspeaker_ted.py [batch] --long-seconds N
    python examples/livelyspeaker_ted.py --long-seconds A,B,... [--drop-finished]
    python examples/livelyspeaker_ted.py [batch] --long-seconds N --edit-frames LO,HI [--edit-joints J0,J1,...] [--edit-text [--clip-text]]
    python examples/livelyspeaker_ted.py --long-seconds 20,45.5,8 --edit-frames LO,HI [--edit-clip K] [...]
    python examples/livelyspeaker_ted.py [batch] --long-seconds N --edit-frames "LO,HI;LO,HI" [--edit-pin N[,N]] [--edit-joints ...] [--edit-clip K]
    python examples/livelyspeaker_ted.py [batch] --long-seconds N --stream-chunk SECONDS [--post [--score]] [--input-sr RATE]
    python examples/livelyspeaker_ted.py [batch] --long-seconds N --score-talk
    python examples/livelyspeaker_ted.py --pool SPEAKERS [--keyed] [--pin 60,95]
    python examples/livelyspeaker_ted.py [batch] --clip-text
--clip-text starts from TOKENS instead of a stand-in feature: synthetic clip.tokenize output -> CLIPTextEncoder (the text tower of CLIP
on the GPU, synthetic weights) -> text features -> SAG decoder -> the same refinement, with no host wait between the two engines.
--from-motion edits a RECORDED clip instead: no text feature is needed, the SAG encoder turns the clip into the CLIP-aligned latent
(recorded clip -> SAG(batch) = MOTIONCLIP.forward -> init_image -> the same 20-step refinement).  With --raw-poses the clip starts as a
RAW recording: joint positions at 25 fps and a waveform go through livelyspeaker_amd.ingest.ted_ingest (resampling to 15 fps, bone
directions, the motion filter's verdicts, 34-frame windows and their 36 267 audio samples, all on the device) and its windows are the
recorded clips and the audio condition.
--long-seconds N synthesises N seconds of gesture for N seconds of speech in ONE call (livelyspeaker_amd.long_form.sample_long): the
34-frame windows are chained on the device, each conditioned on the last four poses of the one before it, the SAG decoder's output for
the window's text feature as its init_image, and stitched into one timeline, which long_form.score_timeline then turns into poses,
motion beats and the beat-consistency score against the speech it was generated from (up to 131 s: the onset detector's 4096 frames).
--long-seconds A,B,... (a comma list) is a RAGGED batch: one speech per entry, each of its own duration, synthesised and scored in one
call each (sample_long(audio_lengths=) -> (timeline, frames) -> score_timeline(frames=, audio_lengths=)); it prints every clip's
frames and beats and the batch's beat-consistency score.  With --drop-finished a speech leaves the batch once its own audio has ended
(sample_long(drop_finished=True)): window w runs only the speeches that still have audio, and the line printed first says how many
clip-windows that saves.
--edit-frames LO,HI (with --long-seconds N) then EDITS the timeline it has just made: the frames [LO, HI) -- with --edit-joints only
the listed joints (0..8) -- are re-synthesised from the existing motion (long_form.edit_long: the inpainting branch on the windows the
range touches, 20 refinement steps each), everything else is kept bit for bit, and the line printed says how many of the W windows ran.
--edit-text makes that edit SCRIPT-GUIDED (edit_long(sag=, text_features=)): the edited frames start from the SAG decoder's output for
one text feature [B, 512] -- a synthetic stand-in, or with --clip-text a sentence of synthetic tokens through CLIPTextEncoder -- and the
kept ones from the existing motion; it prints how far the edited frames moved from the unscripted edit with the same seed.
--edit-frames "LO,HI;LO,HI;..." edits SEVERAL stretches in one call and --edit-pin N[,N...] pins keyframes inside them (those frames
are kept and the motion is re-synthesised around them): both through edit_long(mask=), where "editable" is a mask over the timeline's
elements instead of one rectangle per clip (--edit-text is not wired to this form).
--edit-clip K edits clip K of the batch alone, and --edit-frames after a comma list of durations edits the RAGGED batch (every clip on
the part of [LO, HI) that lies inside its own frames): both through the compact form (edit_long(compact=True / audio_lengths=)), which
runs only the clip-windows the edit touches; the line printed lists them.
--stream-chunk SECONDS (with --long-seconds N) feeds the same waveform to a STREAM instead, SECONDS of audio at a time
(long_form.open_stream: push() returns a window's new frames as soon as the window's audio is complete, close() the zero-padded rest);
it prints when each window's frames appeared and checks that the frames, concatenated, are bit for bit the timeline of the one call.
--input-sr RATE (with --stream-chunk) makes the speech a RATE Hz int16 stereo signal, as a microphone delivers it: the one call samples
audio_io.resample(signal, RATE), the stream is opened with input_sr=RATE, input_channels=2 and fed the int16 chunks themselves;
--post (with --stream-chunk) lets the stream own a post-processing stream (open_stream(post='ted')): every push also returns the new
frames' joint positions and the motion beats that have just become decidable, and it prints the pose shape and the beat times per push.
--score (with --post) lets it own a score stream as well (open_stream(post='ted', score=True, max_seconds=N)): the audio of every push and
the beats of the post stream go in, and the close prints the beat-consistency score, which is the one call's BC bit for bit.
--score-talk (with --long-seconds N) scores the timeline with long_form.score_talk, which has no limit of 4096 frames: --long-seconds 900
--score-talk makes and scores a quarter of an hour (without it, the scoring of the one call stops at 131 s of audio).
--pool SPEAKERS serves that many LIVE speakers from one engine (long_form.open_pool): they start 1.3 s apart and talk for different
times, each joins a slot when it starts and leaves it when its speech ends, audio arrives for all of them every half second, and every
push runs the windows that are complete -- of whichever speakers -- as one batch.  It prints who joined, which batch ran, and who left.
--pin 60,95 (with --pool) opens the pool with pins=128 and pins two poses of the speaker who talks longest at those frames of its
series (long_form.LongPool.pin); the windows that own them run through the inpainting branch, and the distance of the returned frames
from the pinned poses is printed at the end.
--keyed (with --pool, philox) opens the pool with noise_keys='clip': speaker s draws at key 100 + s whatever runs beside it.  After
serving the staggered speakers it runs one of them again, alone, in a fresh keyed pool under the same seed and key, and prints the
max-abs difference between the two runs of that speaker (0 where both ran the same kernel family at the same batch; a kernel family's
distance otherwise).
With real data: load RAG.pt / SAG.pth / the auto-encoder checkpoint with load_model_wo_clip / load_state_dict and build `cond`
exactly as the reference script does; everything below the weight loading is unchanged.
"""
import os
import sys
import time
from types import SimpleNamespace

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from livelyspeaker_amd import synth                                                   # noqa: E402
from livelyspeaker_amd.cfg_sampler import ClassifierFreeSampleModel                   # noqa: E402
from livelyspeaker_amd.model_util import create_model_and_diffusion, load_model_wo_clip   # noqa: E402
from livelyspeaker_amd.motionclip import get_SAG                                      # noqa: E402
from livelyspeaker_amd.motionclip_module import Decoder_TRANSFORMER                   # noqa: E402
from livelyspeaker_amd.postprocess import BeatConsistency, ted_postprocess            # noqa: E402
from livelyspeaker_amd.ted_evaluator import EmbeddingSpaceEvaluator                   # noqa: E402


def build(device="cuda:0"):
    cfg = synth.TED
    args = SimpleNamespace(mdm_condm="text", latent_dim=512, ff_size=1024, layers=8, cond_mask_prob=0.1, arch="trans_enc",
                           emb_trans_dec=False, dataset="humanml", lang_model=None, mlpact="silu", diffusion_steps=1000,
                           noise_schedule="cosine", sigma_small=True, lambda_vel=1.0, lambda_rcxyz=0.0, lambda_fc=0.0, njoints=9)
    model, diffusion = create_model_and_diffusion(args, 'ddim100')                          # test_LivelySpeaker_ted.py:190
    load_model_wo_clip(model, {k: torch.from_numpy(v) for k, v in synth.make_state_dict(cfg).items()})
    model = ClassifierFreeSampleModel(model).to(device)
    model.eval()
    sag_decoder = Decoder_TRANSFORMER(latent_dim=512, n_pre_poses=4, use_style=False)       # motionclip.py:90-91
    sag_decoder.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_sag_state_dict(cfg).items()}, strict=False)
    sag_decoder.to(device)
    sag_decoder.eval()
    evaluator = EmbeddingSpaceEvaluator(ckpt={"pose_dim": 27, "gen_dict": {k: torch.from_numpy(v) for k, v in
                                                                           synth.make_embedding_net_state_dict(27, 32).items()}},
                                        device=device)
    return cfg, model, diffusion, sag_decoder, evaluator


def build_sag(device="cuda:0"):
    """The whole SAG model, loaded the way SAG.pth is loaded (encoder.* / decoder.* keys): motionclip.py:86-92."""
    sag, _ = get_SAG(SimpleNamespace(n_pre_poses=4, use_style=False))          # second item: the CLIP text encoder in the reference
    sag.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_sag_checkpoint(synth.TED).items()}, strict=False)
    sag.to(device)
    sag.eval()
    return sag


def make_inputs(cfg, B, device="cuda:0", guidance_param=2.5, seed=0):
    """What the reference's data loader + CLIP text encoder hand to the loop body (:63-100), on the device (`seed`: which loader batch)."""
    y = synth.make_cond(cfg, B, scale=guidance_param, seed=synth.SEED_COND + seed)
    vec_seq = torch.from_numpy(y["origin_x"]).to(device)                                    # [B,9,3,34] "ground truth" clip
    batch = {"x": vec_seq.clone(), "mask": torch.ones(B, 34, device=device).bool(),
             "z": torch.from_numpy(synth.make_text_features(B, seed=synth.SEED_COND + 2000 + seed)).to(device)}                 # clip_model.encode_text(...) stand-in
    cond = {"y": {"mask": torch.ones(B, 34, device=device).bool(), "audio_input": torch.from_numpy(y["audio_input"]).to(device),
                  "vid_indices": torch.from_numpy(y["vid_indices"]).to(device), "origin_x": vec_seq.clone(),
                  "scale": torch.ones(B, device=device) * guidance_param}}
    return vec_seq, batch, cond


def infer(model, diffusion, sag_decoder, batch, cond, skip_steps=80, seed=233, noise_source="torch_cpu"):
    """SAG decode -> guided refinement (:88-113).  noise_source 'torch_cpu' replays the reference's CPU random stream draw by
    draw (slow: ~1.3 s of host RNG at B=512); 'torch_device' replays the reference's random stream of a GPU run, generated on the
    device inside the loop; 'philox' generates the noise inside the step kernel."""
    diffusion.noise_source = noise_source
    B = batch["x"].shape[0]
    if hasattr(model, "prefetch_condition"):          # optional: the refinement's once-per-call stage overlaps the SAG decode
        model.prefetch_condition(cond["y"] if "y" in cond else cond)
    decoded_motions = sag_decoder(batch)["output"]
    torch.manual_seed(seed)
    sample = diffusion.ddim_sample_loop(model, (B, 9, 3, 34), clip_denoised=False, model_kwargs=cond, skip_timesteps=skip_steps,
                                        init_image=decoded_motions, progress=False, dump_steps=None, noise=None, const_noise=False)
    return decoded_motions, sample


def infer_from_motion(model, diffusion, sag, batch, cond, skip_steps=80, seed=233, noise_source="philox"):
    """Recorded clip -> SAG(batch) (encode to mu, z = mu, decode) -> guided refinement: batch needs 'x' and 'mask' only."""
    diffusion.noise_source = noise_source
    B = batch["x"].shape[0]
    if hasattr(model, "prefetch_condition"):
        model.prefetch_condition(cond["y"] if "y" in cond else cond)
    decoded_motions = sag(batch)["output_xyz"]
    torch.manual_seed(seed)
    sample = diffusion.ddim_sample_loop(model, (B, 9, 3, 34), clip_denoised=False, model_kwargs=cond, skip_timesteps=skip_steps,
                                        init_image=decoded_motions, progress=False, dump_steps=None, noise=None, const_noise=False)
    return decoded_motions, sample


def infer_pipelined(models, diffusion, sag_decoder, batches, conds, skip_steps=80, seed=233):
    """The reference's loader loop (test_LivelySpeaker_ted.py:57-113) over SEVERAL batches, pipelined across calls: the SAG decode and
    the refinement's once-per-call stage of batch n + 1 are ENQUEUED -- on the decoder's stream and on the stream of the other of two
    model replicas -- before batch n's refinement loop is waited for, so they run inside that loop's launch tails and the host never
    stands between two batches.  Results are bitwise those of `infer` called batch by batch with the same seed
    (tests/test_gpu_pipeline.py).  `models`: two CFG-wrapped RAG replicas with the same weights (a handle holds ONE prepared batch)."""
    from livelyspeaker_amd import _lib
    diffusion.noise_source = "philox"
    dev = next(models[0].parameters()).device
    torch_stream = torch.cuda.current_stream(dev).cuda_stream
    sag_stream = sag_decoder.engine()._stream

    def stage(n):
        models[n % 2].prefetch_condition(conds[n]["y"])
        return sag_decoder(batches[n], wait=False)["output"]

    torch.manual_seed(seed)
    decoded = stage(0)
    outs = []
    for n in range(len(batches)):
        _lib.stream_order(dev.index or 0, sag_stream, torch_stream)     # consumers of decode n (this stream, then the engine's) wait for it
        nxt = stage(n + 1) if n + 1 < len(batches) else None            # ... but not for decode n + 1, enqueued behind that point
        B = batches[n]["x"].shape[0]
        outs.append((decoded, diffusion.ddim_sample_loop(models[n % 2], (B, 9, 3, 34), clip_denoised=False, model_kwargs=conds[n],
                                                          skip_timesteps=skip_steps, init_image=decoded, progress=False, dump_steps=None,
                                                          noise=None, const_noise=False)))
        decoded = nxt
    return outs


def main():
    noise_source = "philox"
    if "--noise-source" in sys.argv:                                                        # philox | torch_device | torch_cpu
        i = sys.argv.index("--noise-source")
        noise_source = sys.argv[i + 1]
        del sys.argv[i:i + 2]
    if "--pool" in sys.argv:
        i = sys.argv.index("--pool")
        speakers = int(sys.argv[i + 1])
        if speakers < 1:
            raise SystemExit("--pool takes the number of speakers, >= 1")
        pin = None
        if "--pin" in sys.argv:                                                             # --pin 60,95: frames of the last speaker to pin
            pin = sorted({int(v) for v in sys.argv[sys.argv.index("--pin") + 1].split(",")})
            if not pin or pin[0] < 0 or pin[-1] >= 128:
                raise SystemExit("--pin takes frames in [0, 128), comma-separated")
        return main_pool(speakers, noise_source, keyed="--keyed" in sys.argv, pin=pin)
    if "--long-seconds" in sys.argv:
        i = sys.argv.index("--long-seconds")
        arg = sys.argv[i + 1]
        del sys.argv[i:i + 2]
        edit = None
        if "--edit-frames" in sys.argv:
            j = sys.argv.index("--edit-frames")
            stretches = [tuple(int(v) for v in part.split(",")) for part in sys.argv[j + 1].split(";") if part]
            if not stretches or any(len(st) != 2 for st in stretches):
                raise SystemExit("--edit-frames takes LO,HI or several stretches LO,HI;LO,HI;... (quote the semicolons)")
            edit = {"frames": stretches[0], "stretches": stretches}
            del sys.argv[j:j + 2]
            if len(edit["frames"]) != 2:
                raise SystemExit("--edit-frames takes LO,HI")
        if "--edit-joints" in sys.argv:
            j = sys.argv.index("--edit-joints")
            if edit is None:
                raise SystemExit("--edit-joints goes with --edit-frames")
            edit["joints"] = [int(v) for v in sys.argv[j + 1].split(",") if v]
            del sys.argv[j:j + 2]
        if "--edit-pin" in sys.argv:
            j = sys.argv.index("--edit-pin")
            if edit is None:
                raise SystemExit("--edit-pin goes with --edit-frames")
            edit["pins"] = [int(v) for v in sys.argv[j + 1].split(",") if v]
            del sys.argv[j:j + 2]
        if "--edit-clip" in sys.argv:
            j = sys.argv.index("--edit-clip")
            if edit is None:
                raise SystemExit("--edit-clip goes with --edit-frames")
            edit["clip"] = int(sys.argv[j + 1])
            del sys.argv[j:j + 2]
        if "--edit-text" in sys.argv:
            sys.argv.remove("--edit-text")
            if edit is None:
                raise SystemExit("--edit-text goes with --edit-frames")
            edit["text"] = "clip" if "--clip-text" in sys.argv else "synthetic"
            if edit["text"] == "clip":
                sys.argv.remove("--clip-text")
        stream_chunk = None
        if "--stream-chunk" in sys.argv:
            j = sys.argv.index("--stream-chunk")
            stream_chunk = float(sys.argv[j + 1])
            del sys.argv[j:j + 2]
            if stream_chunk <= 0:
                raise SystemExit("--stream-chunk takes a positive number of seconds")
        input_sr = None
        if "--input-sr" in sys.argv:
            j = sys.argv.index("--input-sr")
            input_sr = int(sys.argv[j + 1])
            del sys.argv[j:j + 2]
            if stream_chunk is None or input_sr < 1:
                raise SystemExit("--input-sr takes a rate in Hz and goes with --stream-chunk: the stream is fed at that rate")
        post = "--post" in sys.argv
        if post:
            sys.argv.remove("--post")
            if stream_chunk is None:
                raise SystemExit("--post goes with --stream-chunk: the stream's frames are post-processed as they arrive")
        score = "--score" in sys.argv
        if score:
            sys.argv.remove("--score")
            if not post:
                raise SystemExit("--score goes with --stream-chunk --post: it scores the beats of the post-processing stream")
        score_talk = "--score-talk" in sys.argv
        if score_talk:
            sys.argv.remove("--score-talk")
        drop = "--drop-finished" in sys.argv
        if drop:
            sys.argv.remove("--drop-finished")
        if stream_chunk is not None and ("," in arg or drop or edit is not None):
            raise SystemExit("--stream-chunk streams the waveform of --long-seconds N (one duration, no edit)")
        if "," in arg:
            return main_long_ragged([float(v) for v in arg.split(",") if v], noise_source, drop, edit)
        if drop:
            raise SystemExit("--drop-finished goes with a comma list of durations: equally long speeches finish together")
        seconds = float(arg)
        return main_long(int(sys.argv[1]) if len(sys.argv) > 1 else 1, seconds, noise_source, edit, stream_chunk, post, score, score_talk, input_sr)
    if "--clip-text" in sys.argv:
        sys.argv.remove("--clip-text")
        return main_clip_text(int(sys.argv[1]) if len(sys.argv) > 1 else 64, noise_source)
    from_motion = "--from-motion" in sys.argv
    if from_motion:
        sys.argv.remove("--from-motion")
    raw_poses = "--raw-poses" in sys.argv
    if raw_poses:
        sys.argv.remove("--raw-poses")
        if not from_motion:
            raise SystemExit("--raw-poses goes with --from-motion: it is the recorded clip that is ingested")
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 64
    if from_motion:
        return main_from_motion(B, noise_source, raw_poses)
    if len(sys.argv) > 2:                                                                   # python examples/livelyspeaker_ted.py B N: N batches, pipelined
        return main_pipelined(B, int(sys.argv[2]))
    cfg, model, diffusion, sag_decoder, evaluator = build()
    vec_seq, batch, cond = make_inputs(cfg, B)
    infer(model, diffusion, sag_decoder, batch, cond, noise_source=noise_source)            # warm-up (graph capture, allocations)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    decoded, sample = infer(model, diffusion, sag_decoder, batch, cond, noise_source=noise_source)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    post = ted_postprocess(sample)                                                          # test_RAG_ted.py:84-111
    real = vec_seq.permute(0, 3, 1, 2).reshape(B, 34, -1)
    for i in range(0, B, 64):
        evaluator.push_samples(post["aligned_motions"][i:i + 64], real[i:i + 64])
    fgd, feat_dist = evaluator.get_scores() if B > 32 else (float("nan"), float("nan"))
    n_beats = sum(len(b) for b in post["motion_beat_times"])
    bc = BeatConsistency()                                                                  # test_RAG_ted.py:112-127
    bc.push(post["motion_beat_times"], audio=cond["y"]["audio_input"], sr=16000)           # onset_detect(y, sr=16000, units='time') per clip, on the device
    beat_score = bc.score() if bc.num_beats else float("nan")
    print(f"B={B} ({noise_source}): SAG decode + 20-step guided refinement {dt * 1e3:.1f} ms ({B * 34 / dt:.0f} pose-frames/s); "
          f"motion beats {n_beats}, audio onsets {bc.num_beats}, BC {beat_score:.4f}; FGD {fgd:.4f}, feature distance {feat_dist:.4f} "
          f"(synthetic weights and audio: numbers are not quality)")
    assert bool(torch.isfinite(sample).all())


def raw_recordings(B, device="cuda:0", seconds=6.0, raw_fps=25):
    """Synthetic RAW recordings, as a motion-capture file and its sound track hold them: joint positions [n, 10, 3] at 25 fps (the
    mean pose with swinging arms) and a 16 kHz waveform each, enough of them for B windows; and ingest.ted_ingest's arguments for them."""
    import numpy as np
    from livelyspeaker_amd.postprocess import TED_DIR_VEC_PAIRS, TED_MEAN_DIR_VEC
    mean_pose = np.zeros((10, 3))
    for j, (parent, child, length) in enumerate(TED_DIR_VEC_PAIRS):
        mean_pose[child] = mean_pose[parent] + length * TED_MEAN_DIR_VEC[3 * j:3 * j + 3]
    n = int(seconds * raw_fps)
    per_recording = (int(seconds * 15) - 42) // 10 + 1                                      # windows of 42 resampled frames, stride 10
    rng = np.random.Generator(np.random.PCG64(synth.SEED_COND + 6000))
    skeletons, audio = [], []
    for _ in range(-(-B // per_recording)):
        t = np.linspace(0.0, seconds, n)[:, None, None]
        pose = np.repeat(mean_pose[None], n, 0)
        pose[:, 4:] += 0.1 * np.sin(2 * np.pi * rng.uniform(0.4, 1.0, (1, 6, 3)) * t + rng.uniform(0, 2 * np.pi, (1, 6, 3)))
        skeletons.append(torch.from_numpy(pose.astype(np.float32)).to(device))
        audio.append(torch.from_numpy((0.1 * rng.standard_normal(int(seconds * 16000))).astype(np.float32)).to(device))
    return skeletons, audio, [0.0] * len(skeletons), [seconds] * len(skeletons), mean_pose.astype(np.float32), TED_MEAN_DIR_VEC


def main_from_motion(B, noise_source, raw_poses=False):
    cfg, model, diffusion, _, _ = build()
    sag = build_sag()
    vec_seq, batch, cond = make_inputs(cfg, B)
    if raw_poses:                                                                           # the recorded clip comes from RAW poses and audio
        from livelyspeaker_amd.ingest import VERDICTS, ted_ingest
        got = ted_ingest(*raw_recordings(B), disable_filtering=True)                        # resample 25 -> 15 fps, directions, windows, audio: on the device
        verdicts = got["verdict"].cpu().numpy()
        print(f"ingest: {len(verdicts)} windows from {int(got['clip'].max()) + 1} raw recordings at 25 fps; verdicts "
              + ", ".join(f"{VERDICTS[v]} {int((verdicts == v).sum())}" for v in sorted(set(verdicts.tolist()))))
        batch["x"] = got["x"][:B].contiguous()
        cond["y"]["origin_x"] = batch["x"].clone()
        cond["y"]["audio_input"] = got["audio"][:B].contiguous()
        assert batch["x"].shape == vec_seq.shape and cond["y"]["audio_input"].shape == (B, 36267)
    lengths = torch.full((B,), 34, device=vec_seq.device)
    lengths[1::2] = 28                                                                      # every other recording is shorter
    batch = {"x": batch["x"], "mask": sag.lengths_to_mask(lengths)}                         # no text feature: z comes from the encoder
    infer_from_motion(model, diffusion, sag, dict(batch), cond, noise_source=noise_source)  # warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    decoded, sample = infer_from_motion(model, diffusion, sag, batch, cond, noise_source=noise_source)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    print(f"B={B} ({noise_source}), from motion: SAG encode + decode + 20-step guided refinement {dt * 1e3:.1f} ms; encode "
          f"{sag.encoder.engine().last_encode_ms():.3f} ms, decode {sag.decoder.engine().last_decode_ms():.3f} ms; "
          f"|mu| mean {float(batch['mu'].norm(dim=-1).mean()):.3f}")
    assert bool(torch.isfinite(sample).all()) and bool((decoded[1, :, :, 28:] == 0).all())


def main_clip_text(B, noise_source):
    """Tokens -> text features -> SAG decode -> refinement.  The encode is enqueued only (wait=False) and the decoder's stream is ordered
    behind the encoder's, so the features never pass through the host."""
    import numpy as np
    from livelyspeaker_amd import _lib
    from livelyspeaker_amd.motionclip import get_clip
    cfg, model, diffusion, sag_decoder, _ = build()
    clip_model = get_clip({k: torch.from_numpy(v) for k, v in synth.synth_clip_text_state().items()}, "cuda:0")
    vec_seq, batch, cond = make_inputs(cfg, B)
    lengths = [int(n) for n in np.random.Generator(np.random.PCG64(13)).integers(6, 25, B)]     # a sentence inside a 2.3 s clip: about a dozen tokens
    text = torch.from_numpy(synth.synth_clip_tokens(lengths))                                   # what clip.tokenize returns: host int64 [B, 77]

    def run():
        batch["z"] = clip_model.encode_text(text, wait=False)
        _lib.stream_order(0, clip_model.engine()._stream, sag_decoder.engine()._stream)
        return infer(model, diffusion, sag_decoder, batch, cond, noise_source=noise_source)

    run()                                                                                   # warm-up (graph capture, allocations)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    decoded, sample = run()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    print(f"B={B} ({noise_source}), from tokens: CLIP text encode + SAG decode + 20-step guided refinement {dt * 1e3:.1f} ms; encode "
          f"{clip_model.engine().last_encode_ms():.3f} ms for {sum(lengths)} of {77 * B} rows, decode {sag_decoder.engine().last_decode_ms():.3f} ms; "
          f"|z| mean {float(batch['z'].norm(dim=-1).mean()):.3f}")
    assert bool(torch.isfinite(sample).all()) and bool(torch.isfinite(decoded).all())


def main_long(B, seconds, noise_source, edit=None, stream_chunk=None, post=False, score=False, score_talk=False, input_sr=None):
    """`seconds` of 16 kHz speech per clip -> one stitched timeline at 15 fps (the LivelySpeaker chain, window after window on the device)."""
    import numpy as np
    from livelyspeaker_amd import long_form
    cfg, model, diffusion, sag_decoder, _ = build()
    diffusion.noise_source = noise_source
    g = np.random.Generator(np.random.PCG64(synth.SEED_COND))
    audio = torch.from_numpy(0.1 * g.standard_normal((B, max(1, int(round(seconds * 16000))))).astype(np.float32)).cuda()
    mic = None
    if input_sr is not None:                                                                # a microphone's signal: int16 stereo at input_sr
        from livelyspeaker_amd import audio_io
        mic = torch.from_numpy((3000 * g.standard_normal((B, max(1, int(round(seconds * input_sr))), 2))).astype(np.int16)).cuda()
        audio, _ = audio_io.resample(mic, input_sr)                                         # what the one call below samples
        print(f"{input_sr} Hz int16 stereo {tuple(mic.shape)} -> 16 kHz mono {tuple(audio.shape)} on the device")
    W, _, n_frames = long_form.plan_windows(audio.shape[1], cfg)
    y = {k: torch.from_numpy(v).cuda() for k, v in synth.make_long_cond(cfg, B, W, scale=2.5).items()}
    text = torch.from_numpy(synth.make_text_features(B * W).reshape(B, W, 512)).cuda()          # one text feature per window
    run = lambda: long_form.sample_long(diffusion, model, audio, y["seed_poses"], y["vid_indices"], y["scale"], sampler="ddim",      # noqa: E731
                                        skip_timesteps=80, sag=sag_decoder, text_features=text)
    torch.manual_seed(233)
    run()                                                                                   # warm-up (graph capture, allocations)
    torch.cuda.synchronize()
    torch.manual_seed(233)
    t0 = time.perf_counter()
    timeline = run()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    assert timeline.shape == (B, 9, 3, n_frames) and bool(torch.isfinite(timeline).all())
    print(f"B={B} ({noise_source}): {seconds:g} s of speech -> {W} chained windows, {n_frames} frames ({n_frames / 15:.1f} s of gesture) in "
          f"{dt * 1e3:.1f} ms ({B * n_frames / dt:.0f} pose-frames/s)")
    # the timeline as one series per clip: joint positions, motion beats and the beat-consistency score against the speech, on the device
    scored = long_form.score_talk(timeline, audio) if score_talk else long_form.score_timeline(timeline, audio)
    n_beats = sum(len(b) for b in scored["motion_beat_times"])
    print(f"pose {tuple(scored['pose'].shape)}, motion beats {n_beats}, BC {scored['bc']:.4f} (synthetic weights and audio: numbers are "
          f"not quality)" + (f"; score_talk: {int(scored['onset_count'].sum())} audio onsets in {audio.shape[1] // 512 + 1} audio frames" if score_talk else ""))
    assert tuple(scored["pose"].shape) == (B, n_frames, 10, 3) and bool(torch.isfinite(scored["pose"]).all())
    if edit is not None:
        edit_timeline(long_form, cfg, model, diffusion, timeline, audio, y, W, edit, sag_decoder)
    if stream_chunk is not None:
        stream_timeline(long_form, model, diffusion, sag_decoder, timeline, audio, y, text, stream_chunk, scored if post else None, score, mic, input_sr)


def stream_timeline(long_form, model, diffusion, sag_decoder, timeline, audio, y, text, chunk_seconds, scored=None, score=False, mic=None,
                    input_sr=None):
    """The waveform main_long sampled in one call, fed to a stream `chunk_seconds` at a time: every push carries the text feature of the
    window it would start (a held value), and a window's frames come back from the push that completed its audio.  `scored` (the
    timeline's post-processing, --post): the stream post-processes its frames as they arrive, and the pushes' poses and beats,
    concatenated, are checked against it.  `mic` (--input-sr): the stream is fed that signal at `input_sr` instead, through its own resampler."""
    rate, fed = (16000, audio) if mic is None else (input_sr, mic)
    n, L, W = max(1, int(round(chunk_seconds * rate))), fed.shape[1], text.shape[1]
    torch.manual_seed(233)                                                                  # the seed of the one call: the same draws
    stream = long_form.open_stream(diffusion, model, y["seed_poses"], y["vid_indices"], y["scale"], sampler="ddim", skip_timesteps=80,
                                   sag=sag_decoder, post=None if scored is None else "ted",
                                   **({"score": True, "max_seconds": L / rate + 1} if score else {}),
                                   **({} if mic is None else {"input_sr": input_sr, "input_channels": 2}))
    parts, poses, beats, t0 = [], [], [[] for _ in range(audio.shape[0])], time.perf_counter()
    for lo in list(range(0, L, n)) + [None]:
        held = {"text_features": text[:, min(stream.windows_run, W - 1)]}
        t1 = time.perf_counter()
        new = stream.close(**held) if lo is None else stream.push(fed[:, lo:lo + n], **held)
        torch.cuda.synchronize()
        if scored is not None:
            new, posted = new
            poses.append(posted["pose"])
            for b, times in enumerate(posted["motion_beat_times"]):
                beats[b] += times
            if new.shape[3] or any(posted["motion_beat_times"]):
                print(f"  post: pose {tuple(posted['pose'].shape)}, beats decided (clip 0, seconds): "
                      + (", ".join(f"{t:.2f}" for t in posted["motion_beat_times"][0]) or "none"))
        if new.shape[3]:
            print(f"  {'close' if lo is None else f'audio {min(lo + n, L) / rate:6.2f} s'}: window {stream.windows_run - 1} -> frames "
                  f"{stream.frames_out - new.shape[3]}..{stream.frames_out - 1}, {(time.perf_counter() - t1) * 1e3:.1f} ms after its last sample "
                  f"arrived ({(time.perf_counter() - t0) * 1e3:.0f} ms into the stream)")
        parts.append(new)
    streamed = torch.cat(parts, dim=3)
    assert torch.equal(streamed, timeline), float((streamed - timeline).abs().max())
    print(f"streamed in {chunk_seconds:g} s chunks ({len(parts) - 1} pushes + close): {stream.windows_run} windows, {stream.frames_out} frames, "
          f"bit for bit the timeline of the one call")
    if scored is not None:
        assert torch.equal(torch.cat(poses, dim=1), scored["pose"]) and beats == scored["motion_beat_times"]
        print(f"post-processed as they arrived: {sum(len(b) for b in beats)} motion beats, poses and beats bit for bit those of the whole timeline")
    if score:
        result = posted["score"]                                                            # the close finished every clip's series
        assert result["bc"] == scored["bc"] or (result["bc"] != result["bc"] and scored["bc"] != scored["bc"])
        print(f"scored at the close: {sum(r['count'] for r in result['slots'].values())} audio onsets, BC {result['bc']:.4f}, bit for bit the "
              f"one call's")


def main_pool(speakers, noise_source, tick_seconds=0.5, keyed=False, pin=None):
    """`speakers` live speakers on ONE engine (long_form.open_pool): speaker s starts talking 1.3 s after speaker s - 1 and talks for
    6 + s seconds; audio arrives for all of them every `tick_seconds`.  A speaker joins a free slot when it starts and leaves when its
    speech ends; every tick is one push, which runs the windows that are complete as one batch.  `pin` (--pin 60,95): the pool is
    opened with pins=128 and the last speaker -- the one who talks longest -- is told, when it joins, which pose to be in at those
    frames; at the end the distance of its returned frames from those poses is printed."""
    import numpy as np
    from livelyspeaker_amd import long_form
    if noise_source == "torch_device":
        raise SystemExit("--pool draws with philox or torch_cpu")
    if keyed and noise_source != "philox":
        raise SystemExit("--keyed keys philox draws")
    cfg, model, diffusion, _, _ = build()
    diffusion.noise_source = noise_source
    if keyed:
        diffusion.philox_seed = 0x5EED_2026             # one seed for the session and for its replay
    opts = {"noise_keys": "clip"} if keyed else {}
    if pin:
        opts["pins"] = 128                              # the horizon: a pin may lie up to 128 frames ahead of the frames returned
        pinned = speakers - 1
        poses = (torch.rand(cfg.njoints, cfg.nfeats, len(pin), generator=torch.Generator().manual_seed(95)) * 2 - 1).cuda()
    n = int(round(tick_seconds * 16000))
    start = [int(round(1.3 * s / tick_seconds)) for s in range(speakers)]                       # the tick a speaker joins in
    length = [int(round((6 + s) * 16000)) for s in range(speakers)]
    y = {k: torch.from_numpy(v).cuda() for k, v in synth.make_long_cond(cfg, speakers, max(length) // 32000 + 2, scale=2.5).items()}
    torch.manual_seed(233)
    pool = long_form.open_pool(diffusion, model, speakers, sampler="ddim", skip_timesteps=80, **opts)
    slot, fed, frames = {}, [0] * speakers, [0] * speakers
    kept = [[] for _ in range(speakers)]
    t0, tick = time.perf_counter(), 0
    while any(fed[s] < length[s] for s in range(speakers)):
        for s in range(speakers):
            if start[s] == tick:
                slot[s] = pool.join(y["seed_poses"][s], y["vid_indices"][s], y["scale"][s], **({"key": 100 + s} if keyed else {}))
                print(f"tick {tick:3d}: speaker {s} joins slot {slot[s]}" + (f" under key {100 + s}" if keyed else ""))
                if pin and s == pinned:
                    pool.pin(slot[s], pin, poses)
                    print(f"tick {tick:3d}: speaker {s} is pinned at frames {pin}: {int(pool.slots['pins'][slot[s]])} pinned frames to come")
        chunk, lengths = torch.zeros(speakers, n, device="cuda"), np.zeros(speakers, np.int64)
        for s, k in slot.items():
            take = min(n, length[s] - fed[s])
            chunk[k, :take] = y["audio"][s, fed[s]:fed[s] + take]
            lengths[k], fed[s] = take, fed[s] + take
        t1 = time.perf_counter()
        new, counts = pool.push(chunk, lengths)
        torch.cuda.synchronize()
        done = {s: int(counts[k]) for s, k in slot.items() if counts[k]}
        if done:
            print(f"tick {tick:3d}: one batch of {len(done)} -> " + ", ".join(f"speaker {s} +{c} frames" for s, c in done.items()) +
                  f" in {(time.perf_counter() - t1) * 1e3:.1f} ms")
        for s, c in done.items():
            frames[s] += c
            kept[s].append(new[slot[s], :, :, :c])
        for s in [s for s in slot if fed[s] == length[s]]:
            tail = pool.leave(slot.pop(s))
            frames[s] += int(tail.shape[2])
            kept[s].append(tail)
            assert frames[s] == long_form.plan_windows(length[s], cfg)[2] and bool(torch.isfinite(tail).all())
            print(f"tick {tick:3d}: speaker {s} leaves after {length[s] / 16000:g} s of speech with {frames[s]} frames")
        tick += 1
    pool.close()
    print(f"{speakers} speakers, {sum(frames)} frames ({noise_source}) in {(time.perf_counter() - t0) * 1e3:.0f} ms over {tick} pushes on one engine")
    if pin:
        served = torch.cat(kept[pinned], dim=2)
        for k, f in enumerate(pin):
            if f < served.shape[2]:
                print(f"speaker {pinned}, frame {f}: max |returned - pinned pose| = {float((served[:, :, f] - poses[:, :, k]).abs().max()):.3e}")
            else:
                print(f"speaker {pinned}, frame {f}: never reached ({served.shape[2]} frames); the pin was dropped when the speaker left")
    if keyed:           # the session replayed for one speaker: alone, in one chunk, in slot 0 of a fresh pool -- same seed, same key
        s = speakers // 2
        solo = long_form.open_pool(diffusion, model, 1, sampler="ddim", skip_timesteps=80, noise_keys="clip")
        solo.join(y["seed_poses"][s], y["vid_indices"][s], y["scale"][s], key=100 + s)
        head, _ = solo.push(y["audio"][s:s + 1, :length[s]].contiguous(), [length[s]])
        again = torch.cat([head[0], solo.leave(0)], dim=2)
        served = torch.cat(kept[s], dim=2)
        assert again.shape == served.shape
        print(f"speaker {s} (key {100 + s}) run again alone in a fresh keyed pool: max |served - replayed| = {float((served - again).abs().max()):.3e} "
              f"over {served.shape[2]} frames")


def edit_timeline(long_form, cfg, model, diffusion, timeline, audio, y, W, edit, sag_decoder=None, lengths=None, frames=None):
    """Re-synthesise the frames [lo, hi) of the timeline main_long made (on the listed joints, or all): only the windows that own a
    frame of the range are sampled, starting from the existing motion -- and with edit['text'] from the SAG decoder's output for one
    script on the edited elements.  edit['clip'] edits that clip of the batch alone, and lengths / frames (main_long_ragged) edit a
    ragged batch, every clip inside its own frames: both through the compact form, which runs only the clip-windows it touches."""
    import numpy as np
    if len(edit.get("stretches", ())) > 1 or edit.get("pins"):
        return edit_timeline_by_mask(long_form, cfg, model, diffusion, timeline, audio, y, W, edit, lengths, frames)
    lo, hi = edit["frames"]
    B = timeline.shape[0]
    joints = None
    if edit.get("joints"):
        joints = np.zeros(cfg.njoints, bool)
        joints[edit["joints"]] = True
    most = np.full(B, timeline.shape[3]) if frames is None else np.asarray(frames)
    ranges = np.stack([np.minimum(lo, most), np.minimum(hi, most)], axis=1).astype(np.int64)
    if edit.get("clip") is not None:
        if not 0 <= edit["clip"] < B:
            raise SystemExit(f"--edit-clip takes a clip of the batch, 0 .. {B - 1}")
        ranges[np.arange(B) != edit["clip"]] = 0
    form = dict(compact=True) if edit.get("clip") is not None or lengths is not None else {}
    if lengths is not None:
        form["audio_lengths"] = lengths
    torch.manual_seed(377)
    t0 = time.perf_counter()
    edited, ran, _ = long_form.edit_long(diffusion, model, timeline, ranges, audio, y["seed_poses"], y["vid_indices"], y["scale"],
                                         joints=joints, sampler="ddim", skip_timesteps=80, return_windows=True, **form)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    kept = torch.ones_like(timeline, dtype=torch.bool)
    for b, (lo_b, hi_b) in enumerate(ranges):
        kept[b, :, :, lo_b:hi_b] = False if joints is None else torch.from_numpy(~joints).to(kept.device)[:, None, None]
    assert torch.equal(edited[kept], timeline[kept]) and bool(torch.isfinite(edited).all())
    changed = int((edited != timeline).sum())
    what = f"{len(ran)} of {W} windows ran ({ran})"
    if form:            # the compact form returns its plan: (w, rows)
        what = f"{sum(len(rows) for _, rows in ran)} clip-windows of {B * W} ran ({', '.join(f'window {w}: clips {rows}' for w, rows in ran)})"
    print(f"edit of frames [{lo}, {hi}){'' if joints is None else ' on joints ' + str(edit['joints'])}"
          f"{'' if edit.get('clip') is None else ' of clip ' + str(edit['clip'])}: {what} in {dt * 1e3:.1f} ms; {changed} of {timeline.numel()} "
          f"values changed, every other one kept bit for bit")
    if not edit.get("text"):
        return
    if edit["text"] == "clip":                  # a sentence as clip.tokenize returns it (synthetic tokens) -> CLIPTextEncoder on the GPU
        from livelyspeaker_amd.motionclip import get_clip
        clip_model = get_clip({k: torch.from_numpy(v) for k, v in synth.synth_clip_text_state().items()}, "cuda:0")
        z = clip_model.encode_text(torch.from_numpy(synth.synth_clip_tokens([12] * B))).float()
    else:
        z = torch.from_numpy(synth.make_text_features(B, seed=synth.SEED_COND + 3000)).cuda()
    torch.manual_seed(377)                      # the seed of the unscripted edit: the same draws
    t0 = time.perf_counter()
    scripted = long_form.edit_long(diffusion, model, timeline, ranges, audio, y["seed_poses"], y["vid_indices"], y["scale"], joints=joints,
                                   sampler="ddim", skip_timesteps=80, sag=sag_decoder, text_features=z, **form)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    assert torch.equal(scripted[kept], timeline[kept]) and bool(torch.isfinite(scripted).all())
    moved = (scripted - edited)[~kept].abs()
    print(f"the same edit guided by one script ({edit['text']} text feature): {dt * 1e3:.1f} ms; the edited values moved by "
          f"{float(moved.mean()):.4f} on average (max {float(moved.max()):.4f}) from the unscripted edit with the same seed")


def edit_timeline_by_mask(long_form, cfg, model, diffusion, timeline, audio, y, W, edit, lengths=None, frames=None):
    """Several stretches in ONE call, with keyframes pinned inside them: edit_long(mask=), True = editable.  The mask holds every
    stretch of --edit-frames (on the listed joints, or all; on edit['clip'] alone, or on every clip inside its own frames) except the
    frames of --edit-pin, which are kept -- the motion is re-synthesised around those poses and passes through them."""
    import numpy as np
    B, N = timeline.shape[0], timeline.shape[3]
    joints = None
    if edit.get("joints"):
        joints = np.zeros(cfg.njoints, bool)
        joints[edit["joints"]] = True
    pins = edit.get("pins", [])
    one = long_form.keyframe_mask(N, pins, cfg, within=edit["stretches"])[0]            # [J, F, N]: the stretches without the pinned frames
    if joints is not None:
        one &= joints[:, None, None]
    mask = np.broadcast_to(one, (B,) + one.shape).copy()
    if edit.get("clip") is not None:
        if not 0 <= edit["clip"] < B:
            raise SystemExit(f"--edit-clip takes a clip of the batch, 0 .. {B - 1}")
        mask[np.arange(B) != edit["clip"]] = False
    for b in range(B if frames is not None else 0):                                    # a ragged batch: every clip inside its own frames
        mask[b, :, :, int(frames[b]):] = False
    form = dict(compact=True) if edit.get("clip") is not None or lengths is not None else {}
    if lengths is not None:
        form["audio_lengths"] = lengths
    torch.manual_seed(377)
    t0 = time.perf_counter()
    edited, ran, _ = long_form.edit_long(diffusion, model, timeline, None, audio, y["seed_poses"], y["vid_indices"], y["scale"], sampler="ddim",
                                         skip_timesteps=80, return_windows=True, mask=mask, **form)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    kept = ~torch.from_numpy(mask).to(timeline.device)
    assert torch.equal(edited[kept], timeline[kept]) and bool(torch.isfinite(edited).all())
    what = f"{len(ran)} of {W} windows ran ({ran})"
    if form:            # the compact form returns its plan: (w, rows)
        what = f"{sum(len(rows) for _, rows in ran)} clip-windows of {B * W} ran ({', '.join(f'window {w}: clips {rows}' for w, rows in ran)})"
    print(f"one edit of the stretches {edit['stretches']}{'' if not pins else ' around the pinned frames ' + str(pins)}"
          f"{'' if joints is None else ' on joints ' + str(edit['joints'])}{'' if edit.get('clip') is None else ' of clip ' + str(edit['clip'])}: "
          f"{what} in {dt * 1e3:.1f} ms; {int((edited != timeline).sum())} of {timeline.numel()} values changed, every other one -- the pinned "
          f"frames included -- kept bit for bit")


def main_long_ragged(seconds, noise_source, drop_finished=False, edit=None):
    """One speech per entry of `seconds`, each of its own length, through one sample_long call and one score_timeline call."""
    import numpy as np
    from livelyspeaker_amd import long_form
    cfg, model, diffusion, sag_decoder, _ = build()
    diffusion.noise_source = noise_source
    B = len(seconds)
    lengths = [max(1, int(round(s * 16000))) for s in seconds]
    plans = long_form.plan_lengths(lengths, cfg)
    W = max(w for w, _ in plans)
    g = np.random.Generator(np.random.PCG64(synth.SEED_COND))
    audio = torch.from_numpy(0.1 * g.standard_normal((B, max(lengths))).astype(np.float32)).cuda()       # rows padded to the longest speech
    y = {k: torch.from_numpy(v).cuda() for k, v in synth.make_long_cond(cfg, B, W, scale=2.5).items()}
    text = torch.from_numpy(synth.make_text_features(B * W).reshape(B, W, 512)).cuda()
    torch.manual_seed(233)
    timeline, frames = long_form.sample_long(diffusion, model, audio, y["seed_poses"], y["vid_indices"], y["scale"], sampler="ddim",
                                             skip_timesteps=80, sag=sag_decoder, text_features=text, audio_lengths=lengths,
                                             drop_finished=drop_finished)
    assert frames.tolist() == [f for _, f in plans] and bool(torch.isfinite(timeline).all())
    scored = long_form.score_timeline(timeline, audio, frames=frames, audio_lengths=lengths)
    print(f"B={B} ({noise_source}): {W} chained windows for the longest speech, timeline {tuple(timeline.shape)}")
    if drop_finished:
        active = long_form.plan_drop(lengths, cfg)[2]
        print(f"  finished speeches dropped: clips per window {active.tolist()}, {int(active.sum())} clip-windows sampled instead of {B * W}")
    for b in range(B):
        print(f"  clip {b}: {seconds[b]:g} s of speech -> {plans[b][0]} windows, {int(frames[b])} frames, "
              f"{len(scored['motion_beat_times'][b])} motion beats")
    print(f"BC {scored['bc']:.4f} over the batch (synthetic weights and audio: numbers are not quality)")
    assert all(not bool(scored["pose"][b, int(frames[b]):].any()) for b in range(B))
    if edit is not None:
        edit_timeline(long_form, cfg, model, diffusion, timeline, audio, y, W, edit, sag_decoder, lengths, frames)


def main_pipelined(B, N):
    cfg, model, diffusion, sag_decoder, _ = build()
    _, model2, _, _, _ = build()
    ins = [make_inputs(cfg, B, seed=n) for n in range(N)]
    batches, conds = [i[1] for i in ins], [i[2] for i in ins]
    infer_pipelined([model, model2], diffusion, sag_decoder, batches[:2], conds[:2])        # warm-up: both replicas capture their graphs
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    outs = infer_pipelined([model, model2], diffusion, sag_decoder, batches, conds)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / N
    print(f"B={B} x {N} batches, pipelined across calls: {dt * 1e3:.2f} ms per batch ({B * 34 / dt:.0f} pose-frames/s)")
    assert all(bool(torch.isfinite(o).all()) for _, o in outs)


if __name__ == "__main__":
    main()
