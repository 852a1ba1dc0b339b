"""Long-form synthesis: 34-frame windows chained on the device into one stitched timeline.

The RAG denoiser is built to be continued: ``origin_x[..., :n_pre_seq]`` (RAG.py:110-112), the indicator bit ``InputProcess`` appends
and the SAG decoder's ``n_pre_poses`` exist so that the last four poses of one clip condition the next.  ``sample_long`` runs that
chain as ONE engine call (``ls_long_prepare`` + ``ls_long_sample``):

* window ``w`` reads ``audio[:, w * AUDIO_STRIDE : w * AUDIO_STRIDE + audio_len]`` (32000 samples = 30 frames at 15 fps of 16 kHz
  audio); the whole waveform goes through the WavEncoder once, in chunks of ``encoder_chunk`` clip-windows;
* window 0 is conditioned on ``seed_poses``, window ``w >= 1`` on ``sample_{w-1}[..., T - n_pre : T]``; the hand-off
  (``k_chain_window``, csrc/ls_chain.hip) happens on the device, the host neither copies nor waits between windows;
* window 0 contributes its 34 frames to the timeline, every later window its frames ``n_pre..33``.

With ``noise_source='torch_cpu'`` the draws are those ``GaussianDiffusion._loop`` makes for one call, window after window
(``ref_draws.RefDraws.windows``), and the result is bit for bit what the same windows give through ``ddim_sample_loop`` /
``p_sample_loop`` (and ``Decoder_TRANSFORMER.forward`` with ``sag``) called once per window with ``origin_x`` rebuilt in between
(tests/test_gpu_long_form.py).  ``'philox'`` draws one key per call; the window index is folded into the Philox counter (csrc/ls_philox.h).

Clips of different lengths (``audio_lengths=``) run the longest clip's windows; with ``drop_finished=True`` a clip leaves the batch once
its own audio has ended (``plan_drop``; ``ls_long_prepare_ragged``), and window ``w`` is a sampling call on the clips that remain.

A finished timeline is corrected with ``edit_long``: a frame range per clip (optionally some joints only) is re-synthesised by the
windows that own one of its frames (``edit_plan``), each through the sampling loop's inpainting branch with the window's slice of the
timeline as the given motion (``edit_window``; ``ls_long_edit``, ``k_edit_gather`` / ``k_edit_scatter``); everything else is kept bit
for bit.  With ``sag=`` / ``text_features=`` the edit is script-guided: every window that runs starts from the SAG decoder's output on
its editable elements (``edit_start``; ``ls_long_edit_sag``, ``k_edit_start``).  ``edit_long(compact=True)`` runs only the
clip-windows the edit touches (``edit_plan_compact``; ``ls_long_prepare_edit`` + ``ls_long_edit_compact``): window w is a sampling call
on the clips that have an editable element in it, and only those clip-windows of audio are encoded; ``audio_lengths=`` edits the
timeline of a ragged ``sample_long`` call that way.  ``edit_long(mask=)`` takes "editable" as a bool mask over the timeline's elements
(True = editable) in place of the rectangle: several stretches, pinned keyframes (``keyframe_mask``), joints per stretch, constrained
generation; the same windows' body, kernels and captured loop (``ls_long_edit_mask`` & co.; ``k_edit_mask_pairs`` plans a device mask).

``open_stream`` is the online form of the same chain: audio arrives in chunks of any size, a window runs as soon as its last sample
is there, and the frames of all pushes are bit for bit ``sample_long``'s for the concatenated audio (``ls_long_stream_open`` /
``ls_long_stream_push``; the session pool's engine with every slot fed alike).

``open_pool`` is a pool of such streams on one engine: clips join and leave slot by slot and are fed at their own rates, and a push
runs the windows that are complete in rounds, each one sampling call on the slots that have one (``pool_plan``; ``ls_long_pool_*``,
``k_pool_gather`` / ``k_pool_scatter``).
"""
from __future__ import annotations

import numpy as np
import torch as th

from . import _lib, audio_io, postprocess, ref_draws
from . import gaussian_diffusion as gd

AUDIO_STRIDE = 32000        # audio samples between two windows: T - n_pre_seq = 30 frames at 15 fps of 16 kHz audio
_UNSUPPORTED = ("const_noise", "dump_steps", "inpainting_mask", "inpainted_motion")


def plan_windows(n_audio_samples, cfg):
    """(W, padded_len, n_frames) for a waveform of ``n_audio_samples`` samples: the windows that cover it, the length it is zero-padded
    to, the frames of the stitched timeline.  ``cfg``: anything with audio_len / nframes / n_pre_seq (synth.PathConfig, RAG)."""
    L, AL = int(n_audio_samples), int(cfg.audio_len)
    if L < 1:
        raise ValueError(f"the waveform holds no sample ({L})")
    W = max(1, -(-(L - AL) // AUDIO_STRIDE) + 1)
    return (W,) + _window_sizes(W, cfg)


def plan_lengths(audio_lengths, cfg):
    """Per clip of a ragged batch: ``(W_b, frames_b)`` -- the windows that cover ``audio_lengths[b]`` samples and the frames of that
    clip's stitched timeline, both from ``plan_windows``."""
    plans = [plan_windows(int(n), cfg) for n in np.asarray(audio_lengths).reshape(-1)]
    return [(W, frames) for W, _, frames in plans]


def plan_drop(audio_lengths, cfg):
    """The batch plan of ``sample_long(audio_lengths=, drop_finished=True)``, from the lengths alone (no GPU):
    ``(order, windows, active, offsets)``, numpy int arrays.

    * ``order`` [B]: slot -> clip.  The clips are held in slots, stably sorted by their window count ``W_b`` (``plan_lengths``),
      longest first; clips with the same count keep the caller's order.
    * ``windows`` [B]: ``W_b`` of the clip in each slot (non-increasing).
    * ``active`` [W_max]: ``B_w``, the clips that run window ``w`` -- those with ``W_b > w``, which are the slots ``[0, B_w)``.
      ``active[0] == B``.
    * ``offsets`` [W_max + 1]: running sums of ``active``; window ``w`` owns the entries ``offsets[w] .. offsets[w + 1]`` of everything
      that is packed window after window (the noise tapes; ``offsets[-1]`` clip-windows in all, against ``B * W_max``).

    One definition for the engine and for this module (``ls_long_plan_drop``)."""
    lens = np.asarray(audio_lengths).reshape(-1)
    order, windows, active = _lib.long_plan_drop(lens, int(cfg.audio_len))
    offsets = np.zeros(active.size + 1, np.int64)
    np.cumsum(active, out=offsets[1:])
    return order.astype(np.int64), windows.astype(np.int64), active.astype(np.int64), offsets


def _window_sizes(W, cfg):
    T, npre = int(cfg.nframes), int(cfg.n_pre_seq)
    return int(cfg.audio_len) + (W - 1) * AUDIO_STRIDE, T + (W - 1) * (T - npre)


def window_audio(audio, w, cfg):
    """The ``[B, audio_len]`` waveform window ``w`` reads, zero-padded at the end where ``audio`` [B, L] runs out."""
    AL, lo = int(cfg.audio_len), int(w) * AUDIO_STRIDE
    if w < 0:
        raise ValueError(f"window index {w}")
    piece = audio[:, lo:lo + AL]
    short = AL - int(piece.shape[1])
    if short <= 0:
        return piece
    if isinstance(audio, np.ndarray):
        return np.concatenate([piece, np.zeros((audio.shape[0], short), audio.dtype)], axis=1)
    return th.cat([piece, piece.new_zeros((audio.shape[0], short))], dim=1)


def _shape(a):
    return tuple(int(s) for s in a.shape)


def _check_args(diffusion, model, audio, seed_poses, vid_indices, scale, emo, n_windows, sampler, skip_timesteps, sag, text_features,
                encoder_chunk, unsupported):
    """Everything that can be refused without an engine (no GPU is touched)."""
    from .cfg_sampler import ClassifierFreeSampleModel
    for k, v in unsupported.items():
        if k not in _UNSUPPORTED:
            raise TypeError(f"sample_long() got an unexpected keyword argument {k!r}")
        if v is not None and v is not False:
            raise NotImplementedError(f"sample_long: {k} is not built for chained windows")
    if not isinstance(model, ClassifierFreeSampleModel):
        raise TypeError(f"sample_long: pass livelyspeaker_amd.ClassifierFreeSampleModel(RAG), got {type(model).__name__}")
    if diffusion.noise_source == "torch_device":
        raise NotImplementedError("sample_long: noise_source='torch_device' is not built for chained windows; use 'torch_cpu' or 'philox'")
    diffusion._check_noise_source()
    if getattr(diffusion, "row_keys", None) is not None:
        raise NotImplementedError("sample_long: diffusion.row_keys key the rows of p_sample_loop / ddim_sample_loop; chained windows draw at "
                                  "sample_offset + b + (w << 48), and a pool's clips at their own keys (open_pool(noise_keys='clip'))")
    if sampler not in ("ddim", "ddpm"):
        raise ValueError(f"sampler must be 'ddim' or 'ddpm', got {sampler!r}")
    rag = model.model
    if rag.nframes != 34:
        raise NotImplementedError("sample_long chains the reference's 34-frame windows")
    if audio.ndim != 2:
        raise ValueError(f"audio must be [B, L], got {list(audio.shape)}")
    B, L = _shape(audio)
    if B < 1 or L < 1:
        raise ValueError(f"audio must be [B, L] with B, L >= 1, got {[B, L]}")
    W = plan_windows(L, rag)[0] if n_windows is None else int(n_windows)
    if W < 1:
        raise ValueError(f"n_windows must be >= 1, got {n_windows}")
    if seed_poses.ndim != 4 or _shape(seed_poses) != (B, rag.njoints, rag.nfeats, rag.n_pre_seq):
        raise ValueError(f"seed_poses must be {[B, rag.njoints, rag.nfeats, rag.n_pre_seq]}, got {list(seed_poses.shape)}")
    if vid_indices.ndim != 1 or _shape(vid_indices) != (B,):
        raise ValueError(f"vid_indices must be [{B}], got {list(vid_indices.shape)}")
    if scale.ndim != 1 or _shape(scale) != (B,):
        raise ValueError(f"scale must be [{B}], got {list(scale.shape)}")
    if rag.n_prefix_tokens == 2:
        if emo is None:
            raise ValueError("the BEAT model needs emo: [B] (one id per clip) or [B, W] (one per window)")
        if emo.ndim not in (1, 2) or _shape(emo) not in ((B,), (B, W)):
            raise ValueError(f"emo must be [{B}] or [{B}, {W}], got {list(emo.shape)}")
    elif emo is not None:
        raise ValueError("emo is a BEAT conditioning; the TED model takes none")
    if text_features is not None and sag is None:
        raise ValueError("text_features without sag: the SAG decoder turns them into every window's init_image")
    if sag is not None:
        if text_features is None:
            raise ValueError("sag needs text_features [B, W, 512]")
        if text_features.ndim != 3 or _shape(text_features) != (B, W, rag.latent_dim):
            raise ValueError(f"text_features must be {[B, W, rag.latent_dim]}, got {list(text_features.shape)}")
        if (sag.njoints, sag.nfeats, sag.num_frames, sag.n_pre_poses) != (rag.njoints, rag.nfeats, rag.nframes, rag.n_pre_seq):
            raise ValueError("the SAG decoder's (njoints, nfeats, num_frames, n_pre_poses) do not match the RAG model's")
    if not 0 <= int(skip_timesteps) < diffusion.num_timesteps:
        raise ValueError(f"skip_timesteps {skip_timesteps} outside [0, {diffusion.num_timesteps})")
    if encoder_chunk is not None and int(encoder_chunk) < 1:
        raise ValueError(f"encoder_chunk must be >= 1, got {encoder_chunk}")
    return B, W


def _as_tensors(*arrays):
    return tuple(a if (a is None or th.is_tensor(a)) else th.as_tensor(np.asarray(a)) for a in arrays)


def _check_model(diffusion, rag):
    """What the engine's loop is built for, refused behind ``_check_args``."""
    if diffusion.model_mean_type != gd.ModelMeanType.START_X or diffusion.model_var_type != gd.ModelVarType.FIXED_SMALL:
        raise NotImplementedError("only START_X + FIXED_SMALL (create_gaussian_diffusion's setting) is built")
    if rag.cond_mask_prob <= 0:
        raise ValueError("ClassifierFreeSampleModel returns None when cond_mask_prob == 0 (cfg_sampler.py:24-31)")


def _bind_engine(diffusion, rag):
    """The model's engine with the diffusion's schedule; its resident conditioning is the caller's from here on."""
    eng = diffusion._bind_schedule(rag.engine())
    rag._cond_key = rag._prefetched_key = None
    return eng


def _emo_windows(emo, W, B):
    """``emo`` [B] or [B, W] (or None) in the engine's [W, B] layout."""
    if emo is None:
        return None
    return (emo[None, :].expand(W, B) if emo.ndim == 1 else emo.t()).contiguous()


def _loop_kw(diffusion, sampler, skip_timesteps, eta, clip_denoised):
    """The sampler arguments every chained-window engine call takes."""
    return dict(sampler=_lib.LS_SAMPLER_DDIM if sampler == "ddim" else _lib.LS_SAMPLER_DDPM, skip_timesteps=int(skip_timesteps),
                eta=float(eta) if sampler == "ddim" else 0.0, use_graph=diffusion.use_graph, clip_denoised=clip_denoised,
                two_pass_always=diffusion.two_pass_always)


def _check_tape_bound(diffusion, who, n_exec, shape, D, renoised=False):
    """``noise_source='torch_cpu'``: one window's tape (with the re-noise plane of an edit when ``renoised``) must fit tape_segment_bytes."""
    per_window = n_exec * (2 * shape[0] * D + (2 if renoised else 1) * int(np.prod(shape))) * 4
    if per_window > diffusion.tape_segment_bytes:
        raise ValueError(f"{who}: one window's noise tape is {per_window} bytes, tape_segment_bytes is "
                         f"{diffusion.tape_segment_bytes}; segmented tapes are not built for chained windows (raise "
                         "tape_segment_bytes or use noise_source='philox')")


def sample_long(diffusion, model, audio, seed_poses, vid_indices, scale, emo=None, n_windows=None, sampler='ddim', skip_timesteps=0,
                eta=0.0, clip_denoised=False, sag=None, text_features=None, encoder_chunk=None, return_windows=False, audio_lengths=None,
                drop_finished=False, **unsupported):
    """``n_windows`` chained windows for ``audio`` [B, L] (default: the windows that cover it, ``plan_windows``) as one timeline
    ``[B, J, F, T + (W - 1) * (T - n_pre)]`` on the inputs' device; ``return_windows=True`` adds the raw windows ``[W, B, J, F, T]``.

    ``seed_poses`` [B, J, F, n_pre] condition window 0; ``vid_indices`` [B] and ``scale`` [B] hold for all windows; ``emo`` (BEAT) is
    [B] or [B, W].  ``sampler``: 'ddim' (``eta``) or 'ddpm'; ``skip_timesteps`` as in the sample loops.  ``sag`` (a
    ``Decoder_TRANSFORMER``) with ``text_features`` [B, W, 512] is the LivelySpeaker chain: window w starts from
    ``sag({'x': origin_x_w, 'z': text_features[:, w], 'mask': ones})['output']`` as its ``init_image``.  The noise source is the
    diffusion object's (``'torch_cpu'`` or ``'philox'``); ``const_noise``, ``dump_steps`` and the inpainting inputs are refused.

    ``audio_lengths`` (a host sequence [B], each in [1, L]): speeches of different lengths in one call.  ``audio[b, audio_lengths[b]:]``
    counts as silence (a zero-filled copy is sampled from; the caller's tensor is not modified), the call runs the windows of the
    longest clip (``W_max`` of ``plan_lengths``; ``emo`` [B, W] and ``text_features`` [B, W, 512] are sized by it), clip b's timeline
    is zero beyond its own ``frames_b``, and the result is ``(timeline, frames)`` -- ``(timeline, frames, windows)`` with
    ``return_windows`` -- with ``frames`` the host int32 [B] that ``score_timeline(frames=, audio_lengths=)`` takes.  Together with
    ``n_windows`` it raises ``ValueError``.  Every clip runs all ``W_max`` windows unless ``drop_finished`` is set.

    ``drop_finished=True`` (needs ``audio_lengths``): a clip runs only its own ``W_b`` windows.  The clips are held longest-first
    (``plan_drop``) and window w is a sampling call on the ``B_w`` clips that still have audio, at that batch: its own kernel plan,
    and the single-pass shortcut when the scales of THOSE clips are all 1.  Inputs, shapes and the return value are those of
    ``audio_lengths`` alone, in the caller's clip order; the raw windows are zero for ``w >= W_b``; entries of ``emo`` and
    ``text_features`` for windows a clip does not run are ignored, and so is ``audio`` beyond a clip's length (it is never read: no
    zero-filled copy is made).  The noise contract:

    * ``'torch_cpu'``: the draws are those of one public sampling call per window at batch ``B_w`` on the active clips in slot
      order, window after window (``RefDraws.windows(batches=)``), and the result is bit for bit that loop's
      (tests/test_gpu_long_drop.py).  The one-window tape bound (``tape_segment_bytes``) is checked for window 0, the largest.
    * ``'philox'``: the clip in slot s draws, in window w, the streams of global sample index ``sample_offset + s + (w << 48)``: the
      streams follow the slot, not the caller's row.  A batch that is already longest-first gets exactly the draws of the same call
      without ``drop_finished`` (and, where no kernel choice differs between the batch sizes, its bits on every clip's valid
      range); any other order gets the draws of the call on the slot-ordered batch.
    * ``'torch_device'`` stays refused.

    Not built: device-resident length arrays."""
    if audio_lengths is not None and n_windows is not None:
        raise ValueError("sample_long: audio_lengths decide the windows of every clip; pass either n_windows or audio_lengths")
    if drop_finished and audio_lengths is None:
        raise ValueError("sample_long: drop_finished drops a clip when its audio_lengths entry is used up; pass audio_lengths")
    audio, seed_poses, vid_indices, scale, emo, text_features = _as_tensors(audio, seed_poses, vid_indices, scale, emo, text_features)
    frames = None
    if audio_lengths is not None and hasattr(model, "model"):      # another model type is _check_args's to refuse
        if audio.ndim != 2:
            raise ValueError(f"audio must be [B, L], got {list(audio.shape)}")
        lens = _lib.host_lengths(audio_lengths, int(audio.shape[0]), 1, int(audio.shape[1]), "audio_lengths")
        plans = plan_lengths(lens, model.model)
        n_windows = max(W for W, _ in plans)
        frames = np.array([f for _, f in plans], np.int32)
        if not drop_finished:
            valid = th.arange(int(audio.shape[1]))[None, :] < th.from_numpy(lens.astype(np.int64))[:, None]
            audio = th.where(valid.to(audio.device), audio, th.zeros((), dtype=audio.dtype, device=audio.device))       # a copy; NaN tails become 0
    B, W = _check_args(diffusion, model, audio, seed_poses, vid_indices, scale, emo, n_windows, sampler, skip_timesteps, sag, text_features,
                       encoder_chunk, unsupported)
    rag = model.model
    _check_model(diffusion, rag)
    out_dev = audio.device
    eng = _bind_engine(diffusion, rag)
    emo = _emo_windows(emo, W, B)
    batches = None
    if drop_finished:       # the engine reads audio and seed poses through its slot table; the B- and W*B-row inputs are put in slot order here
        order, _, active, _ = plan_drop(lens, rag)
        batches = [int(n) for n in active]
        slot = lambda a, dim: a.index_select(dim, th.from_numpy(order).to(a.device))      # noqa: E731
        vid_indices, scale = slot(vid_indices, 0), slot(scale, 0)
        emo = None if emo is None else slot(emo, 1).contiguous()
        text_features = None if text_features is None else slot(text_features, 0)
    eng.long_prepare(audio.float(), seed_poses.float(), vid_indices, scale.float(), emo=emo, n_windows=W, encoder_chunk=encoder_chunk,
                     audio_lengths=lens if drop_finished else None)
    n_exec = diffusion.num_timesteps - int(skip_timesteps)
    shape = (B, rag.njoints, rag.nfeats, rag.nframes)
    kw = dict(_loop_kw(diffusion, sampler, skip_timesteps, eta, clip_denoised), device_out=out_dev.type == "cuda", return_windows=return_windows)
    if sag is not None:
        sag_eng = sag.engine()
        if sag_eng.device != eng.device:
            raise ValueError(f"the SAG decoder runs on cuda:{sag_eng.device}, the RAG model on cuda:{eng.device}")
        kw["sag"] = sag_eng
        kw["text_features"] = text_features.float().permute(1, 0, 2).contiguous()
    if diffusion.noise_source == "philox":
        kw.update(diffusion._philox_key())
    else:
        _check_tape_bound(diffusion, "sample_long", n_exec, shape, eng.D)
        kw["x_init"], kw["eps_tape"], kw["noise_tape"] = ref_draws.RefDraws("cpu").windows(diffusion, W, n_exec, shape, eng.D, batches=batches)
        diffusion.last_tape_segments = 1
    res = eng.long_sample(**kw)
    timeline, windows = res if return_windows else (res, None)
    timeline = gd._as_tensor(timeline, out_dev)
    if drop_finished:       # the engine zero-filled both outputs ahead of window 0
        return (timeline, frames, gd._as_tensor(windows, out_dev)) if return_windows else (timeline, frames)
    if frames is not None:
        keep = th.arange(int(timeline.shape[3]))[None, :] < th.from_numpy(frames.astype(np.int64))[:, None]
        timeline = th.where(keep.to(timeline.device)[:, None, None, :], timeline, th.zeros((), dtype=timeline.dtype, device=timeline.device))
        return (timeline, frames, gd._as_tensor(windows, out_dev)) if return_windows else (timeline, frames)
    return (timeline, gd._as_tensor(windows, out_dev)) if return_windows else timeline


class _Session:
    """What ``LongStream`` and ``LongPool`` share: the ``with`` form, the engine bound at the first engine call (``_open(eng)`` opens the
    session on it), and the refusals of the held conditioning a push passes."""

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self._closed = True        # leaving the block ends the session; the windows a close() would still run are not run
        return False

    def _engine(self):
        if self._eng is None:
            eng = _bind_engine(self._diffusion, self._rag)
            if self._sag is not None and self._sag.engine().device != eng.device:
                raise ValueError(f"the SAG decoder runs on cuda:{self._sag.engine().device}, the RAG model on cuda:{eng.device}")
            self._open(eng)
            self._eng = eng
        return self._eng

    def _init_post(self, post, rag, slots, score=None, max_seconds=None):
        """``post=``: None, or the dataset whose post-processing stream the session owns ('ted' / 'beat', the model's own).  ``score=``:
        None, True or a dict of ``postprocess.open_score_stream``'s options: the session also owns a score stream of as many slots,
        sized for ``max_seconds`` of audio per clip."""
        if post is not None:
            want = "beat" if getattr(rag, "n_prefix_tokens", 1) == 2 else "ted"
            if post != want:
                raise ValueError(f"post must be None or the model's dataset {want!r}, got {post!r}")
        self._post_kind, self._post_slots, self._post, self._score = post, slots, None, None
        if score is not None and score is not False:
            if post is None:
                raise ValueError("score= scores the motion beats of the post-processing stream: pass post= as well")
            if score is not True and not isinstance(score, dict):
                raise ValueError(f"score must be None, True or a dict of open_score_stream's options, got {score!r}")
            if max_seconds is None or not float(max_seconds) > 0:
                raise ValueError(f"score= needs max_seconds > 0 (the audio a clip may hold: the score stream's memory), got {max_seconds!r}")
            # no device yet: the handle is bound, on the engine's device, by the first call that feeds it
            self._score = postprocess.open_score_stream(post, slots, max_seconds, **(score if isinstance(score, dict) else {}))
        elif max_seconds is not None:
            raise ValueError("max_seconds sizes the score stream: pass score=True as well")

    def _init_input(self, input_sr, input_channels, resample, slots):
        """``input_sr=``: None, or the rate of the audio the session is fed: it then owns an ``audio_io.ResampleStream`` of as many slots
        (``input_channels`` interleaved channels, float32 or int16 as the first push has it; ``resample``: a dict of ``zeros``, ``beta``,
        ``rolloff``, ``max_chunk``) whose 16 kHz output is what the windows see.  No device is touched here."""
        self._in = None
        if input_sr is None:
            if input_channels != 1 or resample is not None:
                raise ValueError("input_channels and resample describe the audio of input_sr=: pass input_sr as well")
            return
        opts = dict(resample or {})
        unknown = set(opts) - {"zeros", "beta", "rolloff", "max_chunk"}
        if unknown:
            raise ValueError(f"resample takes zeros, beta, rolloff and max_chunk, got {sorted(unknown)}")
        self._in = audio_io.open_resample_stream(slots, input_sr, audio_io.OUT_SR, channels=input_channels, dtype=None, **opts)

    def _input_plan(self, audio, lengths=None, finish=None):
        """What a chunk at the input rate (or the finish of the slots flagged) will give the windows, ahead of anything that runs:
        ``(out_count [S], feed)``.  The resampler checks the chunk and plans its outputs on the host and is left as it is; ``feed()``
        pushes the chunk through it on the engine's device and returns the 16 kHz samples ``[S, K]`` on the chunk's side.  ``_feed``
        calls it once every refusal of the session has passed, so a refused call leaves session and resampler as they were."""
        count = self._in.check(audio, lengths, finish)[5]
        cuda = self._last_dev.type == "cuda" if audio is None else _lib._is_cuda(audio)

        def feed():
            self._in.device = self._engine().device
            got = self._in.push(audio, lengths, finish, device_out=cuda)
            assert (got["out_count"] == count).all()
            return gd._as_tensor(got["audio"], th.device("cuda", self._in.device) if cuda else th.device("cpu"))

        return count, feed

    def _check_post_frames(self, most):
        """Ahead of the sampling: a push of the post-processing stream takes at most 256 frames per slot."""
        if self._post_kind is not None and most > postprocess.POST_STREAM_MAX_CHUNK:
            raise ValueError(f"with post=, a call may complete at most {postprocess.POST_STREAM_MAX_CHUNK} frames per clip (8 windows), this one "
                             f"would complete {most}: feed the audio in smaller chunks")

    def _post_push(self, frames, counts, finish, audio=None, lengths=None):
        """The session's frames into its post-processing stream (opened on the engine's device at the first call): a device tensor
        goes in as it is, without a host copy.  With ``score=``: the call's ``audio`` and the beats of that push into the score stream,
        and for the slots that ``finish`` the result under ``'score'``."""
        if self._post is None:
            rag = self._rag
            self._post = postprocess.open_post_stream(self._post_kind, self._post_slots, device=self._eng.device, joints=int(rag.njoints))
        res = self._post.push(frames, counts, finish)
        if self._score is not None:
            self._score_push(res, finish, audio, lengths)
        if self._closed:                  # the session's last call has finished every series: the handles go with it
            self._post.close()
            if self._score is not None:
                self._score.close()
        return res

    def _score_push(self, res, finish, audio, lengths):
        sc = self._score
        sc.device = self._eng.device
        if audio is not None and int(audio.shape[1]):
            n = int(audio.shape[1])
            lens = np.full(self._post_slots, n, np.int64) if lengths is None else np.asarray(lengths, np.int64)
            for c0 in range(0, n, sc.max_chunk):      # a push of the score stream takes max_chunk samples per slot
                piece = audio[:, c0:c0 + sc.max_chunk]
                sc.push(audio=piece, lengths=np.clip(lens - c0, 0, int(piece.shape[1])))
        sc.push(beats=res)
        ending = [] if finish is None else [s for s in np.nonzero(np.asarray(finish).reshape(-1))[0] if sc.samples_in[s] > 0]
        if ending:
            res["score"] = score_summary(sc, sc._finish([int(s) for s in ending]))

    def _check_held(self, emo, text_features, rows):
        """``emo`` [rows] (BEAT) and ``text_features`` [rows, latent_dim] (with ``sag=``), each None or one row per clip."""
        rag = self._rag
        if emo is not None:
            if rag.n_prefix_tokens != 2:
                raise ValueError("emo is a BEAT conditioning; the TED model takes none")
            if _shape(emo) != (rows,):
                raise ValueError(f"emo must be [{rows}], got {list(emo.shape)}")
        if text_features is not None:
            if self._sag is None:
                raise ValueError("text_features without sag: the SAG decoder turns them into every window's init_image")
            if _shape(text_features) != (rows, rag.latent_dim):
                raise ValueError(f"text_features must be {[rows, rag.latent_dim]}, got {list(text_features.shape)}")


    # ---- pinned poses for frames the session has yet to make (open_pool(pins=), open_stream(pins=)) ----
    def _init_pins(self, pins, rag, slots):
        """``pins=``: None, or the horizon H -- an int of at least nframes: a pin may name a frame in ``[frames_out, frames_out + H)``.
        ``self._pending[s]``: the pinned frames of slot s whose window has yet to run (the engine holds the same list)."""
        if pins is not None:
            T = int(getattr(rag, "nframes", 34))
            if isinstance(pins, bool) or not isinstance(pins, (int, np.integer)) or not T <= int(pins) <= 1 << 20:
                raise ValueError(f"pins must be None or the horizon in frames, an int in [{T}, 2^20], got {pins!r}")
            pins = int(pins)
        self._pins, self._pending = pins, [set() for _ in range(slots)]

    def _check_pin(self, frames, poses, mask, lead, frames_out):
        """The refusals of ``pin``, ahead of any engine call: ``frames`` [K] distinct host ints in ``[frames_out, frames_out + H)``,
        ``poses`` ``lead + [J, F, K]`` and ``mask`` None or bool of that shape.  Returns (frames int64 [K], poses, mask)."""
        rag = self._rag
        if self._pins is None:
            raise ValueError("pin needs a session opened with pins=H (the horizon in frames)")
        if self._sag is not None:
            raise ValueError("pins with sag= are not built: a pinned window would start from edit_start(motion, mask, sag_out)")
        if hasattr(frames, "detach"):
            frames = frames.detach().cpu().numpy()
        fr = np.asarray(frames)
        if fr.ndim != 1 or fr.size < 1 or fr.dtype.kind not in "iu":
            raise ValueError(f"frames must be a host sequence [K] of ints, K >= 1, got {frames!r}")
        fr = fr.astype(np.int64)
        if len(set(fr.tolist())) != fr.size:
            raise ValueError(f"frames names a frame twice: {fr.tolist()}")
        if fr.min() < frames_out or fr.max() >= frames_out + self._pins:
            raise ValueError(f"frames {fr.tolist()} outside [{frames_out}, {frames_out + self._pins}): a pin names a frame that has not been "
                             f"returned yet (frames_out) and lies within the horizon pins={self._pins}")
        poses, mask = _as_tensors(poses, mask)
        want = tuple(lead) + (rag.njoints, rag.nfeats, int(fr.size))
        if _shape(poses) != want:
            raise ValueError(f"poses must be {list(want)}, got {list(poses.shape)}")
        if mask is not None and (_shape(mask) != want or mask.dtype != th.bool):
            raise ValueError(f"mask must be bool {list(want)} (True = pinned), got {mask.dtype} {list(mask.shape)}")
        return fr, poses.float(), mask

    def _check_unpin(self, frames, frames_out):
        if self._pins is None:
            raise ValueError("unpin needs a session opened with pins=H")
        if frames is None:
            return None
        fr = np.asarray(frames.detach().cpu().numpy() if hasattr(frames, "detach") else frames)
        if fr.ndim != 1 or fr.size < 1 or fr.dtype.kind not in "iu" or len(set(fr.tolist())) != fr.size:
            raise ValueError(f"frames must be None or a host sequence [K] of distinct ints, got {frames!r}")
        if fr.min() < frames_out or fr.max() >= frames_out + self._pins:
            raise ValueError(f"frames {fr.tolist()} outside [{frames_out}, {frames_out + self._pins})")
        return fr.astype(np.int64)

    def _calls(self, rounds, windows_run):
        """The sampling calls of a push that runs ``rounds``: ``pool_pin_plan`` on the pending pins (without pins: the rounds)."""
        if self._pins is None or not any(self._pending):
            return [(r, False, list(slots)) for r, slots in enumerate(rounds)]
        n_windows = [sum(s in r for r in rounds) for s in range(len(self._pending))]
        return pool_pin_plan(windows_run, n_windows, self._pending, self._rag)

    def _consume(self, calls, windows_run, leaving):
        """After a push: the pins of the windows that ran pinned are spent, and a slot that leaves drops the rest."""
        for r, pinned, slots in calls:
            for s in slots if pinned else ():
                lo, hi = _owned(int(windows_run[s]) + r, self._rag)
                self._pending[s] -= {n for n in self._pending[s] if lo <= n < hi}
        for s in leaving:
            self._pending[int(s)].clear()


def _owned(w, cfg):
    """The series frames ``[lo, hi)`` window w owns: all 34 for w = 0, the 30 behind its prefix otherwise (``edit_plan``'s ownership)."""
    T, S = int(cfg.nframes), int(cfg.nframes) - int(cfg.n_pre_seq)
    return (0 if w == 0 else w * S + int(cfg.n_pre_seq)), w * S + T


def pool_pin_plan(windows_run, n_windows, pins, cfg):
    """The sampling calls of one push of a session with pinned poses, from host counts alone (no GPU): a list of ``(round, pinned,
    slots)`` in the order they run.  Slot s runs ``n_windows[s]`` windows in the push (``pool_plan``'s rounds: round r holds the slots
    with ``n_windows[s] > r``), its window ``windows_run[s] + r`` in round r; ``pins[s]`` holds the slot's pending pinned frames (series
    frames, any order).  The slot's row in round r is PINNED iff one of them is a frame that window owns (all 34 frames for window 0,
    ``30 w + 4 .. 30 w + 33`` otherwise).  Round r becomes its unpinned slots, ascending, as one plain call, then its pinned slots,
    ascending, as one inpainting call; an empty half is skipped -- without pins the calls are ``pool_plan``'s rounds.  One definition for
    the engine and for this module (``ls_long_pool_pin_plan``)."""
    return _lib.long_pool_pin_plan(windows_run, n_windows, pins, int(cfg.nframes), int(cfg.n_pre_seq))


def _call_draws(diffusion, rag, calls, n_exec, D):
    """``'torch_cpu'``: what one public sampling call per call of the plan draws, in order (``RefDraws.windows`` for a plain call,
    ``RefDraws.edit_windows`` for a pinned one; the TED tree re-noises the kept motion), packed as the engine reads them: x
    [sum A, J, F, T], flat eps / noise, and the flat re-noise tape of the pinned calls (None without one)."""
    noised = rag.n_prefix_tokens == 1
    xs, eps, nz, inz = [], [], [], []
    for _, pinned, slots in calls:
        shape = (len(slots), rag.njoints, rag.nfeats, rag.nframes)
        if pinned:
            d = ref_draws.RefDraws("cpu").edit_windows(diffusion, 1, n_exec, shape, D, noised)
            if noised:
                inz.append(d[3].reshape(-1))
        else:
            d = ref_draws.RefDraws("cpu").windows(diffusion, 1, n_exec, shape, D)
        xs.append(d[0][0]); eps.append(d[1].reshape(-1)); nz.append(d[2].reshape(-1))
    return th.cat(xs, dim=0), th.cat(eps), th.cat(nz), (th.cat(inz) if inz else None)


def score_summary(stream, finished):
    """What a session reports for the slots a call finished: ``{'slots': {slot: ScoreStream.finish dict}}`` plus, on TED, ``'bc'`` -- the
    beat-consistency score over those slots, accumulated as ``BeatConsistency.push_timeline`` does (nan without an onset) -- and on BEAT
    ``'align'``, the slots' BeatAlign scores in slot order."""
    out = {"slots": finished}
    order = sorted(finished)
    if stream.dataset == "ted":
        acc = postprocess.BeatConsistency(sigma=stream.sigma)
        acc.push_score({s: finished[s] for s in order})
        out["bc"] = acc.score() if acc.num_beats else float("nan")
    else:
        out["align"] = np.array([finished[s]["align"] for s in order], np.float32)
    return out


class LongStream(_Session):
    """A running ``open_stream`` session; see there.  ``samples_in``, ``windows_run``, ``frames_out``: host ints."""

    def __init__(self, diffusion, model, seed_poses, vid_indices, scale, emo, sampler, skip_timesteps, eta, clip_denoised, sag, post=None,
                 score=None, max_seconds=None, input_sr=None, input_channels=1, resample=None, pins=None):
        seed_poses, vid_indices, scale, emo = _as_tensors(seed_poses, vid_indices, scale, emo)
        B = int(seed_poses.shape[0]) if seed_poses.ndim else 0
        rag = getattr(model, "model", None)
        beat = getattr(rag, "n_prefix_tokens", 1) == 2
        # _check_args on a one-window stand-in: a stream has no waveform yet, and its per-window conditioning arrives with the pushes
        _check_args(diffusion, model, th.empty(max(B, 0), 1), seed_poses, vid_indices, scale,
                    emo if (emo is not None or not beat) else th.zeros(B, dtype=th.long), None, sampler, skip_timesteps, sag,
                    None if sag is None else th.empty(B, 1, int(rag.latent_dim)), None, {})
        _check_model(diffusion, rag)
        if emo is not None and emo.ndim != 1:
            raise ValueError(f"a stream holds one emotion id per clip: emo must be [{B}], got {list(emo.shape)}")
        self._diffusion, self._rag, self._sag, self._B = diffusion, rag, sag, B
        self._init_post(post, rag, B, score, max_seconds)
        self._init_input(input_sr, input_channels, resample, B)
        self._init_pins(pins, rag, B)
        self.input_samples_in = 0                       # frames at input_sr; samples_in counts the 16 kHz samples the windows see
        self._cond = (seed_poses.float(), vid_indices, scale.float())
        self._emo, self._text = emo, None               # held on the host side only until the next engine call takes them
        self._have_emo = self._have_text = False
        self._kw = _loop_kw(diffusion, sampler, skip_timesteps, eta, clip_denoised)
        if diffusion.noise_source == "philox":          # one key per stream: window w draws at sample_offset + b + (w << 48)
            self._kw.update(diffusion._philox_key())
        self._n_exec = diffusion.num_timesteps - int(skip_timesteps)
        self._eng = None
        self._closed = False
        self._last_dev = th.device("cpu")
        self.samples_in = self.windows_run = self.frames_out = 0

    def _open(self, eng):
        eng.long_stream_open(*self._cond)
        if self._pins is not None:
            eng.long_pool_pins(self._pins)

    @property
    def pins(self):
        """The pinned frames whose window has yet to run (every clip holds the same ones); 0 without ``pins=``."""
        return len(self._pending[0]) if self._pending else 0

    def pin(self, frames, poses, mask=None):
        """Pin poses of frames the stream has yet to return (opened with ``pins=H``), every clip alike: ``frames`` [K], distinct host
        ints in ``[frames_out, frames_out + H)``; ``poses`` [B, J, F, K]; ``mask`` [B, J, F, K] bool, True = pinned, default the whole
        pose.  The same as ``LongPool.pin`` on each of the B slots of the pool the stream runs on."""
        if self._closed:
            raise RuntimeError("the stream is closed")
        fr, poses, mask = self._check_pin(frames, poses, mask, (self._B,), self.frames_out)
        eng = self._engine()
        done = []
        try:                            # every clip or none: a call that fails midway takes back what the clips before it were given
            for b in range(self._B):
                eng.long_pool_pin(b, fr, poses[b], None if mask is None else mask[b])
                done.append(b)
        except Exception:
            fresh = np.array(sorted(set(fr.tolist()) - self._pending[0]), np.int64)     # frames pinned before keep their pins
            for b in done if fresh.size else ():
                eng.long_pool_unpin(b, fresh)
            raise
        for b in range(self._B):        # the mirror moves only once the engine holds the pins of all clips
            self._pending[b] |= set(fr.tolist())

    def unpin(self, frames=None):
        """Drop the pins of ``frames`` (None: all of them) of every clip."""
        if self._closed:
            raise RuntimeError("the stream is closed")
        fr = self._check_unpin(frames, self.frames_out)
        eng = self._engine()
        for b in range(self._B):        # an un-pin only clears: a clip it has reached stays cleared, and the mirror follows clip by clip
            eng.long_pool_unpin(b, fr)
            self._pending[b] = set() if fr is None else self._pending[b] - set(fr.tolist())

    def _feed(self, chunk, emo, text_features, closing, lazy=None):
        """``lazy`` (with ``input_sr=``): ``(n, feed)`` in place of ``chunk`` -- its 16 kHz samples per clip, known ahead, and the call that
        makes it (``_input_plan``), which runs behind every refusal."""
        if self._closed:
            raise RuntimeError("the stream is closed")
        rag, B, diffusion = self._rag, self._B, self._diffusion
        chunk, emo, text_features = _as_tensors(chunk, emo, text_features)
        if lazy is None and (chunk.ndim != 2 or int(chunk.shape[0]) != B):
            raise ValueError(f"audio_chunk must be [{B}, n], got {list(chunk.shape)}")
        self._check_held(emo, text_features, B)
        n = int(chunk.shape[1]) if lazy is None else int(lazy[0])
        first, k = _lib.long_stream_plan(self.samples_in, n, int(rag.audio_len), closing)
        emo = emo if emo is not None else self._emo
        text_features = text_features if text_features is not None else self._text
        if k and rag.n_prefix_tokens == 2 and emo is None and not self._have_emo:
            raise ValueError("the BEAT model needs emo [B] for the stream's first window: pass it to open_stream or to this push")
        if k and self._sag is not None and text_features is None and not self._have_text:
            raise ValueError("sag needs text_features [B, 512] for the stream's first window: pass them to this push")
        shape = (B, rag.njoints, rag.nfeats, rag.nframes)
        self._check_post_frames(k * (rag.nframes - rag.n_pre_seq) + (rag.n_pre_seq if k and first == 0 else 0))
        kw = dict(self._kw)
        if k and diffusion.noise_source != "philox":
            _check_tape_bound(diffusion, "open_stream", self._n_exec, shape, int(rag.latent_dim))
        eng = self._engine()
        calls = self._calls([list(range(B))] * k, np.full(B, first))       # every clip alike: a window is one call, plain or pinned
        if self._sag is not None and any(pinned for _, pinned, _ in calls):
            raise ValueError("a pinned window with sag= is not built")
        if k and diffusion.noise_source != "philox":
            if any(pinned for _, pinned, _ in calls):
                x, eps, nz, renoise = _call_draws(diffusion, rag, calls, self._n_exec, eng.D)
                kw["x_init"], kw["eps_tape"], kw["noise_tape"] = x.view((k,) + shape), eps.view(k, self._n_exec, 2, B, eng.D), nz.view((k, self._n_exec) + shape)
                if renoise is not None:
                    kw["inpaint_noise"] = renoise
            else:
                kw["x_init"], kw["eps_tape"], kw["noise_tape"] = ref_draws.RefDraws("cpu").windows(diffusion, k, self._n_exec, shape, eng.D)
            diffusion.last_tape_segments = 1
        if self._sag is not None:
            kw["sag"] = self._sag.engine()
            kw["text_features"] = None if text_features is None else text_features.float()
        if lazy is not None:
            chunk = lazy[1]()
        out_dev = self._last_dev = chunk.device
        frames, ran = eng.long_stream_push(chunk.float(), closing=closing, emo=emo, device_out=out_dev.type == "cuda", **kw)
        self._have_emo, self._have_text = self._have_emo or emo is not None, self._have_text or text_features is not None
        self._emo = self._text = None                   # the engine holds them now
        self._closed = bool(closing)
        self._consume(calls, np.full(B, first), range(B) if closing else ())
        self.samples_in += n
        self.windows_run += ran
        self.frames_out += int(frames.shape[3])
        assert (first, k) == (self.windows_run - ran, ran)
        frames = gd._as_tensor(frames, out_dev)
        if self._post_kind is None:
            return frames
        return frames, self._post_push(frames, None, np.full(B, bool(closing)), chunk)

    def push(self, audio_chunk, emo=None, text_features=None):
        """Feed ``audio_chunk`` [B, n], n >= 0; returns the new frames ``[B, J, F, k]`` of the windows it completed (k may be 0); with
        ``post=``, ``(frames, post_dict)``.  With ``input_sr=``: ``[B, n]`` or ``[B, n, C]`` at that rate."""
        if self._in is None:
            return self._feed(audio_chunk, emo, text_features, False)
        if self._closed:
            raise RuntimeError("the stream is closed")
        count, feed = self._input_plan(audio_chunk)                 # every clip is fed alike: the counts are equal
        res = self._feed(None, emo, text_features, False, lazy=(count[0], feed))
        self.input_samples_in = int(self._in.samples_in[0])
        return res

    def close(self, emo=None, text_features=None):
        """End the stream: the frames of the windows ``plan_windows(samples_in)`` still owes, with silence behind the last sample."""
        tail = th.zeros((self._B, 0), device=self._last_dev)       # on the device of the last chunk
        if self._in is None or self._closed or not self.input_samples_in:
            return self._feed(tail, emo, text_features, True)
        count, feed = self._input_plan(None, finish=np.ones(self._B, bool))       # the resampler's last outputs come first
        res = self._feed(None, emo, text_features, True, lazy=(count[0], feed))
        self._in.close()
        return res


def open_stream(diffusion, model, seed_poses, vid_indices, scale, emo=None, sampler='ddim', skip_timesteps=0, eta=0.0, clip_denoised=False,
                sag=None, post=None, score=None, max_seconds=None, input_sr=None, input_channels=1, resample=None, pins=None):
    """The online form of ``sample_long``: a session that is fed audio in chunks of any size and returns a window's new frames as soon
    as that window's audio is complete.

        st = open_stream(diffusion, model, seed_poses, vid_indices, scale, emo=None, sampler='ddim', ...)
        new = st.push(audio_chunk, emo=None, text_features=None)    # [B, n], n >= 0  ->  [B, J, F, k] on the chunk's device
        tail = st.close(emo=None, text_features=None)               # the windows plan_windows(total) still owes, zero-padded

    The frames of all pushes and the close, concatenated, are bit for bit what ``sample_long`` gives for the concatenated audio with the
    same model, schedule, conditioning and seed (no ``n_windows``, no ``audio_lengths``), whatever the chunking
    (tests/test_gpu_long_stream.py).  A push runs, in order, every window w with ``32000 w + audio_len <= samples_in``
    (``ls_long_stream_plan``); k is 34 for window 0 and 30 for each later one, and a push that completes no window returns
    ``[B, J, F, 0]`` and launches no sampling work.  ``close`` on exactly ``audio_len + 32000 m`` samples returns no frame.  After
    ``close`` (or after leaving the ``with`` block the session also works as) a push raises ``RuntimeError``.

    ``emo`` (BEAT, [B]) and ``text_features`` ([B, 512], with ``sag=``) are HELD: what a push or ``close`` passes applies to every window
    started from then on.  The first window needs a value.  In ``sample_long`` terms window w sees ``emo[:, w]`` /
    ``text_features[:, w]`` equal to the value held when it ran.

    Noise (``diffusion.noise_source``): ``'torch_cpu'`` draws a window's tape at the push that runs it, in window order
    (``RefDraws.windows`` per push; the one-window ``tape_segment_bytes`` bound applies); ``'philox'`` takes its key here, once, and
    window w draws at ``sample_offset + b + (w << 48)`` -- clip b is keyed as a clip of a keyed pool is (``open_pool(noise_keys='clip')``),
    with ``key = sample_offset + b`` -- and a key must not repeat, so a stream runs at most 2^16 windows under
    ``'philox'`` (about 36 hours of audio; the push that would run the next one raises ``_lib.EngineError``); ``'torch_device'`` is
    refused.

    The engine runs a stream as an ``open_pool`` session whose B slots are joined at the open and fed alike: per clip a ring of
    ``audio_len + 32000`` samples, the hand-off poses and the held conditioning, plus one gathered window and one window's features.
    Device memory does not grow with the stream (``ls_long_stream_info``).  The engine is bound at the first push; a ``ddim_sample_loop``,
    ``sample_long`` or ``edit_long`` on the same model afterwards replaces its conditioning and ends the stream (the next push raises
    ``_lib.EngineError``).

    ``post='ted'`` / ``'beat'`` (the model's own dataset): the session owns a ``postprocess.open_post_stream`` of B slots, and ``push``
    and ``close`` return ``(frames, post_dict)`` -- ``PostStream.push``'s dict for the new frames (poses, the change curve or the Euler
    planes, and the motion beats that have just become decidable); ``close`` finishes every series.  The frames go from the engine to
    the post-processing kernels on the device when the audio was on the device.  The frames themselves are bit for bit those of
    ``post=None``, which changes nothing.  A call may complete at most 256 frames per clip then (8 windows).

    ``score=True`` (or a dict of ``postprocess.open_score_stream``'s options) with ``post=`` and ``max_seconds=`` (the audio a clip may
    hold): the session also owns a score stream of B slots.  It is fed the audio of every push and the beats of the post stream, and
    ``close`` adds ``'score'`` to its post dict: ``{'slots': {b: count, onset_raw, align_sum, n_beats | align, ...}, 'bc': ...}`` (BEAT:
    ``'align'`` [B]), which is what ``score_timeline`` gives for the concatenated frames and audio -- without its limits of 4096 frames.
    ``score=True`` without ``post=`` raises; with ``score`` unset nothing changes.

    ``input_sr=`` (an integer rate in Hz; with it ``input_channels=`` and ``resample=``, a dict of ``audio_io.resample``'s ``zeros``, ``beta``,
    ``rolloff`` and of ``max_chunk``): ``push`` takes chunks at THAT rate, ``[B, n]`` or interleaved ``[B, n, C]``, float32 or int16 (as the
    first push has it), at most ``max_chunk`` (65536) frames each.  The session owns an ``audio_io.ResampleStream`` of B slots on the
    engine's device; what it emits is what the windows see, so the frames are bit for bit those of a plain stream fed
    ``audio_io.resample(whole, input_sr)`` (tests/test_gpu_long_stream_sr.py).  A chunk on the device stays there; ``close`` finishes the
    resampler first.  ``samples_in`` stays in 16 kHz samples, ``input_samples_in`` counts the frames fed.  ``score=True`` sees the resampled
    audio.  ``input_sr=None``: nothing changes.

    Clips that join or leave while others run, each fed at its own rate: ``open_pool``.

    ``pins=H`` (an int >= 34; None: nothing changes) lets ``stream.pin(frames [K], poses [B, J, F, K], mask=None)`` pin poses of frames the
    stream has yet to return, every clip alike, and ``stream.unpin(frames=None)`` drop them: ``open_pool``'s pins on the B slots the
    stream runs on (see there; ``stream.pins`` counts the pinned frames still to come).

    Not built: ``audio_lengths`` / ``drop_finished``, ``edit_long`` on frames a running stream has already returned, pins with ``sag=``, PLMS, ``const_noise``, ``dump_steps``,
    sharded calls, a non-blocking ``push``."""
    return LongStream(diffusion, model, seed_poses, vid_indices, scale, emo, sampler, skip_timesteps, eta, clip_denoised, sag, post, score, max_seconds,
                      input_sr, input_channels, resample, pins)


def pool_plan(samples_in, windows_run, new, closing, open, cfg):
    """What one ``LongPool.push`` runs, from host counts alone (no GPU): ``(rounds, frames)``.

    Each of the S slots is a stream of its own: slot s, open, with ``samples_in[s]`` samples fed and ``windows_run[s]`` windows run so
    far, receives ``new[s]`` samples, and runs the windows ``_lib.long_stream_plan(samples_in[s], new[s], audio_len, closing[s])`` names.
    ``rounds[r]`` lists, ascending, the slots that still have a window to run after r earlier rounds of the call; slot s runs its window
    ``windows_run[s] + r`` there, and the round is one sampling call at batch ``len(rounds[r])``.  ``frames`` (int32 [S]): 34 frames for
    a slot's window 0, 30 for each later one.  ``ValueError``: samples for a slot that is not open, closing a slot that was never fed,
    negative counts.  One definition for the engine and for this module (``ls_long_pool_plan``)."""
    return _lib.long_pool_plan(samples_in, windows_run, new, closing, open, int(cfg.audio_len))


class LongPool(_Session):
    """A running ``open_pool`` session; see there.  ``slots``: per-slot host arrays ``samples_in``, ``windows_run``, ``frames_out``, ``open``,
    and in a keyed pool ``key`` (uint64; of a free slot: its last clip's)."""

    def __init__(self, diffusion, model, capacity, sampler, skip_timesteps, eta, clip_denoised, sag, post=None, noise_keys=None, score=None,
                 max_seconds=None, input_sr=None, input_channels=1, resample=None, pins=None):
        S = int(capacity)
        if S < 1:
            raise ValueError(f"capacity must be >= 1, got {capacity}")
        if noise_keys not in (None, "clip"):
            raise ValueError(f"noise_keys must be None or 'clip', got {noise_keys!r}")
        if noise_keys == "clip" and diffusion.noise_source != "philox":
            raise ValueError(f"noise_keys='clip' keys Philox draws: noise_source is {diffusion.noise_source!r}, not 'philox'")
        rag = getattr(model, "model", None)
        beat = getattr(rag, "n_prefix_tokens", 1) == 2
        npre, J, F = (int(getattr(rag, k, 1)) for k in ("n_pre_seq", "njoints", "nfeats"))
        # _check_args on a one-window stand-in at batch S: the slots' own conditioning arrives with the joins
        _check_args(diffusion, model, th.empty(S, 1), th.empty(S, J, F, npre), th.zeros(S, dtype=th.long), th.ones(S),
                    th.zeros(S, dtype=th.long) if beat else None, None, sampler, skip_timesteps, sag,
                    None if sag is None else th.empty(S, 1, int(rag.latent_dim)), None, {})
        _check_model(diffusion, rag)
        self._diffusion, self._rag, self._sag, self._S = diffusion, rag, sag, S
        self._init_post(post, rag, S, score, max_seconds)
        self._init_input(input_sr, input_channels, resample, S)
        self._init_pins(pins, rag, S)
        self._kw = _loop_kw(diffusion, sampler, skip_timesteps, eta, clip_denoised)
        self._keyed, self._joins = noise_keys == "clip", 0
        if diffusion.noise_source == "philox":          # one seed per pool: row r of round q draws at sample_offset + r + (q << 48); keyed: at the clip's key
            self._kw.update(diffusion._philox_key())
            self._offset = int(self._kw["sample_offset"])
            if self._keyed and not 0 <= self._offset < 1 << 48:
                raise ValueError(f"noise_keys='clip': sample_offset {self._offset} outside [0, 2^48) (the default keys start there)")
        else:                                           # the largest round a push can run (with pins on TED: and its re-noise tape)
            _check_tape_bound(diffusion, "open_pool", diffusion.num_timesteps - int(skip_timesteps), (S, J, F, int(rag.nframes)), int(rag.latent_dim),
                              renoised=self._pins is not None and not beat)
        self._n_exec = diffusion.num_timesteps - int(skip_timesteps)
        self._eng = None
        self._closed = False
        self._last_dev = th.device("cpu")
        self._state = {"samples_in": np.zeros(S, np.int64), "windows_run": np.zeros(S, np.int64), "frames_out": np.zeros(S, np.int64),
                       "open": np.zeros(S, bool)}
        if self._keyed:
            self._state["key"] = np.zeros(S, np.uint64)
        if self._pins is not None:
            self._state["pins"] = np.zeros(S, np.int64)
        self._have_text = np.zeros(S, bool)

    @property
    def slots(self):
        out = {k: v.copy() for k, v in self._state.items()}
        if self._in is not None:
            out["input_samples_in"] = self._in.samples_in          # frames at input_sr of each slot's running clip
        return out

    def _open(self, eng):
        eng.long_pool_open(self._S)
        if self._keyed:
            eng.long_pool_keyed(True)
        if self._pins is not None:
            eng.long_pool_pins(self._pins)

    def _refresh(self):
        info = self._eng.long_pool_info()
        for k in self._state:
            if k not in ("key", "pins"):        # the keys are held here: the engine has what join set
                self._state[k] = np.array(info[k])
        if self._pins is not None:              # the engine's count of pending pinned frames; the frames themselves are mirrored here
            self._state["pins"] = self._eng.long_pool_pin_info()["pending"].astype(np.int64)
            assert self._state["pins"].tolist() == [len(p) for p in self._pending], (self._state["pins"], self._pending)

    def join(self, seed_poses, vid_index, scale, emo=None, text_features=None, slot=None, key=None):
        """Open a slot for a new clip: ``seed_poses`` [J, F, n_pre], its speaker id and guidance scale, ``emo`` (BEAT: required) and
        ``text_features`` [512] (with ``sag=``; may also come with the push that runs the slot's first window).  Returns the slot: the
        lowest free one unless ``slot`` names one.  Nothing is sampled and nothing is drawn.  ``key`` (a pool opened with
        ``noise_keys='clip'`` only; ``ValueError`` otherwise): the clip's Philox key, an int in [0, 2^48); default
        ``diffusion.sample_offset`` + the joins since the pool was opened."""
        if self._closed:
            raise RuntimeError("the pool is closed")
        if key is not None:
            if not self._keyed:
                raise ValueError("join(key=) needs a keyed pool: open_pool(..., noise_keys='clip')")
            if isinstance(key, bool) or not isinstance(key, (int, np.integer)) or not 0 <= int(key) < 1 << 48:
                raise ValueError(f"key must be an int in [0, 2^48), got {key!r}")
        rag, S = self._rag, self._S
        seed_poses, text_features = _as_tensors(seed_poses, text_features)
        if _shape(seed_poses) != (rag.njoints, rag.nfeats, rag.n_pre_seq):
            raise ValueError(f"seed_poses must be {[rag.njoints, rag.nfeats, rag.n_pre_seq]}, got {list(seed_poses.shape)}")
        if rag.n_prefix_tokens == 2:
            if emo is None:
                raise ValueError("the BEAT model needs emo: one id for the clip that joins")
        elif emo is not None:
            raise ValueError("emo is a BEAT conditioning; the TED model takes none")
        if text_features is not None:
            if self._sag is None:
                raise ValueError("text_features without sag: the SAG decoder turns them into every window's init_image")
            if _shape(text_features) != (rag.latent_dim,):
                raise ValueError(f"text_features must be [{rag.latent_dim}], got {list(text_features.shape)}")
        free = [s for s in range(S) if not self._state["open"][s]]
        if slot is None:
            if not free:
                raise ValueError(f"all {S} slots of the pool are occupied")
            slot = free[0]
        slot = int(slot)
        if not 0 <= slot < S:
            raise ValueError(f"slot {slot} outside [0, {S})")
        if slot not in free:
            raise ValueError(f"slot {slot} is occupied")
        one = lambda v, dt: (v.detach().reshape(1).to(dt) if th.is_tensor(v) else th.tensor([v], dtype=dt))      # noqa: E731
        eng = self._engine()
        eng.long_pool_join(slot, seed_poses.float(), one(vid_index, th.long), one(scale, th.float32), None if emo is None else one(emo, th.long),
                           None if text_features is None else text_features.float())
        if self._keyed:
            k = (self._offset + self._joins) % (1 << 48) if key is None else int(key)
            eng.long_pool_set_key(slot, k)
            self._state["key"][slot] = k
        self._joins += 1
        if self._in is not None:
            self._in.reset(slot)          # a new series at sample 0 (a slot that left or was closed is empty already)
        if self._pins is not None:
            self._pending[slot].clear()   # a new clip starts with no pin (the engine's join drops them too)
        self._refresh()
        self._have_text[slot] = text_features is not None
        return slot

    def _feed(self, audio, lengths, closing, emo, text_features, given, lazy=None):
        """``lazy`` (with ``input_sr=``): the call that makes ``audio`` (``_input_plan``) -- ``lengths`` are then its 16 kHz counts, known
        ahead -- which runs behind every refusal."""
        if self._closed:
            raise RuntimeError("the pool is closed")
        rag, S, diffusion = self._rag, self._S, self._diffusion
        audio, emo, text_features = _as_tensors(audio, emo, text_features)
        if lazy is None and (audio.ndim != 2 or int(audio.shape[0]) != S):
            raise ValueError(f"audio must be [{S}, n_max], got {list(audio.shape)}")
        n_max = int(audio.shape[1]) if lazy is None else int(np.max(lengths))
        lens = _lib.host_lengths(lengths, S, 0, n_max, "lengths").astype(np.int64)
        self._check_held(emo, text_features, S)
        st = self._state
        if given is None:                               # what is passed holds for every open slot
            given = st["open"].copy()
        given = np.asarray(given.detach().cpu().numpy() if hasattr(given, "detach") else given).reshape(-1).astype(bool)
        if given.shape != (S,) or (given & ~st["open"]).any():
            raise ValueError(f"given must mark open slots only, one entry per slot: got {given.tolist()} for open {st['open'].tolist()}")
        bits = given.astype(np.int32) * ((1 if emo is not None else 0) | (2 if text_features is not None else 0))
        rounds, owed = pool_plan(st["samples_in"], st["windows_run"], lens, closing, st["open"], rag)
        self._check_post_frames(int(owed.max()) if len(owed) else 0)
        ending = np.asarray(closing).astype(bool) & st["open"]
        for s in {s for r in rounds for s in r}:
            if self._sag is not None and st["windows_run"][s] == 0 and not self._have_text[s] and not bits[s] & 2:
                raise ValueError(f"sag needs text_features [512] for slot {s}'s first window: pass them to join or to this push")
        kw = dict(self._kw)
        calls = self._calls(rounds, st["windows_run"])              # the rounds, split where pending pins say so
        if self._sag is not None and any(pinned for _, pinned, _ in calls):
            raise ValueError("a pinned window with sag= is not built: unpin the frames, or open the pool without sag")
        eng = self._engine()
        if calls and diffusion.noise_source != "philox":            # one public sampling call per call of the plan, at its batch, in order
            kw["x_init"], kw["eps_tape"], kw["noise_tape"], renoise = _call_draws(diffusion, rag, calls, self._n_exec, eng.D)
            if renoise is not None:
                kw["inpaint_noise"] = renoise
            diffusion.last_tape_segments = 1
        if self._sag is not None:
            kw["sag"] = self._sag.engine()
        if lazy is not None:
            audio = lazy()
        out_dev = self._last_dev = audio.device
        frames, counts, ran = eng.long_pool_push(audio.float(), lens, closing=closing, emo=emo if bits.any() else None,
                                                 text_features=None if text_features is None or not bits.any() else text_features.float(),
                                                 given=bits if bits.any() else None, device_out=out_dev.type == "cuda", **kw)
        assert ran == rounds
        self._have_text |= (bits & 2).astype(bool)
        self._consume(calls, st["windows_run"], np.nonzero(ending)[0])
        self._refresh()
        self._have_text &= self._state["open"]
        frames = gd._as_tensor(frames, out_dev)
        if self._post_kind is None:
            return frames, counts
        return frames, counts, self._post_push(frames, counts, ending, audio, lens)

    def push(self, audio, lengths, emo=None, text_features=None, given=None):
        """Feed ``audio`` [S, n_max]: ``lengths[s]`` samples for slot s (0 for a slot that is free or has nothing new).  Returns
        ``(frames [S, J, F, K], counts)``: slot s's new frames in ``frames[s, ..., :counts[s]]``, zero behind them; K = max(counts).
        With ``post=``: ``(frames, counts, post_dict)``.  With ``input_sr=``: ``[S, n_max]`` or ``[S, n_max, C]`` at that rate, ``lengths`` in its
        frames."""
        if self._in is None:
            return self._feed(audio, lengths, np.zeros(self._S, np.int32), emo, text_features, given)
        if self._closed:
            raise RuntimeError("the pool is closed")
        n_max = int(audio.shape[1]) if hasattr(audio, "shape") and len(audio.shape) >= 2 else 0
        lens = _lib.host_lengths(lengths, self._S, 0, n_max, "lengths")
        if (lens[~self._state["open"]] > 0).any():
            raise ValueError(f"samples for a slot that is not open: lengths {lens.tolist()}, open {self._state['open'].tolist()}")
        count, feed = self._input_plan(audio, lens)
        return self._feed(None, count, np.zeros(self._S, np.int32), emo, text_features, given, lazy=feed)

    def pin(self, slot, frames, poses, mask=None):
        """Pin poses of frames the clip in ``slot`` has yet to return (a pool opened with ``pins=H``): ``frames`` [K], distinct host
        ints in ``[slots['frames_out'][slot], ... + H)`` in the numbering of the slot's returned frames; ``poses`` [J, F, K]; ``mask``
        [J, F, K] bool, True = pinned, default the whole pose; host or device.  The window that owns a pinned frame runs through the
        reference's inpainting branch and keeps the pinned elements (``open_pool``).  Elements a later call's mask leaves out keep what
        an earlier call pinned.  ``ValueError`` ahead of any engine call for every refusal."""
        if self._closed:
            raise RuntimeError("the pool is closed")
        slot = int(slot)
        if not 0 <= slot < self._S or not self._state["open"][slot]:
            raise ValueError(f"slot {slot} is not open")
        fr, poses, mask = self._check_pin(frames, poses, mask, (), int(self._state["frames_out"][slot]))
        self._engine().long_pool_pin(slot, fr, poses, mask)
        self._pending[slot] |= set(fr.tolist())
        self._refresh()

    def unpin(self, slot, frames=None):
        """Drop the pins of ``frames`` (same range as in ``pin``; a frame that holds none is no error) of ``slot``, or all of them."""
        if self._closed:
            raise RuntimeError("the pool is closed")
        slot = int(slot)
        if not 0 <= slot < self._S or (frames is not None and not self._state["open"][slot]):
            raise ValueError(f"slot {slot} is not open")
        fr = self._check_unpin(frames, int(self._state["frames_out"][slot]))
        self._engine().long_pool_unpin(slot, fr)
        self._pending[slot] = set() if fr is None else self._pending[slot] - set(fr.tolist())
        self._refresh()

    def _leave(self, which):
        closing = np.zeros(self._S, np.int32)
        closing[which] = 1
        J, F = int(self._rag.njoints), int(self._rag.nfeats)
        if self._in is not None and closing.any():      # the resampler's last outputs of the slots that leave come first
            held = self._in.samples_in > 0
            if not held[closing.astype(bool)].all():
                raise ValueError(f"closing a slot that was fed no sample: slots {np.nonzero(closing.astype(bool) & ~held)[0].tolist()}")
            count, feed = self._input_plan(None, finish=closing.astype(bool))
            return self._feed(None, count, closing, None, None, None, lazy=feed)
        if not closing.any():
            frames, counts = th.zeros((self._S, J, F, 0), device=self._last_dev), np.zeros(self._S, np.int32)
            if self._post_kind is None:
                return frames, counts
            return frames, counts, (self._post_push(frames, counts, None) if self._eng is not None else None)      # no engine: nothing was ever fed
        return self._feed(th.zeros((self._S, 0), device=self._last_dev), np.zeros(self._S, np.int64), closing, None, None, None)

    def leave(self, slot):
        """End slot ``slot``'s clip: the frames ``[J, F, k]`` of the windows ``plan_windows(samples_in)`` still owes it, with silence
        behind its last sample.  The slot is free afterwards.  With ``post=``: ``(frames, counts, post_dict)`` -- the slot's frames, the
        call's counts [S] and the post-processing of the call (rows of the other slots are empty), which finishes the slot's series."""
        slot = int(slot)
        if not 0 <= slot < self._S or not self._state["open"][slot]:
            raise ValueError(f"slot {slot} is not open")
        res = self._leave([slot])
        frames = res[0][slot, :, :, :int(res[1][slot])]
        return frames if self._post_kind is None else (frames, res[1], res[2])

    def close(self):
        """Leave every open slot and end the session: ``(frames [S, J, F, K], counts)`` as from ``push``."""
        res = self._leave(np.nonzero(self._state["open"])[0])
        self._closed = True
        if self._post is not None:
            self._post.close()            # every series has been finished by the call above
        if self._score is not None:
            self._score.close()
        if self._in is not None:
            self._in.close()
        return res


def pool_keys(keys, windows_run, n_windows):
    """The key table of one push of a keyed pool (``open_pool(noise_keys='clip')``), from host counts alone (no GPU): uint64
    [sum n_windows] in ``pool_plan``'s row order.  Slot s, holding ``keys[s]`` in [0, 2^48) with ``windows_run[s]`` windows run, runs
    ``n_windows[s]`` windows in this push; its row in round r draws every Philox stream at ``gidx = keys[s] + ((windows_run[s] + r) <<
    48)``.  ``ValueError``: a key of a running slot at or above 2^48; ``_lib.EngineError``: a clip's window index would reach 2^16.  One
    definition for the engine and for this module (``ls_long_pool_keys``)."""
    return _lib.long_pool_keys(keys, windows_run, n_windows)


def open_pool(diffusion, model, capacity, sampler='ddim', skip_timesteps=0, eta=0.0, clip_denoised=False, sag=None, post=None, noise_keys=None,
              score=None, max_seconds=None, input_sr=None, input_channels=1, resample=None, pins=None):
    """``open_stream`` for clips that start and stop at different times and arrive at different rates: a session pool of ``capacity``
    slots on ONE engine.

        pool = open_pool(diffusion, model, capacity, sampler='ddim', ...)
        slot = pool.join(seed_poses, vid_index, scale, emo=None, text_features=None, slot=None)     # the lowest free slot unless given
        frames, counts = pool.push(audio, lengths, emo=None, text_features=None, given=None)        # [S, n_max], [S] -> [S, J, F, K], [S]
        tail = pool.leave(slot)                                                                     # [J, F, k]; frees the slot
        frames, counts = pool.close()                                                               # leaves every open slot

    Every slot is a stream of its own: its frames, concatenated over the pushes and its ``leave``, are the chain ``open_stream`` defines
    for its audio (34 frames for its window 0, 30 for each later one, window w as soon as ``32000 w + audio_len`` of ITS samples are
    in).  What a push runs is ``pool_plan``: round r holds, ascending, the slots that still have a complete window after r earlier rounds
    of the call, and is one sampling call at batch A = the slots in it -- its own kernel plan, the single-pass shortcut when the scales
    of THOSE slots are all 1, its own captured loop (kept per batch size and replayed).  So S live speakers run at batch up to S, not as
    S engines at batch 1.

    ``emo`` (BEAT) is needed at ``join``; ``text_features`` (with ``sag=``) before a slot's first window, at ``join`` or with a push.
    Both are HELD per slot; a push replaces them for the slots marked in ``given`` (bool [S]; default: every open slot).

    Noise (``diffusion.noise_source``): ``'torch_cpu'`` draws, per round and in round order, what one public sampling call at batch A
    draws (``RefDraws.windows(diffusion, 1, n_exec, (A, J, F, T), D)``), and the result is bit for bit that loop of public calls on the
    active slots' windows (tests/test_gpu_long_pool.py); the one-window tape bound is checked at ``capacity``.  ``'philox'`` takes its
    key here, once: row r of the pool's q-th round since it was opened draws at ``sample_offset + r + (q << 48)``.  That is
    ``open_stream``'s key -- and its bits -- when the pool is used like a stream (all slots joined in order, fed alike); otherwise a
    clip's draws depend on the push schedule and on which slots run beside it.  A pool runs at most 2^16 rounds under ``'philox'``.
    ``'torch_device'`` is refused.

    ``noise_keys='clip'`` (needs ``'philox'``; ``ValueError`` otherwise) makes a clip's noise its own.  Every clip has a KEY, an int in
    [0, 2^48): ``join(key=)``, default ``diffusion.sample_offset`` + the joins since the pool was opened (a pool joined in order holds
    ``o, o + 1, ...``); ``pool.slots['key']`` lists them.  The clip in slot s draws in its own window w (``slots['windows_run'][s]``, 0
    again after a ``join``) at ``gidx = key + (w << 48)`` under the pool's one seed (``pool_keys`` is the table of a push).  THE CONTRACT:
    a clip's frames are a function of the model, the schedule, its own audio and conditioning, the seed and its key -- not of the other
    slots, the slot index, the chunking or the pool's age.  They are what ``sample_long`` gives for that audio with
    ``diffusion.sample_offset = key`` and the same seed: bit for bit where both runs go through the same kernel family at the same
    batch, and otherwise as far apart as two of the project's kernel families are.  So a session can be replayed or regenerated offline,
    one clip at a time.  Two open slots may hold the same key: same audio and conditioning then give the same frames; nothing polices
    it.  A clip may run 2^16 windows (the push that would run the next raises ``_lib.EngineError``); the pool's round count is no
    limit.  ``join(key=)`` on a pool that is not keyed raises ``ValueError``.  The draws of a keyed round are written to device tapes
    by one small launch per ring refill (csrc/ls_philox_rows.hip) and the step kernels read them as they read ``'torch_device'`` draws.

    Device memory is allocated for ``capacity`` slots when the engine is bound (the first ``join``) and does not grow
    (``Engine.long_pool_info()['device_bytes']``).  A ``ddim_sample_loop``, ``sample_long``, ``edit_long`` or ``open_stream`` push on the
    same model replaces the engine's conditioning and ends the pool (the next call raises ``_lib.EngineError``).  ``close`` and
    ``leave`` refuse a slot that was never fed a sample (``ValueError``), as ``LongStream.close`` does.

    ``post='ted'`` / ``'beat'`` (the model's own dataset): the pool owns a ``postprocess.open_post_stream`` of ``capacity`` slots;
    ``push``, ``leave`` and ``close`` return ``(frames, counts, post_dict)`` with ``PostStream.push``'s dict for the call's frames.
    ``leave`` and ``close`` finish the series of the slots they end, and a ``join`` into a freed slot starts a fresh one.  A call may
    complete at most 256 frames per slot then.  With ``post=None`` nothing changes.  ``score=True`` (or a dict of
    ``postprocess.open_score_stream``'s options) with ``post=`` and ``max_seconds=``: the pool also owns a score stream of ``capacity``
    slots, fed the audio of every push and the post stream's beats; the post dict of a ``leave`` (and of ``close``) carries ``'score'``
    for the slots it finished -- each clip's own onsets and alignment score, as in ``open_stream``.

    ``input_sr=``, ``input_channels=``, ``resample=``: as in ``open_stream`` -- ``push`` takes ``[S, n_max]`` or ``[S, n_max, C]`` at that rate with
    ``lengths`` in its frames, through an ``audio_io.ResampleStream`` of ``capacity`` slots on the engine's device.  ``leave`` and ``close``
    finish the resampler of the slots they end before the windows those still owe; ``join`` resets its slot's resampler
    (``ResampleStream.reset``; a no-op for a slot that left).  ``slots['samples_in']`` stays in 16 kHz samples,
    ``slots['input_samples_in']`` is added beside it.

    ``pins=H`` (an int >= 34, the horizon in frames; None: nothing changes, nothing is allocated) -- "be in this pose at frame 412", for
    frames a clip has yet to return::

        pool.pin(slot, frames [K], poses [J, F, K], mask=None)      # mask [J, F, K] bool, True = pinned; default: the whole pose
        pool.unpin(slot, frames=None)                               # None: every pin of the slot
        pool.slots['pins']                                          # pinned frames per slot whose window has yet to run

    ``frames`` are in the numbering of the slot's returned frames (``slots['frames_out']``), distinct, each in ``[frames_out,
    frames_out + H)``; host or device ``poses`` / ``mask``.  Window w of a slot covers its frames ``30 w .. 30 w + 33`` and OWNS all 34 for
    w = 0 and ``30 w + 4 ..`` otherwise (``edit_plan``'s ownership).  When the window that owns a pinned frame runs, it runs through the
    reference's inpainting branch (p_mean_variance, gaussian_diffusion.py:314-320; TED re-noises the kept motion, BEAT does not) with
    ``inpainting_mask`` True exactly on the pinned elements of the frames it owns -- its prefix frames are never kept, even when they
    carry a pin: the window before owned them and has honoured it -- and ``inpainted_motion`` the pinned values there, zero elsewhere.
    A window whose owned frames carry no pin runs exactly as without pins.  Each of ``pool_plan``'s rounds is split into at most two
    sampling calls (``pool_pin_plan``): its unpinned slots, ascending, as a plain call, then its pinned slots, ascending, as an
    inpainting call; an empty half is skipped.  So a clip without a pin never enters the inpainting kernels because a neighbour has
    one, and a pool with no pending pin makes precisely the calls it made before.  Every call is one public sampling call:
    ``'torch_cpu'`` draws what that call draws, in call order (``RefDraws.windows`` for a plain call, ``RefDraws.edit_windows`` for a pinned
    one), and the result is bit for bit that loop of public calls (tests/test_gpu_long_pool_pins.py); un-keyed ``'philox'`` draws row r
    of the q-th CALL since the open at ``sample_offset + r + (q << 48)``; ``noise_keys='clip'`` keeps the clip's key and its own window,
    so a pinned clip's frames still do not depend on its neighbours.  ``join`` starts a clip with no pin and ``leave`` drops the pins
    its clip never reached.  On the device: a ring of H (rounded up to a multiple of 4) frames of values and bytes per slot, written by
    ``k_pool_pin_store``, turned into a pinned call's inpainting planes by ``k_pool_pin_gather`` (csrc/ls_chain.hip), allocated when the
    engine is bound.  ``ValueError`` ahead of any engine call: a pool opened without ``pins=``, a slot that is not open, a frame below
    ``frames_out`` or at or beyond ``frames_out + H``, a frame named twice, wrong shapes, ``sag=``.  What a pinned round costs beside a
    plain one has not been measured.

    Not built: device-resident ``lengths``, ``edit_long`` on frames a pool has already returned, pins with ``sag=`` (a pinned window would
    start from ``edit_start(motion, mask, sag_out)``: a kernel form of its own), soft (fractional) pins, device-resident frame lists,
    PLMS, ``const_noise``,
    ``dump_steps``, sharded calls, a non-blocking ``push``."""
    return LongPool(diffusion, model, capacity, sampler, skip_timesteps, eta, clip_denoised, sag, post, noise_keys, score, max_seconds, input_sr,
                    input_channels, resample, pins)


def _edit_ranges(frames, B, n_frames):
    """``frames`` -- one (lo, hi) pair for every clip, or [B, 2] -- as host int32 (lo [B], hi [B]) with 0 <= lo <= hi <= n_frames."""
    if hasattr(frames, "detach"):
        frames = frames.detach().cpu().numpy()
    fr = np.asarray(frames)
    if fr.shape == (2,):
        fr = np.broadcast_to(fr, (B, 2))
    if fr.shape != (B, 2) or fr.dtype.kind not in "iu":
        raise ValueError(f"frames must be one integer (lo, hi) pair or [{B}, 2], got shape {list(fr.shape)} of {fr.dtype}")
    lo, hi = fr[:, 0].astype(np.int64), fr[:, 1].astype(np.int64)
    if (lo < 0).any() or (lo > hi).any() or (hi > n_frames).any():
        raise ValueError(f"every frame range must satisfy 0 <= lo <= hi <= {n_frames}, got {fr.tolist()}")
    return lo.astype(np.int32), hi.astype(np.int32)


def _edit_joints(joints, B, cfg):
    """``joints`` (None = all, or bool [J] / [B, J]) as a host bool [B, J]."""
    J = int(cfg.njoints)
    if joints is None:
        return np.ones((B, J), bool)
    if hasattr(joints, "detach"):
        joints = joints.detach().cpu().numpy()
    sel = np.asarray(joints)
    if sel.shape == (J,):
        sel = np.broadcast_to(sel, (B, J))
    if sel.shape != (B, J) or sel.dtype != np.bool_:
        raise ValueError(f"joints must be a bool mask [{J}] or [{B}, {J}], got shape {list(sel.shape)} of {sel.dtype}")
    return np.ascontiguousarray(sel)


def _edit_mask(mask, B, cfg, n_frames):
    """An element mask of ``edit_long`` -- bool, True = EDITABLE, numpy or torch on any device, shaped [N], [B, N], [B, J, N] or
    [B, J, F, N] (a leading 1 stands for every clip) -- as a contiguous bool tensor [B, J * F, N] on the mask's own device."""
    J, F, N = int(cfg.njoints), int(cfg.nfeats), int(n_frames)
    m = mask if hasattr(mask, "detach") else th.from_numpy(np.ascontiguousarray(mask))
    if m.dtype != th.bool:
        raise ValueError(f"mask must be bool (True = editable), got {m.dtype}")
    shape = _shape(m)
    lead = (1, B)
    ok = {1: shape == (N,), 2: len(shape) == 2 and shape[0] in lead and shape[1] == N,
          3: len(shape) == 3 and shape[0] in lead and shape[1:] == (J, N),
          4: len(shape) == 4 and shape[0] in lead and shape[1:] == (J, F, N)}.get(m.ndim, False)
    if not ok:
        raise ValueError(f"mask must be [{N}], [{B}, {N}], [{B}, {J}, {N}] or [{B}, {J}, {F}, {N}], got {list(shape)}")
    m = m.reshape({1: (1, 1, 1, N), 2: (shape[0], 1, 1, N), 3: (shape[0], J, 1, N), 4: shape}[m.ndim])
    return m.expand(B, J, F, N).reshape(B, J * F, N).contiguous()


def edit_mask(ranges, joints, n_frames, cfg):
    """The rectangle of the range form as an element mask: numpy bool [B, J, F, n_frames], True (= editable) on the joints ``joints``
    (None = all, bool [J] or [B, J]) and the frames ``lo_b <= n < hi_b`` of ``ranges`` ((lo, hi) or [B, 2]).  B is the ranges' or the
    joints' leading size (1 when neither has one).  ``edit_long(mask=edit_mask(r, j, N, cfg))`` is ``edit_long(frames=r, joints=j)``,
    bit for bit."""
    fr = np.asarray(ranges.detach().cpu().numpy() if hasattr(ranges, "detach") else ranges)
    sel = None if joints is None else np.asarray(joints.detach().cpu().numpy() if hasattr(joints, "detach") else joints)
    B = int(fr.shape[0]) if fr.ndim == 2 else int(sel.shape[0]) if sel is not None and sel.ndim == 2 else 1
    lo, hi = _edit_ranges(fr, B, int(n_frames))
    sel = _edit_joints(sel, B, cfg)
    n = np.arange(int(n_frames))
    inside = (n[None, :] >= lo[:, None]) & (n[None, :] < hi[:, None])
    return np.ascontiguousarray(np.broadcast_to(sel[:, :, None, None] & inside[:, None, None, :], (B, int(cfg.njoints), int(cfg.nfeats), int(n_frames))))


def keyframe_mask(n_frames, pinned_frames, cfg, joints=None, within=None):
    """The mask of in-betweening and of constrained generation: numpy bool [1, J, F, n_frames] (one mask for every clip), True
    (= editable) everywhere -- with ``within`` (one (lo, hi) pair or a list of them) only inside those frame ranges -- except on the
    ``pinned_frames`` (a sequence of frame indices), where the joints ``joints`` (bool [J]; None = all) are KEPT.  A timeline that
    holds poses at the pinned frames, this mask and ``skip_timesteps=0``: "generate a talk that passes through these poses"."""
    N, J, F = int(n_frames), int(cfg.njoints), int(cfg.nfeats)
    pins = np.asarray(list(pinned_frames), dtype=np.int64).reshape(-1)
    if ((pins < 0) | (pins >= N)).any():
        raise ValueError(f"pinned_frames must lie in [0, {N}), got {pins.tolist()}")
    sel = _edit_joints(joints, 1, cfg)[0]
    frames = np.ones(N, bool)
    if within is not None:
        pairs = np.asarray(within, dtype=np.int64).reshape(-1, 2)
        frames[:] = False
        for lo, hi in pairs:
            if lo < 0 or lo > hi or hi > N:
                raise ValueError(f"every range of `within` must satisfy 0 <= lo <= hi <= {N}, got {pairs.tolist()}")
            frames[lo:hi] = True
    mask = np.broadcast_to(frames[None, None, :], (J, F, N)).copy()
    mask[np.ix_(np.flatnonzero(sel), np.arange(F), pins)] = False
    return mask[None]


def _host_mask(mask, n_windows, cfg, frames=None):
    """``mask`` on the host as [B, J * F, N] for the plans: B from the mask ([N]: from ``frames``, else 1)."""
    N = _window_sizes(int(n_windows), cfg)[1]
    m = mask.detach().cpu() if hasattr(mask, "detach") else th.from_numpy(np.ascontiguousarray(mask))
    B = int(m.shape[0]) if m.ndim > 1 and int(m.shape[0]) != 1 else 1 if frames is None else int(np.asarray(frames).size)
    return _edit_mask(m, B, cfg, N).numpy()


def edit_plan(ranges, n_windows, cfg, mask=None):
    """The windows ``edit_long`` runs for the per-clip frame ranges ``ranges`` ((lo, hi) or [B, 2]) of a timeline of ``n_windows``
    windows, as a sorted list: window w runs when some clip's range meets the frames it OWNS -- [0, T) for w = 0,
    [w * S + n_pre, w * S + T) with S = T - n_pre otherwise, the frames it contributes to the stitched timeline.  No range meets any
    (all are empty): ``ValueError``.  One definition for the engine and for this module (``ls_long_edit_plan``).

    ``mask=`` (with ``ranges=None``; ``edit_long``'s element mask, True = editable): window w runs when some clip has a True element
    on a frame w owns (``ls_long_edit_plan_mask``).  An empty mask: ``ValueError``."""
    T, npre, W = int(cfg.nframes), int(cfg.n_pre_seq), int(n_windows)
    if mask is not None:
        if ranges is not None:
            raise ValueError("edit_plan: mask excludes ranges")
        windows = [w for w, _ in _lib.long_edit_plan_mask(_host_mask(mask, W, cfg), W, None, T, npre)]
        if not windows:
            raise ValueError("edit_plan: the mask is empty, no window would run")
        return windows
    fr = np.asarray(ranges.detach().cpu().numpy() if hasattr(ranges, "detach") else ranges)
    lo, hi = _edit_ranges(fr, 1 if fr.ndim == 1 else int(fr.shape[0]), _window_sizes(W, cfg)[1])
    windows = _lib.long_edit_plan(lo, hi, W, T, npre)
    if not windows:
        raise ValueError("edit_plan: every frame range is empty, no window would run")
    return windows


def edit_plan_compact(ranges, n_windows, cfg, joints=None, frames=None, mask=None):
    """The clip-windows the COMPACT ``edit_long`` runs, as a list of ``(w, rows)``: the windows that run, ascending, each with the
    clips that have an editable element in it, ascending (``rows``, a list of clip indices).  The pair (clip b, window w) is in the
    plan iff b's range meets the frames w OWNS (``edit_plan``'s rule), at least one joint of b is selected by ``joints`` (None = all,
    bool [J] or [B, J]), and -- with ``frames`` (int [B], a ragged batch: ``plan_lengths``) -- ``w`` is one of the clip's own
    ``(frames[b] - T) / S + 1`` windows.  Without ``frames`` the windows are exactly ``edit_plan``'s.  A range outside
    ``[0, frames[b]]``, ``lo > hi`` or a ``frames[b]`` that is no stitched length (34 + 30 k): ``ValueError``.  No pair at all is an
    empty list, which ``edit_long`` refuses.  One definition for the engine and for this module (``ls_long_edit_plan_compact``).

    ``mask=`` (with ``ranges=None`` and ``joints=None``; ``edit_long``'s element mask, True = editable): the pair (b, w) is in the plan
    iff clip b has a True element on a frame w owns and, with ``frames``, w is one of its own windows; a True element at or beyond
    ``frames[b]``: ``ValueError`` (``ls_long_edit_plan_mask``).  Both forms reduce to pair flags and share the rest."""
    T, npre, W = int(cfg.nframes), int(cfg.n_pre_seq), int(n_windows)
    if mask is not None:
        if ranges is not None or joints is not None:
            raise ValueError("edit_plan_compact: mask excludes ranges and joints")
        return [(w, [int(b) for b in rows]) for w, rows in _lib.long_edit_plan_mask(_host_mask(mask, W, cfg, frames), W, frames, T, npre)]
    fr = np.asarray(ranges.detach().cpu().numpy() if hasattr(ranges, "detach") else ranges)
    B = int(fr.shape[0]) if fr.ndim == 2 else 1 if frames is None else int(np.asarray(frames).size)      # one pair: for every clip of `frames`
    lo, hi = _edit_ranges(fr, B, _window_sizes(W, cfg)[1])
    sel = _edit_joints(joints, B, cfg)
    return [(w, [int(b) for b in rows]) for w, rows in _lib.long_edit_plan_compact(lo, hi, W, sel, frames, T, npre)]


def edit_window(timeline, w, ranges, joints, seed_poses, cfg, mask=None):
    """Window ``w`` of a timeline edit in plain torch: ``(origin_x, inpainting_mask, inpainted_motion)``, each [B, J, F, T], as
    ``edit_long`` hands them to the sampling loop.

    * ``inpainted_motion`` is the slice ``timeline[..., w * S : w * S + T]`` (a contiguous copy) -- of the timeline as the earlier
      windows of the call left it.
    * ``origin_x[..., :n_pre]`` is the slice's first ``n_pre`` frames for w > 0 (the hand-off ``sample_long`` makes) and ``seed_poses``
      for w = 0; beyond the prefix it is zero.
    * ``inpainting_mask`` is True where the given motion is KEPT (the reference's meaning): False exactly on the editable elements
      (b, j, :, f) -- joint j of ``joints`` (None = all, bool [J] or [B, J]) selected, ``lo_b <= w * S + f < hi_b``, and frame
      ``w * S + f`` owned by window w (``edit_plan``).  The first ``n_pre`` frames of a later window belong to the window before it
      and are never editable in it.
    * ``mask=`` (with ``ranges=None`` and ``joints=None``): ``edit_long``'s element mask for these clips, True = EDITABLE -- the
      opposite of the ``inpainting_mask`` returned.  Element (b, j, k, f) is editable iff ``mask[b, j, k, w * S + f]`` and frame
      ``w * S + f`` is owned by window w; nothing else changes."""
    T, npre = int(cfg.nframes), int(cfg.n_pre_seq)
    S, w = T - npre, int(w)
    B, J, F, N = _shape(timeline)
    if w < 0 or w * S + T > N:
        raise ValueError(f"window {w} lies outside a timeline of {N} frames")
    motion = timeline[..., w * S:w * S + T].contiguous()
    origin_x = th.zeros_like(motion)
    origin_x[..., :npre] = motion[..., :npre] if w > 0 else th.as_tensor(seed_poses).to(motion)
    if mask is not None:
        if ranges is not None or joints is not None:
            raise ValueError("edit_window: mask excludes ranges and joints")
        own = th.from_numpy((np.arange(T) >= npre) | (w == 0)).to(motion.device)
        editable = _edit_mask(mask, B, cfg, N).reshape(B, J, F, N)[..., w * S:w * S + T].to(motion.device) & own
        return origin_x, ~editable, motion
    lo, hi = _edit_ranges(ranges, B, N)
    sel = _edit_joints(joints, B, cfg)
    t = w * S + np.arange(T)
    frame_ok = (t[None, :] >= lo[:, None]) & (t[None, :] < hi[:, None]) & ((np.arange(T) >= npre) | (w == 0))[None, :]       # [B, T]
    editable = sel[:, :, None, None] & frame_ok[:, None, None, :]
    mask = th.from_numpy(~np.broadcast_to(editable, (B, J, F, T))).to(motion.device)
    return origin_x, mask, motion


def edit_start(motion, mask, sag_out):
    """The image a window of a SCRIPTED edit starts from, in plain torch on any device: ``where(mask, motion, sag_out)`` -- the
    existing motion where it is kept, the SAG decoder's output on the editable elements.  ``motion`` and ``mask`` are
    ``edit_window``'s ``inpainted_motion`` and ``inpainting_mask`` (True = kept), ``sag_out`` is the decoder's ``['output']``, all
    [B, J, F, T].  A clip that keeps everything starts from its slice, bit for bit.  On the device: ``k_edit_start``."""
    if _shape(motion) != _shape(mask) or _shape(motion) != _shape(sag_out) or mask.dtype != th.bool:
        raise ValueError(f"edit_start: motion, mask (bool) and sag_out share one shape, got {list(motion.shape)}, {list(mask.shape)} "
                         f"of {mask.dtype}, {list(sag_out.shape)}")
    return th.where(mask, motion, sag_out)


def edit_long(diffusion, model, timeline, frames, audio, seed_poses, vid_indices, scale, emo=None, joints=None, sampler='ddim',
              skip_timesteps=0, eta=0.0, clip_denoised=False, encoder_chunk=None, return_windows=False, sag=None, text_features=None,
              compact=None, audio_lengths=None, mask=None):
    """Re-synthesise a stretch of a timeline ``sample_long`` made: the frames ``frames`` -- one ``(lo, hi)`` pair for all clips or a
    host int array [B, 2], ``lo == hi`` leaves a clip alone -- on the joints ``joints`` (None = all; a bool mask [J] or [B, J]), with
    the conditioning of the ``sample_long`` call (``audio``, ``seed_poses``, ``vid_indices``, ``scale``, ``emo``).  Returns a new
    timeline; the caller's tensor is not modified.  ``return_windows=True``: ``(timeline, windows that ran, their raw samples
    [We, B, J, F, T])``.

    Only the windows of ``edit_plan`` are sampled, in ascending order, all clips each (one engine call: ``ls_long_prepare`` +
    ``ls_long_edit``; ``k_edit_gather`` / ``k_edit_scatter``, csrc/ls_chain.hip).  Window w runs the sampling loop with the inputs
    of ``edit_window`` -- the reference's inpainting branch (p_mean_variance, gaussian_diffusion.py:314-320; TED re-noises the kept
    motion, BEAT mixes it in as it is), ``init_image`` = the slice when ``skip_timesteps > 0`` (the edit starts from the existing
    motion, re-noised to the first executed step), x_T otherwise -- and its editable elements replace the timeline's; every other
    element of the result is the input's, bit for bit.  With ``noise_source='torch_cpu'`` the result is bit for bit the loop
    "for w in edit_plan: edit_window -> ddim_sample_loop / p_sample_loop -> write the editable elements back"
    (tests/test_gpu_long_edit.py; the draws: ``RefDraws.edit_windows``).  ``'philox'``: clip b draws, in window w, the streams of
    ``sample_offset + b + (w << 48)`` -- what ``sample_long`` draws there, whichever other windows run.  ``'torch_device'`` is refused.

    ``sag`` (a ``Decoder_TRANSFORMER``) with ``text_features`` is the SCRIPTED edit -- "re-do these frames, and make them mean this
    sentence" (the reference's test_LivelySpeaker_ted.py:85-113, on a stretch of a timeline).  Windows, order, ``edit_window``'s
    inputs, draws (the decoder in eval mode draws nothing) and the write-back are the same; only the image window w starts from
    changes::

        sag_out = sag({'x': origin_x_w, 'z': text_features[:, w], 'mask': ones[B, T]})['output']
        init_w  = edit_start(inpainted_motion_w, inpainting_mask_w, sag_out)        # kept: the existing motion; editable: the decoder's

    and ``init_image=init_w`` is passed at EVERY ``skip_timesteps >= 0`` (at 0 the loops use it as ``q_sample(init_image, T - 1,
    x_T)``, gaussian_diffusion.py:709-716, as ``sample_long(sag=)`` does).  ``origin_x_w`` is ``edit_window``'s, so the decoder of
    window w + 1 sees the frames window w has just written.  ``text_features`` is [B, W, 512], sized by the timeline's W windows as in
    ``sample_long`` (entries of windows that do not run are ignored), or [B, 512]: one script for the whole stretch.  A clip whose
    range misses a running window starts from its slice there; with ``joints`` only the selected joints start from the decoder.  The
    bitwise contract holds with ``edit_start`` in the loop above (tests/test_gpu_long_edit_sag.py); on the device it is one more
    kernel per window (``ls_long_edit_sag``; ``k_edit_start``).  One of ``sag`` / ``text_features`` without the other, a wrong
    shape, a decoder whose geometry is not the RAG model's or that sits on another device: ``ValueError``.

    ``compact=True`` runs only the CLIP-WINDOWS the edit touches (``edit_plan_compact``; ``ls_long_prepare_edit`` +
    ``ls_long_edit_compact``): window w is one sampling call at batch ``len(rows)`` on the clips that have an editable element in
    it -- its own kernel plan, the single-pass shortcut when the scales of THOSE clips are all 1 -- and only those clip-windows of
    audio go through the WavEncoder.  A clip outside a window's rows does not run in it; a clip in no window is returned as given.
    ``return_windows=True`` then returns ``(timeline, plan, raw samples [sum len(rows), J, F, T])`` with ``plan`` the list of
    ``(w, rows)``, the samples row after row in plan order.  The noise contract:

    * ``'torch_cpu'``: the draws of one public sampling call per planned window at batch ``len(rows)``, window after window
      (``RefDraws.edit_windows(batches=)``); the result is bit for bit the loop above run on ``timeline[rows]`` with those clips'
      ranges, joints, seed poses and conditioning (tests/test_gpu_long_edit_compact.py);
    * ``'philox'``: clip b draws, in window w, EVERY stream at ``sample_offset + b + (w << 48)`` -- the clip's index, not its row --
      so its edited frames do not depend on which other clips share its windows, and where every clip is in every running window the
      result is the dense call's, bit for bit.

    ``audio_lengths`` (a host sequence [B], each in [1, L]) edits a RAGGED batch, the timeline of ``sample_long(audio_lengths=...)``
    with or without ``drop_finished``; it implies the compact form (together with ``compact=False``: ``ValueError``).  Clip b has
    ``frames[b]`` frames and ``W_b`` windows (``plan_lengths``); its range must lie inside ``[0, frames[b]]`` (``ValueError``
    otherwise), windows ``w >= W_b`` never run for it, ``audio[b, audio_lengths[b]:]`` is never read and counts as silence, and the
    frames beyond ``frames[b]`` are returned bit for bit as given.  ``emo`` [B, W] and ``text_features`` [B, W, 512] are sized by the
    longest clip's W, in the caller's clip order; entries of pairs outside the plan are not used.

    To know, not to be surprised by:

    * a window behind the last edited one is NOT resampled, even though its four conditioning frames may have changed; widen the
      range to have it resampled;
    * in the dense form (``compact`` unset) a clip whose range misses a window that runs for another clip still runs in it, with every
      element kept; its result is discarded, and all W windows of every clip go through the WavEncoder.  The compact form does neither;
    * ``compact=None`` (the default) means the dense form unless ``audio_lengths`` is given.

    ``mask=`` (with ``frames=None`` and ``joints=None``; combined with either: ``ValueError``) makes "editable" DATA instead of a
    rectangle.  **In ``mask``, True means EDITABLE -- re-synthesise this element.**  That is the OPPOSITE of ``edit_window``'s
    ``inpainting_mask`` (and the reference's), where True means KEEP.  ``mask`` is bool, numpy or torch, host or device, shaped ``[N]``,
    ``[B, N]``, ``[B, J, N]`` or ``[B, J, F, N]`` in the timeline's own frame axis.  Element (b, j, k, f) of window w is editable iff
    ``mask[b, j, k, w * S + f]`` and frame ``w * S + f`` is owned by w (``edit_plan``'s ownership); with ``audio_lengths`` a True
    element at or beyond ``frames[b]`` is a ``ValueError``, not a silent no-op.  Several stretches in one call, keyframes pinned
    inside a stretch (``keyframe_mask``), other joints in other stretches and constrained generation (a timeline of pinned poses,
    everything else editable, ``skip_timesteps=0``) are all masks; ``edit_mask(ranges, joints, N, cfg)`` is the range form, and gives
    the range call's result bit for bit.  Everything above holds with the mask in place of the rectangle -- ``compact=``,
    ``audio_lengths=``, ``sag=`` / ``text_features=``, ``return_windows=``, both noise sources; the dense form runs window w iff some
    clip has an editable element in it, the compact form the pair (b, w) iff clip b has one (``edit_plan(mask=)`` /
    ``edit_plan_compact(mask=)``) -- and with ``'torch_cpu'`` the result is bit for bit the loop above with ``edit_window(mask=)``
    (tests/test_gpu_long_edit_mask.py).  The engine runs the same kernels and the same captured loop (``ls_long_edit_mask`` & co.).  A
    device mask stays on the device: ``k_edit_mask_pairs`` reduces it to one flag per clip-window and only those W * B bytes reach the
    host for planning.

    Not built: edits of frames a running stream or pool has already returned (frames still to come can be pinned: ``open_pool(pins=)``,
    ``open_stream(pins=)``), bit-packed masks, soft (fractional) masks, PLMS,
    ``const_noise``, ``dump_steps``, ``'torch_device'``, resampling windows behind
    the last edited one, the SAG encoder (motion -> latent) as the source of ``text_features`` (chain ``MOTIONCLIP`` yourself) and
    device-resident length arrays; in the dense form also ragged batches (``audio_lengths=``) and re-encoding only the edited windows'
    audio (all W windows go through the WavEncoder, as in ``sample_long``)."""
    from .cfg_sampler import ClassifierFreeSampleModel
    if not isinstance(model, ClassifierFreeSampleModel):
        raise TypeError(f"edit_long: pass livelyspeaker_amd.ClassifierFreeSampleModel(RAG), got {type(model).__name__}")
    if diffusion.noise_source == "torch_device":
        raise NotImplementedError("edit_long: noise_source='torch_device' is not built for chained windows; use 'torch_cpu' or 'philox'")
    if audio_lengths is not None and compact is not None and not compact:
        raise ValueError("edit_long: audio_lengths edits a ragged batch, which only the compact form does; drop compact=False")
    compact = bool(compact) or audio_lengths is not None
    timeline, audio, seed_poses, vid_indices, scale, emo, text_features = _as_tensors(timeline, audio, seed_poses, vid_indices, scale, emo,
                                                                                      text_features)
    rag = model.model
    T, npre = int(rag.nframes), int(rag.n_pre_seq)
    if timeline.ndim != 4 or _shape(timeline)[1:3] != (rag.njoints, rag.nfeats):
        raise ValueError(f"timeline must be [B, {rag.njoints}, {rag.nfeats}, N], got {list(timeline.shape)}")
    B, N = int(timeline.shape[0]), int(timeline.shape[3])
    if T != 34 or N < T or (N - T) % (T - npre):
        raise ValueError(f"a timeline holds 34 + 30 (W - 1) frames, got {N}")
    W = (N - T) // (T - npre) + 1
    if mask is not None and (frames is not None or joints is not None):
        raise ValueError("edit_long: mask (True = editable) says which frames and joints are edited; pass frames=None and joints=None with it")
    if mask is None and frames is None:
        raise ValueError("edit_long: pass the frames to edit, or mask=")
    if mask is not None:
        emask = _edit_mask(mask, B, rag, N)                            # bool [B, J * F, N] on the mask's device
    else:
        lo, hi = _edit_ranges(frames, B, N)
        sel = _edit_joints(joints, B, rag)
    if audio.ndim != 2 or int(audio.shape[0]) != B:
        raise ValueError(f"audio must be [{B}, L], got {list(audio.shape)}")
    if text_features is not None and text_features.ndim == 2 and _shape(text_features) == (B, rag.latent_dim):
        text_features = text_features[:, None, :].expand(B, W, rag.latent_dim)         # one script for the whole stretch
    _check_args(diffusion, model, audio, seed_poses, vid_indices, scale, emo, W, sampler, skip_timesteps, sag, text_features, encoder_chunk, {})
    _check_model(diffusion, rag)
    if mask is None:
        hi = np.where(sel.any(axis=1), hi, lo).astype(np.int32)       # a clip with no joint selected is not edited
    lens = frames = None
    if audio_lengths is not None:
        lens = _lib.host_lengths(audio_lengths, B, 1, int(audio.shape[1]), "audio_lengths")
        plans = plan_lengths(lens, rag)
        frames = np.array([f for _, f in plans], np.int32)
        if max(Wb for Wb, _ in plans) != W:
            raise ValueError(f"the timeline holds {W} windows, the longest of audio_lengths needs {max(Wb for Wb, _ in plans)}")
        if mask is None and (hi > frames).any():
            raise ValueError(f"every frame range must lie inside its own clip, 0 <= lo <= hi <= frames[b] = {frames.tolist()}, got "
                             f"{np.stack([lo, hi], axis=1).tolist()}")
        if mask is not None:
            beyond = th.arange(N, device=emask.device)[None, None, :] >= th.from_numpy(frames).to(emask.device)[:, None, None]
            if bool((emask & beyond).any()):
                raise ValueError(f"mask is True at or beyond a clip's own frames[b] = {frames.tolist()}; nothing is edited there")
    plan = None
    if mask is not None:
        channels, rect = None, dict(mask=emask)
        if emask.device.type == "cpu":                                 # a device mask is planned by the engine, from its pair flags
            plan = [(w, [int(b) for b in rows]) for w, rows in _lib.long_edit_plan_mask(emask.numpy(), W, frames, T, npre)]      # edit_plan_compact(mask=)
    else:
        channels = np.repeat(sel, rag.nfeats, axis=1)
        rect = dict(channels=channels)
        if compact:
            plan = edit_plan_compact(np.stack([lo, hi], axis=1), W, rag, joints=sel, frames=frames)
        else:
            windows = edit_plan(np.stack([lo, hi], axis=1), W, rag)
    if plan is not None and not plan:
        raise ValueError("edit_long: the mask is empty, no window would run" if mask is not None else
                         "edit_long: every frame range is empty, no window would run")
    out_dev = timeline.device
    eng = _bind_engine(diffusion, rag)
    if mask is not None:
        if plan is None:
            plan = [(w, [int(b) for b in rows]) for w, rows in eng.long_edit_mask_plan(emask, W, frames)]
            if not plan:
                raise ValueError("edit_long: the mask is empty, no window would run")
        windows = [w for w, _ in plan]
        lo = hi = None
    if compact:
        batches = [len(rows) for _, rows in plan]
        eng.long_prepare_edit(audio.float(), seed_poses.float(), vid_indices, scale.float(), lo, hi, emo=_emo_windows(emo, W, B), n_windows=W,
                              encoder_chunk=encoder_chunk, audio_lengths=lens, **rect)
        assert [(w, [int(b) for b in rows]) for w, rows in eng.edit_plan] == plan, (eng.edit_plan, plan)
    else:
        eng.long_prepare(audio.float(), seed_poses.float(), vid_indices, scale.float(), emo=_emo_windows(emo, W, B), n_windows=W,
                         encoder_chunk=encoder_chunk)
    n_exec = diffusion.num_timesteps - int(skip_timesteps)
    shape = (max(batches) if compact else B, rag.njoints, rag.nfeats, T)       # the compact form: its largest window batch
    noised = rag.n_prefix_tokens == 1                  # the TED tree re-noises the kept motion, the BEAT tree does not
    kw = dict(_loop_kw(diffusion, sampler, skip_timesteps, eta, clip_denoised), device_out=out_dev.type == "cuda", return_windows=return_windows,
              inpaint_noised=noised, **rect)
    if sag is not None:
        sag_eng = sag.engine()
        if sag_eng.device != eng.device:
            raise ValueError(f"the SAG decoder runs on cuda:{sag_eng.device}, the RAG model on cuda:{eng.device}")
        kw["sag"] = sag_eng
        kw["text_features"] = text_features.float().permute(1, 0, 2).contiguous()
    if diffusion.noise_source == "philox":
        kw.update(diffusion._philox_key())
    else:
        _check_tape_bound(diffusion, "edit_long", n_exec, shape, eng.D, renoised=noised)
        kw["x_init"], kw["eps_tape"], kw["noise_tape"], kw["inpaint_noise"] = ref_draws.RefDraws("cpu").edit_windows(
            diffusion, len(plan) if compact else len(windows), n_exec, shape, eng.D, noised, batches=batches if compact else None)
        diffusion.last_tape_segments = 1
    res = (eng.long_edit_compact if compact else eng.long_edit)(timeline.float(), lo, hi, **kw)
    if compact:
        res = (res[0], plan) + tuple(res[2:])
    edited = gd._as_tensor(res[0], out_dev)
    return (edited, res[1], gd._as_tensor(res[2], out_dev)) if return_windows else edited


def timeline_clips(x, stride=34, frames=None):
    """Frame-major timeline planes [B, N, C] (``aligned_motions``, ``decoded_motions``, ``pred_euler``) cut into 34-frame clips
    [B * K, 34, C], one every ``stride`` frames (K = (N - 34) // stride + 1; clip b * K + k starts at frame k * stride of timeline b), so
    that a timeline feeds ``EmbeddingSpaceEvaluator.push_samples`` / ``BeatEvaluator.push`` unchanged.  Tail frames that do not fill a
    clip are dropped.  torch ``unfold`` plus a reshape; numpy in, numpy out.

    ``frames`` (a host sequence [B], each in [1, N]): clip b holds ``frames[b]`` valid frames.  The result is then the pair (packed
    clips [sum K_b, 34, C], offsets [B + 1] host int64) with K_b = (frames[b] - 34) // stride + 1, and 0 for a clip shorter than 34
    frames; timeline b owns clips offsets[b] .. offsets[b + 1].  One advanced-indexing gather from indices built on the host."""
    as_np = isinstance(x, np.ndarray)
    t = th.as_tensor(x)
    if int(stride) < 1:
        raise ValueError(f"stride must be >= 1, got {stride}")
    if frames is not None:
        if t.ndim != 3:
            raise ValueError(f"expected [B, N, C], got {list(t.shape)}")
        B, N, Cn = _shape(t)
        fr = _lib.host_lengths(frames, B, 1, N, "frames").astype(np.int64)
        K = np.where(fr >= 34, (fr - 34) // int(stride) + 1, 0)
        offsets = np.zeros(B + 1, np.int64)
        np.cumsum(K, out=offsets[1:])
        rows = np.repeat(np.arange(B), K)
        first = (np.arange(int(offsets[-1])) - offsets[rows]) * int(stride)
        ri = th.from_numpy(rows).to(t.device)[:, None]
        fi = th.from_numpy(first[:, None] + np.arange(34)[None, :]).to(t.device)
        clips = t[ri, fi].contiguous()                                   # [sum K_b, 34, C]
        return (clips.numpy() if as_np else clips), offsets
    if t.ndim != 3 or int(t.shape[1]) < 34:
        raise ValueError(f"expected [B, N, C] with N >= 34, got {list(t.shape)}")
    B, _, Cn = _shape(t)
    clips = t.unfold(1, 34, int(stride)).permute(0, 1, 3, 2).reshape(-1, 34, Cn).contiguous()       # [B, K, C, 34] -> [B*K, 34, C]
    return clips.numpy() if as_np else clips


def score_timeline(timeline, audio, dataset="ted", sr=16000, device=0, target_euler=None, semantic=None, bc=None, frames=None,
                   audio_lengths=None, **options):
    """The whole chain behind ``sample_long``: post-process a stitched timeline [B, J, F, N] and score it against the ``audio`` [B, L] it
    was generated from, on the device (N up to 4096 frames; audio up to the onset detector's 4096 audio frames, 131 s at 16 kHz; longer
    talks: ``score_talk``).

    ``dataset='ted'``: ``ted_postprocess_timeline``, onsets as ``librosa.onset.onset_detect(y, sr=16000)`` finds them, and the
    beat-consistency score; returns pose, beat_mask, motion_beat_times and bc (this call's score, or the running score of the
    ``BeatConsistency`` passed as ``bc``).  ``dataset='beat'``: ``beat_postprocess_timeline``, onsets as ``alignment.load_audio``
    finds them, ``beat_metrics_timeline``; returns pred_euler, beat_mask, align [B], and srgr (the rate over the call) when
    ``target_euler`` [B, N, J*3] is given (``semantic`` [B, N] weighs its frames).  ``options`` go to the metric calls (BEAT: order,
    sigma, threshold, ...; TED: pad_mode, fmax, delta of the onset detector).

    ``frames`` [B] with ``audio_lengths`` [B] (host sequences, as ``sample_long(audio_lengths=)`` returns and takes them): clips of
    different lengths in one call.  N and L are then row strides, every clip is post-processed and scored at its own length (the
    ragged engine entries), the outputs are 0 beyond a clip's valid frames, BEAT's srgr divides by sum(frames) * J, and the limits of
    4096 frames apply per clip.  One without the other raises ``ValueError``."""
    from . import audio_onsets as ao
    from . import beat_metrics as bm
    from . import postprocess as pp
    if dataset not in ("ted", "beat"):
        raise ValueError(f"dataset must be 'ted' or 'beat', got {dataset!r}")
    if len(audio.shape) != 2 or int(audio.shape[0]) != int(timeline.shape[0]):
        raise ValueError(f"audio must be [B, L] with one row per timeline clip, got {list(audio.shape)}")
    if (frames is None) != (audio_lengths is None):
        raise ValueError("frames and audio_lengths go together: the valid frames of every timeline and the valid samples of its audio")
    B = int(timeline.shape[0])
    longest = int(audio.shape[1])
    if audio_lengths is not None:
        audio_lengths = _lib.host_lengths(audio_lengths, B, 1, longest, "audio_lengths")
        frames = _lib.host_lengths(frames, B, 1, int(timeline.shape[3]), "frames")
        longest = int(audio_lengths.max())
        audio = audio[:, :longest]                        # the row stride: nothing past the longest clip is looked at
    audio_frames = 1 + longest // ao.HOP
    if audio_frames > ao.MAX_FRAMES:
        raise NotImplementedError(f"the onset detector takes at most {ao.MAX_FRAMES} audio frames ({ao.MAX_FRAMES * ao.HOP / float(sr):.0f} s "
                                  f"at {sr} Hz); this audio has {audio_frames}")
    if dataset == "ted":
        post = pp.ted_postprocess_timeline(timeline, device=device, frames=frames)
        acc = bc if bc is not None else pp.BeatConsistency()
        acc.push_timeline(post["beat_mask"], audio=audio, sr=sr, device=device, frames=frames, audio_lengths=audio_lengths, **options)
        return {"pose": post["pose"], "beat_mask": post["beat_mask"], "motion_beat_times": post["motion_beat_times"],
                "bc": acc.score() if acc.num_beats else float("nan")}
    onset_opts = {k: options.pop(k) for k in ("pad_mode", "fmax") if k in options}
    post = pp.beat_postprocess_timeline(timeline, device=device, frames=frames)
    onsets = ao.onset_times(audio, sr, 22050, which="onset_bt_rms", time_sr=22050, device=device, lengths=audio_lengths, **onset_opts)
    want = ("beat_mask", "align") + (("srgr_sum",) if target_euler is not None else ())
    got = bm.beat_metrics_timeline(post["pred_euler"], target_euler, semantic, onsets, joints=int(timeline.shape[1]), device=device,
                                   want=want, frames=frames, **options)
    res = {"pred_euler": post["pred_euler"], "beat_mask": got["beat_mask"], "align": got["align"]}
    if target_euler is not None:
        s = got["srgr_sum"]
        s = s.detach().cpu().numpy() if hasattr(s, "detach") else np.asarray(s)
        total_frames = B * int(timeline.shape[3]) if frames is None else int(frames.astype(np.int64).sum())
        res["srgr"] = float(s.astype(np.float64).sum()) / (total_frames * int(timeline.shape[1]))
    return res


def score_talk(timeline, audio, dataset="ted", frames=None, audio_lengths=None, sr=16000, device=0, bc=None, chunk_seconds=4.0, **options):
    """``score_timeline`` without its limits: a stitched timeline [B, J, F, N] of ANY length against the ``audio`` [B, L] it was
    generated from -- a talk of a quarter of an hour is 13 500 pose frames and 28 126 audio frames.  It drives a
    ``postprocess.open_post_stream`` in 256-frame pushes and a ``postprocess.open_score_stream`` in chunks of ``chunk_seconds``, one slot
    per clip, so ``frames`` [B] and ``audio_lengths`` [B] (the clips' valid frames and samples; either may be None: all of them) make
    the call ragged for free.  Returns what ``score_timeline`` returns -- TED: pose, beat_mask [B, N], motion_beat_times, bc (this
    call's, or the running score of ``bc``); BEAT: pred_euler, beat_mask [B, 6, N - 1], align [B] -- zero beyond a clip's own frames,
    plus ``onset_count`` [B] and ``slots`` (the score stream's per-clip dicts).  Where ``score_timeline`` applies the numbers are the
    same bits.  ``options``: the score stream's (pad_mode, fmax, delta, sigma, ...) and, for BEAT, ``order`` and ``series_joints``.
    SRGR is not part of it (it needs targets frame by frame: ``beat_metrics_timeline`` up to 4096 frames)."""
    from . import postprocess as pp
    if dataset not in ("ted", "beat"):
        raise ValueError(f"dataset must be 'ted' or 'beat', got {dataset!r}")
    if len(timeline.shape) != 4:
        raise ValueError(f"expected a timeline [B, J, F, N], got {list(timeline.shape)}")
    B, J, _, N = (int(v) for v in timeline.shape)
    if len(audio.shape) != 2 or int(audio.shape[0]) != B:
        raise ValueError(f"audio must be [B, L] with one row per timeline clip, got {list(audio.shape)}")
    L = int(audio.shape[1])
    beat = dataset == "beat"
    order = int(options.pop("order", 2))
    series = options.pop("series_joints", pp.BEAT_SERIES_JOINTS)
    least = 2 * order + 2 if beat else 4
    frames = np.full(B, N, np.int64) if frames is None else _lib.host_lengths(frames, B, least, N, "frames").astype(np.int64)
    lens = np.full(B, L, np.int64) if audio_lengths is None else _lib.host_lengths(audio_lengths, B, 1, L, "audio_lengths").astype(np.int64)
    if N < least or L < 1:
        raise ValueError(f"need at least {least} frames and one sample per clip, got N = {N}, L = {L}")
    step = max(1, int(round(float(chunk_seconds) * float(sr))))
    ps = pp.open_post_stream(dataset, B, device=device, order=order, series_joints=series, joints=J)
    fps = float(options.get("fps", pp.TED_FPS))
    seconds = max(int(lens.max()) / float(sr), (int(frames.max()) + 1) / fps)          # the slots hold the audio and the motion beats
    ss = pp.open_score_stream(dataset, B, seconds, sr=sr, device=device, max_chunk=step, **options)
    rows, masks, firsts, counts = [], [], [], []
    try:
        for c0 in range(0, int(lens.max()), step):
            piece = audio[:, c0:c0 + step]
            ss.push(audio=piece, lengths=np.clip(lens - c0, 0, int(piece.shape[1])))
        K = pp.POST_STREAM_MAX_CHUNK
        for t0 in range(0, int(frames.max()), K):
            k = np.clip(frames - t0, 0, K)
            got = ps.push(timeline[..., t0:t0 + K], k, (frames > t0) & (frames <= t0 + K))
            ss.push(beats=got)
            rows.append(got["pred_euler" if beat else "pose"])
            masks.append(got["beat_mask"]), firsts.append(got["beat_first"]), counts.append(got["beat_count"])
        finished = ss.close()
    finally:
        ps.close()
        if not ss._closed:
            ss._closed = True
            if ss._eng is not None:
                ss._eng.close()
    host = lambda a: a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)      # noqa: E731
    mask = np.zeros((B, 6, N - 1) if beat else (B, N), bool)
    for m, first, count in zip(masks, firsts, counts):
        m = host(m)
        for b in range(B):
            mask[b, ..., int(first[b]):int(first[b]) + int(count[b])] = m[b, ..., :int(count[b])]
    if hasattr(rows[0], "detach"):
        import torch
        body, mask_out = torch.cat(rows, dim=1), torch.from_numpy(mask).to(rows[0].device)
    else:
        body, mask_out = np.concatenate(rows, axis=1), mask
    res = {"beat_mask": mask_out, "slots": finished, "onset_count": np.array([finished[b]["count"] for b in range(B)], np.int64)}
    if beat:
        res["pred_euler"] = body
        res["align"] = np.array([finished[b]["align"] for b in range(B)], np.float32)
        return res
    acc = bc if bc is not None else pp.BeatConsistency(sigma=ss.sigma)
    acc.push_score(finished)
    res["pose"] = body
    res["motion_beat_times"] = [[float(t) / pp.TED_FPS for t in np.nonzero(mask[b])[0]] for b in range(B)]
    res["bc"] = acc.score() if acc.num_beats else float("nan")
    return res
