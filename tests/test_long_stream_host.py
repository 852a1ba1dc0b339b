"""Host side of ``long_form.open_stream``: the windows a push or close runs (ls_long_stream_plan) against a brute-force restatement of
the definition, the ABI of the two new structs, and the refusals raised before an engine exists.  No GPU."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from livelyspeaker_amd import _lib, long_form, synth
from test_long_form_host import _no_engine, _parts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STRIDE = 32000
AUDIO_LENS = (synth.CONFIGS["ted"].audio_len, synth.CONFIGS["beat"].audio_len)


class _Cfg:
    nframes, n_pre_seq = 34, 4

    def __init__(self, audio_len):
        self.audio_len = audio_len


def _done(total, AL):
    """Window w runs when 32000 w + AL <= total: how many have, counted one by one."""
    w = 0
    while STRIDE * w + AL <= total:
        w += 1
    return w


def _brute(before, new, AL, closing):
    first, last = _done(before, AL), _done(before + new, AL)
    if closing:
        last = max(last, long_form.plan_windows(before + new, _Cfg(AL))[0])
    return first, last - first


def test_both_audio_lengths_are_covered():
    assert sorted(AUDIO_LENS) == [36266, 36267]


@pytest.mark.parametrize("AL", AUDIO_LENS)
def test_plan_on_the_named_edges(AL):
    plan = _lib.long_stream_plan
    for total, want in ((AL - 1, 0), (AL, 1), (AL + 1, 1), (AL + STRIDE - 1, 1), (AL + STRIDE, 2), (AL + STRIDE + 1, 2)):
        assert plan(0, total, AL) == (0, want) == _brute(0, total, AL, False), total
        assert plan(total, 0, AL) == (want, 0), total                              # new = 0 runs nothing
        for before in (0, 1, AL - 1, AL):
            if before <= total:
                assert plan(before, total - before, AL) == _brute(before, total - before, AL, False), (before, total)
    assert plan(AL - 1, 1, AL) == (0, 1) and plan(AL, STRIDE - 1, AL) == (1, 0) and plan(AL + STRIDE - 1, 1, AL) == (1, 1)
    assert plan(AL - 1, 1 + 2 * STRIDE, AL) == (0, 3)                              # one chunk completes three windows
    assert plan(5, 3 * STRIDE + AL, AL) == (0, 4)
    # close: what plan_windows(total) still owes; nothing on exactly AL + 32000 m samples
    assert plan(20000, 0, AL, True) == (0, 1)
    for m in range(4):
        assert plan(AL + STRIDE * m, 0, AL, True) == (m + 1, 0)
        assert plan(AL + STRIDE * m + 1, 0, AL, True) == (m + 1, 1)
        assert plan(AL + STRIDE * m - 1, 0, AL, True) == (m, 1)
    assert plan(0, 1, AL, True) == (0, 1)
    with pytest.raises(ValueError):
        plan(0, 0, AL, True)                                                       # a waveform without a sample (plan_windows raises too)
    with pytest.raises(ValueError):
        plan(-1, 5, AL)
    with pytest.raises(ValueError):
        plan(5, -1, AL)


def test_plan_agrees_with_brute_force_on_random_triples():
    rng = np.random.default_rng(20260501)
    n = 0
    for AL in AUDIO_LENS:
        for _ in range(150):
            before = int(rng.integers(0, 8 * STRIDE))
            new = int(rng.choice([0, 1, int(rng.integers(0, 4000)), int(rng.integers(0, 5 * STRIDE))]))
            closing = bool(rng.integers(0, 2)) and before + new >= 1
            assert _lib.long_stream_plan(before, new, AL, closing) == _brute(before, new, AL, closing), (AL, before, new, closing)
            n += 1
    assert n == 300


@pytest.mark.parametrize("AL", AUDIO_LENS)
def test_any_chunking_plus_the_close_runs_plan_windows(AL):
    rng = np.random.default_rng(7)
    for L in (1, 20000, AL - 1, AL, AL + 1, AL + STRIDE, AL + 2 * STRIDE - 5000, int(rng.integers(1, 10 * STRIDE))):
        for pieces in (1, 2, 7, 40):
            cuts = np.sort(rng.integers(0, L + 1, size=pieces - 1))
            sizes = np.diff(np.concatenate([[0], cuts, [L]]))
            fed = ran = 0
            for s in sizes:
                first, k = _lib.long_stream_plan(fed, int(s), AL)
                assert first == ran
                fed, ran = fed + int(s), ran + k
            first, k = _lib.long_stream_plan(fed, 0, AL, True)
            assert first == ran and ran + k == long_form.plan_windows(L, _Cfg(AL))[0], (L, sizes.tolist())


COND_FIELDS = ("batch", "on_device", "seed_poses", "vid_indices", "scale")
PUSH_FIELDS = ("sampler", "noise_mode", "skip_timesteps", "on_device", "use_graph", "clip_denoised", "two_pass_always", "eta", "closing",
               "capacity", "n_samples", "audio", "emo", "sag", "text_features", "x_init", "eps_tape", "noise_tape", "seed", "sample_offset",
               "frames", "n_frames", "n_windows")
NEW_EXPORTS = ("ls_long_stream_plan", "ls_long_stream_open", "ls_long_stream_push", "ls_long_stream_info")


def test_stream_structs_match_the_header_and_the_abi_is_unchanged(tmp_path):
    lib = _lib.load_library()
    assert lib.ls_abi_version() == 5
    hdr = open(os.path.join(ROOT, "include", "ls_hip.h")).read()
    for name in NEW_EXPORTS:
        assert name in _lib.EXPORTS and f"int {name}(" in hdr and hasattr(lib, name), name
    assert [n for n, _ in _lib.LsLongStreamCond._fields_] == list(COND_FIELDS)
    assert [n for n, _ in _lib.LsLongStreamPushArgs._fields_] == list(PUSH_FIELDS)
    prints = "".join(f'    printf("%zu\\n", offsetof(ls_long_stream_cond, {f}));\n' for f in COND_FIELDS)
    prints += "".join(f'    printf("%zu\\n", offsetof(ls_long_stream_push_args, {f}));\n' for f in PUSH_FIELDS)
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "ls_hip.h"\nint main(void) {\n'
                   '    printf("%zu %zu %zu %zu %d\\n", sizeof(ls_long_stream_cond), sizeof(ls_long_stream_push_args), sizeof(ls_long_cond),\n'
                   '           sizeof(ls_long_sample_args), LS_ABI_VERSION);\n' + prints + '    return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got[:5] == [ctypes.sizeof(_lib.LsLongStreamCond), ctypes.sizeof(_lib.LsLongStreamPushArgs), 64, 104, 5]
    nc = len(COND_FIELDS)
    assert got[5:5 + nc] == [getattr(_lib.LsLongStreamCond, f).offset for f in COND_FIELDS]
    assert got[5 + nc:] == [getattr(_lib.LsLongStreamPushArgs, f).offset for f in PUSH_FIELDS]
    assert ctypes.sizeof(_lib.LsLongCond) == 64 and ctypes.sizeof(_lib.LsLongSampleArgs) == 104
    for name in ("long_stream_open", "long_stream_push", "long_stream_info"):
        assert hasattr(_lib.Engine, name)


@pytest.mark.parametrize("ds", ["ted", "beat"])
def test_stream_refusals_come_before_any_engine(ds, monkeypatch):
    _no_engine(monkeypatch)
    cfg, model, diffusion = _parts(ds)
    B = 2
    y = synth.make_long_cond(cfg, B, 2)
    emo = {"emo": y["emo"][:, 0]} if ds == "beat" else {}

    def open_(model=model, **kw):
        return long_form.open_stream(diffusion, model, y["seed_poses"], y["vid_indices"], y["scale"], **{**emo, **kw})

    with pytest.raises(TypeError):
        open_(model=model.model)                                            # the bare RAG, not the CFG wrapper
    with pytest.raises(ValueError):
        open_(sampler="plms")
    with pytest.raises(ValueError):
        open_(skip_timesteps=diffusion.num_timesteps)
    with pytest.raises(ValueError):
        long_form.open_stream(diffusion, model, y["seed_poses"][:, :-1], y["vid_indices"], y["scale"], **emo)
    with pytest.raises(ValueError):
        long_form.open_stream(diffusion, model, y["seed_poses"], y["vid_indices"][:1], y["scale"], **emo)
    diffusion.noise_source = "torch_device"
    with pytest.raises(NotImplementedError):
        open_()
    diffusion.noise_source = "torch_cpu"
    if ds == "ted":
        with pytest.raises(ValueError, match="BEAT"):
            open_(emo=np.zeros(B, np.int64))
    else:
        with pytest.raises(ValueError, match="emo"):
            open_(emo=y["emo"])                                             # [B, W]: a stream holds one id per clip

    st = open_()                                                            # opening touches no engine
    assert (st.samples_in, st.windows_run, st.frames_out) == (0, 0, 0)
    for bad in (np.zeros(100, np.float32), np.zeros((B, 10, 1), np.float32), np.zeros((B + 1, 100), np.float32)):
        with pytest.raises(ValueError, match="audio_chunk"):
            st.push(bad)
    with pytest.raises(ValueError, match="text_features without sag"):
        st.push(np.zeros((B, 100), np.float32), text_features=np.zeros((B, 512), np.float32))
    if ds == "beat":
        with pytest.raises(ValueError, match="emo"):
            st.push(np.zeros((B, 100), np.float32), emo=np.zeros(B + 1, np.int64))
        bare = long_form.open_stream(diffusion, model, y["seed_poses"], y["vid_indices"], y["scale"])     # legal: emo may come with a push
        with pytest.raises(ValueError, match="first window"):
            bare.push(np.zeros((B, cfg.audio_len), np.float32))            # ... but the first window needs one
        with pytest.raises(ValueError):
            bare.close()                                                    # a stream without a sample has no window to close on
    else:
        with pytest.raises(ValueError, match="BEAT"):
            st.push(np.zeros((B, 100), np.float32), emo=np.zeros(B, np.int64))
    assert (st.samples_in, st.windows_run, st.frames_out) == (0, 0, 0)     # a refused push feeds nothing
    with open_() as inside:
        assert inside is not None
    with pytest.raises(RuntimeError, match="closed"):
        inside.push(np.zeros((B, 100), np.float32))                         # after close, a push raises
    with pytest.raises(RuntimeError, match="closed"):
        inside.close()
