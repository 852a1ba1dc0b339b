"""The score stream, host side: the plan of the audio frames a push decides (ls_score_stream_plan) against its definition, the plan's
unit under the host sanitizers (tests/score_plan_main.cpp, a stand-alone program), the ABI of the three new structs, the refusals of
open / push / finish ahead of any device call, and the Python surface's argument errors.  No GPU."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from livelyspeaker_amd import _lib, build, long_form, postprocess as pp
from test_long_form_host import _no_engine, _parts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENGTHS = (1, 511, 512, 1023, 1024, 1025, 1536, 36267, 2103486)
MOST = 2 ** 31 - 2048


def decided(pad, n):
    """The definition: frame f once samples >= 512 f + 1024, and under reflect padding once samples >= 1025."""
    f = 0
    while n >= 512 * f + 1024 and (pad == "constant" or n >= 1025):
        f += 1
    return f


@pytest.mark.parametrize("pad", ["constant", "reflect"])
@pytest.mark.parametrize("L", LENGTHS)
def test_plan_tiles_the_frames_once_and_in_order(L, pad):
    rng = np.random.default_rng(L)
    for trial in range(4):
        cuts = np.sort(rng.integers(0, L + 1, size=int(rng.integers(0, 12))))
        if trial == 3:                                                          # empty pushes among them
            cuts = np.sort(np.concatenate([cuts, cuts[:3]]))
        edges = np.concatenate([[0], cuts, [L]])
        n = nxt = 0
        for a, b in zip(edges[:-1], edges[1:]):
            first, count = pp.score_stream_plan(n, int(b - a), False, pad)
            assert first == nxt and count >= 0
            n, nxt = int(b), nxt + count
            if L < 100000:
                assert nxt == decided(pad, n)                                   # no frame before its rule allows, none later
            elif count:
                assert n >= 512 * (nxt - 1) + 1024 and n < 512 * nxt + 1024
        if pad == "reflect" and L <= 1024:
            with pytest.raises(ValueError):
                pp.score_stream_plan(L, 0, True, pad)
            continue
        first, count = pp.score_stream_plan(L, 0, True, pad)
        assert first == nxt and first + count == 1 + L // 512


def test_plan_refusals():
    lib = _lib.load_library()
    first, count = ctypes.c_int64(), ctypes.c_int32()

    def rc(pad, before, new, fin, f=first, c=count):
        return lib.ls_score_stream_plan(pad, before, new, fin, ctypes.byref(f) if f is not None else None, ctypes.byref(c) if c is not None else None)

    assert rc(0, 0, 1024, 0) == 0 and (first.value, count.value) == (0, 1)
    assert rc(0, -1, 5, 0) == -1 and rc(0, 5, -1, 0) == -1                      # negative counts
    assert rc(0, MOST, 0, 0) == 0 and rc(0, MOST, 1, 0) == -1 and rc(0, 0, MOST + 1, 0) == -1      # a total above 2^31 - 2048
    assert rc(0, 0, 0, 1) == -1 and rc(1, 0, 0, 1) == -1                        # finishing an empty series
    assert rc(1, 1024, 0, 1) == -1 and rc(1, 1000, 24, 1) == -1 and rc(1, 1025, 0, 1) == 0          # reflect and L <= 1024
    assert rc(0, 1024, 0, 1) == 0 and rc(0, 1, 0, 1) == 0
    assert rc(2, 0, 5, 0) == -1 and rc(-1, 0, 5, 0) == -1
    assert rc(0, 0, 5, 0, f=None) == -1 and rc(0, 0, 5, 0, c=None) == -1
    with pytest.raises(ValueError, match="pad_mode"):
        pp.score_stream_plan(0, 5, pad_mode="edge")
    with pytest.raises(ValueError):
        pp.score_stream_plan(0, 0, True)


def test_plan_on_its_edges_under_asan_and_ubsan(tmp_path):
    """tests/score_plan_main.cpp with the plan's unit, as plain C++ with the host sanitizers linked statically: a child process of its
    own, nothing preloaded, nothing inside Python, no GPU."""
    exe = str(tmp_path / "score_plan")
    made = subprocess.run([build.hipcc_path(), "-x", "c++", "-std=c++17", "-O1", "-g", "-fno-gpu-sanitize", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "score_plan_main.cpp"),
                           os.path.join(ROOT, "livelyspeaker_amd", "csrc", "ls_score_plan.cpp"), "-o", exe], capture_output=True, text=True)
    assert made.returncode == 0, made.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr
    assert run.stderr == "", run.stderr


STRUCTS = (("ls_score_config", _lib.LsScoreConfig), ("ls_score_stream_push_args", _lib.LsScoreStreamPushArgs),
           ("ls_score_stream_outputs", _lib.LsScoreStreamOutputs))
NEW_EXPORTS = ("ls_score_stream_plan", "ls_score_stream_open", "ls_score_stream_push", "ls_score_stream_finish", "ls_score_stream_info",
               "ls_score_stream_close", "ls_score_stream_last_error")


def test_abi_mirrors(tmp_path):
    lines = []
    for cname, cls in STRUCTS:
        lines.append(f'    printf("%zu", sizeof({cname}));\n')
        lines += [f'    printf(" %zu", offsetof({cname}, {n}));\n' for n, _ in cls._fields_]
        lines.append('    printf("\\n");\n')
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ls_hip.h"\nint main(void) {\n' + "".join(lines) +
                   '    printf("%d %d %d\\n", LS_ABI_VERSION, LS_SCORE_TILE, LS_SCORE_STREAM_MAX_BEATS);\n    return 0;\n}\n')
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [[int(v) for v in line.split()] for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()]
    for row, (cname, cls) in zip(got, STRUCTS):
        assert row == [ctypes.sizeof(cls)] + [getattr(cls, n).offset for n, _ in cls._fields_], cname
    from livelyspeaker_amd import audio_onsets as ao
    assert got[3] == [5, ao.SCORE_TILE, _lib.SCORE_STREAM_MAX_BEATS]
    hdr = open(os.path.join(ROOT, "include", "ls_hip.h")).read()
    lib = ctypes.CDLL(_lib.library_path())
    for name in NEW_EXPORTS:
        assert name in _lib.EXPORTS and re.search(rf"\b{name}\s*\(", hdr) and hasattr(lib, name), name
        assert re.fullmatch(r"[a-z_]+", name)
    for src_name in ("ls_score_stream.hip", "ls_score_stream_api.cpp", "ls_score_plan.cpp", "ls_onsets_long.hip"):
        assert src_name in build.SOURCES


def good_config():
    c = _lib.LsScoreConfig()
    c.sr, c.sr_pick, c.pad_mode, c.fmax, c.delta, c.hop, c.onset_source, c.max_chunk = 16000.0, 16000.0, 0, 11025.0, 0.07, 512, 0, 4096
    c.fps, c.sigma, c.time_rate = 15.0, 0.1, 22050.0
    return c


def test_open_refuses_ahead_of_any_device_call():
    lib = _lib.load_library()
    h = ctypes.c_void_p()

    def rc(dataset=0, capacity=2, frames=100, beats=50, out=h, **kw):
        c = good_config()
        for k, v in kw.items():
            setattr(c, k, v)
        return lib.ls_score_stream_open(0, dataset, capacity, frames, beats, ctypes.byref(c), ctypes.byref(out) if out is not None else None)

    assert lib.ls_score_stream_open(0, 0, 2, 100, 50, None, ctypes.byref(h)) == -1 and rc(out=None) == -1
    assert rc(dataset=2) == -1 and rc(dataset=-1) == -1 and rc(capacity=0) == -1
    assert rc(frames=0) == -1 and rc(frames=2 ** 22 - 2) == -1 and rc(beats=-1) == -1
    for bad in (dict(sr=0.0), dict(sr_pick=0.0), dict(pad_mode=2), dict(fmax=0.0), dict(hop=0), dict(onset_source=3), dict(onset_source=-1),
                dict(max_chunk=0), dict(fps=0.0), dict(sigma=0.0), dict(time_rate=0.0)):
        assert rc(**bad) == -1, bad
        assert lib.ls_score_stream_last_error(None).decode().startswith("ls_score_stream_open")
    assert not h.value
    assert lib.ls_score_stream_push(None, None) == -1 and lib.ls_score_stream_finish(None, None, None) == -1
    assert lib.ls_score_stream_info(None, None, None, None, None) == -1
    lib.ls_score_stream_close(None)


def test_every_refusal_sits_in_front_of_the_device():
    """In the three entries no line that returns LS_EINVAL or LS_ESTATE follows a HIP call: the device work lives in helpers
    (allocate, push, finish) that the entries call once every check has passed."""
    src = open(os.path.join(ROOT, "livelyspeaker_amd", "csrc", "ls_score_stream_api.cpp")).read()
    for entry, helper in (("int ls_score_stream_open(", "allocate(h)"), ("int ls_score_stream_push(", "push(h, a,"),
                          ("int ls_score_stream_finish(", "finish(h, counts")):
        body = src[src.index(entry):]
        body = body[:body.index("\n}\n")]
        head, tail = body[:body.index(helper)], body[body.index(helper):]
        assert "LS_EINVAL" not in tail and "LS_ESTATE" not in tail, entry
        hip_calls = [c for c in re.findall(r"\bhip[A-Z]\w+", head) if c != "hipGetDeviceCount" and c != "hipSuccess"]
        assert not hip_calls, (entry, hip_calls)
    for helper in ("int allocate(H* h)", "int push(H* h", "int finish_slot(H* h", "int finish(H* h"):
        body = src[src.index(helper):]
        body = body[:body.index("\n}\n")]
        assert "LS_EINVAL" not in body and "LS_ESTATE" not in body, helper


def test_python_surface_refuses_before_a_device_is_touched(monkeypatch):
    monkeypatch.setattr(_lib, "ScoreStreamEngine", lambda *a, **k: (_ for _ in ()).throw(AssertionError("an engine was opened")))
    for bad in (dict(dataset="tedx"), dict(capacity=0), dict(max_seconds=0.0), dict(pad_mode="edge"), dict(want=("onsets",)),
                dict(onset_source="raw"), dict(align_series=6), dict(max_chunk=0), dict(sigma=0.0), dict(max_seconds=2.0 ** 31)):
        kw = dict(dataset="ted", capacity=2, max_seconds=5.0)
        kw.update(bad)
        with pytest.raises(ValueError):
            pp.open_score_stream(**kw)
    ss = pp.open_score_stream("ted", 2, 5.0)
    assert (ss.max_audio_frames, ss.max_beat_entries, ss.max_samples) == (1 + 80000 // 512, 76, 80000)
    assert ss.frames_in.tolist() == [0, 0] and ss.samples_in.tolist() == [0, 0]
    with pytest.raises(ValueError, match="audio, beats"):
        ss.push()
    with pytest.raises(ValueError, match="max_chunk"):
        ss.push(audio=np.zeros((2, 65537), np.float32))
    with pytest.raises(ValueError):
        ss.push(audio=np.zeros((3, 100), np.float32))
    with pytest.raises(ValueError, match="lengths"):
        ss.push(audio=np.zeros((2, 100), np.float32), lengths=[100, 101])
    with pytest.raises(ValueError, match="lengths"):
        ss.push(lengths=[1, 1], beats={"beat_mask": np.zeros((2, 0), bool), "beat_first": [0, 0], "beat_count": [0, 0]})
    with pytest.raises(ValueError, match="max_seconds"):                        # more audio than the slot was opened for
        ss._samples[:] = 60000
        ss.push(audio=np.zeros((2, 30000), np.float32))
    ss._samples[:] = 0
    beats = {"beat_mask": np.zeros((2, 4), bool), "beat_first": [0, 3], "beat_count": [2, 2]}
    with pytest.raises(ValueError, match="starts at 3"):
        ss.push(beats=beats)
    with pytest.raises(ValueError, match="beat_count"):
        ss.push(beats=dict(beats, beat_first=[0, 0], beat_count=[2, 5]))
    ss._beats[:] = 75
    with pytest.raises(ValueError, match="max_seconds"):
        ss.push(beats=dict(beats, beat_first=[75, 75]))
    ss._beats[:] = 0
    with pytest.raises(ValueError, match="no audio"):
        ss.finish(0)
    with pytest.raises(ValueError, match="no audio"):
        ss.finish(2)
    assert ss.close() == {}
    with pytest.raises(RuntimeError):
        ss.push(audio=np.zeros((2, 10), np.float32))
    with pytest.raises(ValueError, match="6"):
        pp.open_score_stream("beat", 1, 5.0).push(beats={"beat_mask": np.zeros((1, 4), bool), "beat_first": [0], "beat_count": [1]})
    bc = pp.BeatConsistency()
    with pytest.raises(ValueError, match="finish dict"):
        bc.push_score({"align": 0.5})
    bc.push_score({})
    bc.push_score({"align_sum": 1.5, "n_beats": 2, "count": 4})
    bc.push_score({0: {"align_sum": 9.0, "n_beats": 0, "count": 7}, 1: {"align_sum": 0.5, "n_beats": 1, "count": 1}})
    assert (bc.align_sum, bc.num_beats, bc.motion_beats_sum) == (11.0, 5, 3)


@pytest.mark.parametrize("ds", ["ted", "beat"])
def test_sessions_refuse_score_without_post(ds, monkeypatch):
    _no_engine(monkeypatch)
    cfg, model, diffusion = _parts(ds)
    from livelyspeaker_amd import synth
    y = synth.make_long_cond(cfg, 2, 2)
    emo = y.get("emo")
    emo = None if emo is None else emo[:, 0]
    args = (diffusion, model, y["seed_poses"], y["vid_indices"], y["scale"])
    with pytest.raises(ValueError, match="post="):
        long_form.open_stream(*args, emo=emo, score=True, max_seconds=60)
    with pytest.raises(ValueError, match="max_seconds"):
        long_form.open_stream(*args, emo=emo, post=ds, score=True)
    with pytest.raises(ValueError, match="score"):
        long_form.open_stream(*args, emo=emo, post=ds, max_seconds=60)
    with pytest.raises(ValueError, match="score must"):
        long_form.open_stream(*args, emo=emo, post=ds, score="yes", max_seconds=60)
    with pytest.raises(ValueError, match="pad_mode"):
        long_form.open_stream(*args, emo=emo, post=ds, score={"pad_mode": "edge"}, max_seconds=60)
    with pytest.raises(ValueError, match="post="):
        long_form.open_pool(diffusion, model, 2, score=True, max_seconds=60)
    with pytest.raises(ValueError, match="max_seconds"):
        long_form.open_pool(diffusion, model, 2, post=ds, score=True)
    st = long_form.open_stream(*args, emo=emo, post=ds, score=True, max_seconds=60)
    assert st._score is not None and st._score.capacity == 2 and st._score.dataset == ds
    assert long_form.open_stream(*args, emo=emo, post=ds)._score is None
    pool = long_form.open_pool(diffusion, model, 3, post=ds, score={"delta": 0.1}, max_seconds=30)
    assert pool._score.capacity == 3 and abs(pool._score._cfg.delta - 0.1) < 1e-7


def test_score_talk_refuses_bad_arguments():
    t = np.zeros((2, 9, 3, 40), np.float32)
    y = np.zeros((2, 4000), np.float32)
    with pytest.raises(ValueError, match="dataset"):
        long_form.score_talk(t, y, dataset="tedx")
    with pytest.raises(ValueError, match="timeline"):
        long_form.score_talk(t[0], y)
    with pytest.raises(ValueError, match="audio"):
        long_form.score_talk(t, y[:1])
    with pytest.raises(ValueError, match="frames"):
        long_form.score_talk(t, y, frames=[40, 41])
    with pytest.raises(ValueError, match="audio_lengths"):
        long_form.score_talk(t, y, audio_lengths=[4000, 0])
