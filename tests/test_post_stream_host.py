"""Host side of ``postprocess.open_post_stream``: the beat entries a push decides (ls_post_stream_plan) against a brute-force restatement
written here, the ABI of the new struct and entries, the refusals that come before a device is touched, and
tests/post_stream_plan_main.cpp -- a stand-alone program around the plan unit -- under the host sanitizers.  No GPU."""
import ctypes
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

from livelyspeaker_amd import _lib, build, long_form, postprocess as pp
from test_long_form_host import _no_engine, _parts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ls_post_stream_plan", "ls_post_stream_check", "ls_post_stream_open", "ls_post_stream_push", "ls_post_stream_info")
PUSH_FIELDS = ("on_device", "K", "beat_capacity", "reserved", "frames", "counts", "finish", "aligned", "pose", "angle_diff", "decoded",
               "euler_deg", "beat_mask", "beat_first", "beat_count")


def _decidable(dataset, order, n, final):
    """Brute force: the entries of a series that holds n frames which no continuation can change.  TED: the beat at frame f reads
    angle_diff[f - 1 .. f + 1], so frames f - 2 .. f + 1, and lies in [2, N - 2]: known once frame f + 1 exists, or the series has
    ended.  BEAT: the minimum at velocity f reads v[f - order .. f + order] (clamped to the series), v[i] frames i and i + 1: known
    once frame f + order + 1 exists, or the series has ended (V = n - 1 velocities)."""
    if dataset == "ted":
        return [f for f in range(n) if final or f + 1 <= n - 1]
    return [f for f in range(max(n - 1, 0)) if final or f + order + 1 <= n - 1]


def _splits(N):
    """Every split of N frames into chunks from {0, 1, 2, 3, N}, with at most one idle push in a row (more add nothing)."""
    def rec(left, prev_zero):
        if left == 0:
            yield ()
            return
        for c in (0, 1, 2, 3, N):
            if c > left or (c == 0 and prev_zero):
                continue
            for rest in rec(left - c, c == 0):
                yield (c,) + rest
    return rec(N, False)


@pytest.mark.parametrize("dataset,order", [("ted", 1)] + [("beat", o) for o in (1, 2, 3, 4, 8)])
def test_plan_agrees_with_the_restatement_on_every_step_a_split_can_take(dataset, order):
    """The plan of a push depends on (frames before, new frames, finishing) alone, so EVERY split of N frames into chunks from
    {0, 1, 2, 3, N} is a path through the steps checked here -- all of them, for every N of the issue, 40 included, where the splits
    themselves are too many to walk (the test below walks them for N <= 9 and samples them above)."""
    for N in sorted({1, 2, 3, 4, 5, 2 * order + 1, 2 * order + 2, 40}):
        for n in range(N + 1):
            before = set(_decidable(dataset, order, n, False))
            for c in (0, 1, 2, 3, N):
                if n + c > N:
                    continue
                for last in (False, True) if n + c == N else (False,):
                    first, count = pp.post_stream_plan(dataset, n, c, last, order)
                    want = [f for f in _decidable(dataset, order, n + c, last) if f not in before]
                    assert list(range(first, first + count)) == want, (N, n, c, last)
                    assert first == len(before)                          # the ranges follow one another: no gap, no overlap


@pytest.mark.parametrize("dataset,order", [("ted", 1)] + [("beat", o) for o in (1, 2, 3, 4, 8)])
def test_plan_tiles_the_series_once_in_order_under_every_split(dataset, order):
    sizes = sorted({1, 2, 3, 4, 5, 2 * order + 1, 2 * order + 2, 40})
    for N in sizes:
        total = N if dataset == "ted" else N - 1
        splits = _splits(N) if N <= 9 else itertools.chain(
            [(N,), (1,) * N, (3,) * (N // 3) + (1,) * (N % 3), (0, 2) * (N // 2) + (1,) * (N % 2)],
            (tuple(int(c) for c in np.random.default_rng(N + k).choice([0, 1, 2, 3], 4 * N)) for k in range(40)))
        for split in splits:
            if sum(split) > N:                                          # a random draw: cut to N frames
                cut, acc = [], 0
                for c in split:
                    c = min(c, N - acc)
                    cut.append(c)
                    acc += c
                    if acc == N:
                        break
                split = tuple(cut)
            if sum(split) != N:
                continue
            for finish_alone in (False, True):
                n, seen = 0, []
                for i, c in enumerate(split):
                    last = i == len(split) - 1 and not finish_alone
                    first, count = pp.post_stream_plan(dataset, n, c, last, order)
                    want = [f for f in _decidable(dataset, order, n + c, last) if f not in set(_decidable(dataset, order, n, False))]
                    assert list(range(first, first + count)) == want, (N, split, i)
                    seen += want
                    n += c
                if finish_alone:
                    first, count = pp.post_stream_plan(dataset, n, 0, True, order)
                    seen += list(range(first, first + count))
                    assert count <= (1 if dataset == "ted" else order)
                assert seen == list(range(total)), (N, split, finish_alone)


def test_plan_refusals():
    for bad in (("ted", -1, 1), ("ted", 1, -1), ("ted", 0, 0, True), ("beat", 0, 1, False, 0), ("beat", 0, 1, False, 9), ("g", 0, 1)):
        with pytest.raises(ValueError):
            pp.post_stream_plan(*bad)
    assert pp.post_stream_plan("ted", 0, 0) == (0, 0) and pp.post_stream_plan("beat", 3, 0, True, 8) == (0, 2)


def test_struct_layout_and_exports_match_the_header(tmp_path):
    hdr = open(os.path.join(ROOT, "include", "ls_hip.h")).read()
    lib = ctypes.CDLL(_lib.library_path())
    for name in NAMES:
        assert name in _lib.EXPORTS and re.search(rf"\bint {name}\s*\(", hdr) and hasattr(lib, name), name
    assert "ls_post_stream_close" in _lib.EXPORTS and re.search(r"\bvoid ls_post_stream_close\s*\(", hdr) and hasattr(lib, "ls_post_stream_close")
    lib.ls_abi_version.restype = ctypes.c_int
    assert lib.ls_abi_version() == 5
    A = _lib.LsPostStreamPushArgs
    assert [n for n, _ in A._fields_] == list(PUSH_FIELDS)
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ls_hip.h"\nint main(void) {\n'
                   '    printf("%zu", sizeof(ls_post_stream_push_args));\n' +
                   "".join(f'    printf(" %zu", offsetof(ls_post_stream_push_args, {n}));\n' for n in PUSH_FIELDS) +
                   '    printf(" %d %d %d %zu %zu\\n", LS_ABI_VERSION, LS_POST_STREAM_MAX_CHUNK, LS_POST_STREAM_MAX_ORDER, sizeof(ls_post_config),\n'
                   '           sizeof(ls_ted_align_args));\n    return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [ctypes.sizeof(A)] + [getattr(A, n).offset for n in PUSH_FIELDS] + [
        5, pp.POST_STREAM_MAX_CHUNK, _lib.POST_STREAM_MAX_ORDER, ctypes.sizeof(_lib.LsPostConfig), ctypes.sizeof(_lib.LsTedAlignArgs)]
    assert pp.POST_STREAM_MAX_CHUNK == 256


def test_every_refusal_returns_before_a_device_is_touched():
    """ls_post_stream_check is the check a push runs ahead of any launch; ls_post_stream_open's own refusals sit in front of its first
    HIP call.  -1 is LS_EINVAL, -2 LS_ESTATE; reaching the device without a GPU would give LS_EHIP (-3)."""
    lib = _lib.load_library()
    i64 = lambda v: np.array(v, np.int64)       # noqa: E731
    i32 = lambda v: np.array(v, np.int32)       # noqa: E731
    p64 = lambda a: a.ctypes.data_as(_lib.c_i64p) if a is not None else None      # noqa: E731
    p32 = lambda a: a.ctypes.data_as(_lib.c_i32p) if a is not None else None      # noqa: E731

    def check(dataset=0, order=1, n=(0, 5), K=4, counts=(4, 0), finish=None, cap=8):
        n, counts, finish = i64(n), None if counts is None else i32(counts), None if finish is None else i32(finish)
        return lib.ls_post_stream_check(dataset, order, len(n), p64(n), K, p32(counts), p32(finish), cap, None, None)

    assert check() == 0
    assert check(counts=None) == -1                                       # null counts
    assert check(counts=(-1, 0)) == -1                                    # negative counts
    assert check(counts=(5, 0)) == -1                                     # counts[s] > K
    assert check(K=257, counts=(257, 0), cap=600) == -1                   # a chunk over the cap
    assert check(K=256, counts=(256, 0), cap=600) == 0
    for order in (0, 9, -1):
        assert check(dataset=1, order=order) == -1                        # order outside 1..8
    assert check(dataset=1, order=8) == 0
    assert check(cap=2) == -1 and check(cap=3) == 0                       # beat_capacity too small: slot 0 decides frames [0, 3)
    assert check(finish=(0, 1), cap=3) == 0 and check(finish=(0, 1), counts=(4, 3), cap=3) == -1      # ... slot 1: [4, 8) at the finish
    assert check(n=(0, 0), counts=(4, 0), finish=(0, 1)) == -2            # finish on a slot with no frames
    assert check(n=(0, 0), counts=(4, 1), finish=(0, 1)) == 0

    cfg = pp.ted_post_config()
    joints = (ctypes.c_int32 * 6)(4, 3, 5, 26, 25, 27)
    h = ctypes.c_void_p()
    op = lambda ds, S, c, J, o, sj, out=h: lib.ls_post_stream_open(0, ds, S, ctypes.byref(c) if c else None, J, o, sj,      # noqa: E731
                                                                  ctypes.byref(out) if out is not None else None)
    assert op(0, 2, cfg, 0, 0, None, out=None) == -1
    assert op(2, 2, cfg, 0, 0, None) == -1 and op(0, 0, cfg, 0, 0, None) == -1 and op(0, 2, None, 0, 0, None) == -1
    bad = pp.ted_post_config()
    bad.njoints = 17
    assert op(0, 2, bad, 0, 0, None) == -1                                # what ls_ted_post refuses
    for order in (0, 9):
        assert op(1, 2, None, 47, order, joints) == -1
    assert op(1, 2, None, 0, 2, joints) == -1 and op(1, 2, None, 27, 2, joints) == -1 and op(1, 2, None, 47, 2, None) == -1
    assert not h.value and b"ls_post_stream_open" in lib.ls_post_stream_last_error(None)
    assert lib.ls_post_stream_push(None, None) == -1 and lib.ls_post_stream_info(None, None, None) == -1
    lib.ls_post_stream_close(None)


def test_python_refusals_come_before_the_handle_exists():
    for bad in (dict(dataset="g"), dict(capacity=0), dict(dataset="beat", order=0), dict(dataset="beat", order=9),
                dict(dataset="beat", series_joints=(0, 1, 2)), dict(dataset="beat", joints=5)):
        kw = dict(dataset="ted", capacity=2)
        kw.update(bad)
        with pytest.raises(ValueError):
            pp.open_post_stream(**kw)
    ps = pp.open_post_stream("ted", 2)
    assert ps.frames_in.tolist() == [0, 0] and ps._eng is None
    z = lambda K, F=3: np.zeros((2, 9, F, K), np.float32)      # noqa: E731
    with pytest.raises(ValueError, match="frames must be"):
        ps.push(z(4, 6))
    with pytest.raises(ValueError, match="256"):
        ps.push(z(257))
    with pytest.raises(ValueError, match="counts"):
        ps.push(z(4), [5, 0])
    with pytest.raises(ValueError, match="counts"):
        ps.push(z(4), [-1, 0])
    with pytest.raises(ValueError, match="one count"):
        ps.push(z(4), [1])
    with pytest.raises(ValueError, match="without a frame"):
        ps.push(z(4), [4, 0], [False, True])
    with pytest.raises(ValueError, match="no running series"):
        ps.finish(0)
    assert ps._eng is None and ps.close() is None
    with pytest.raises(RuntimeError, match="closed"):
        ps.push(z(4))
    beat = pp.open_post_stream("beat", 1, order=3, joints=5, series_joints=(0, 1, 2, 3, 4, 2))
    with pytest.raises(ValueError, match="frames must be"):
        beat.push(np.zeros((1, 5, 3, 4), np.float32))


@pytest.mark.parametrize("ds", ["ted", "beat"])
def test_sessions_check_post_against_the_model(ds, monkeypatch):
    _no_engine(monkeypatch)
    cfg, model, diffusion = _parts(ds)
    other = "beat" if ds == "ted" else "ted"
    for bad in (other, "euler", True):
        with pytest.raises(ValueError, match="post"):
            long_form.open_pool(diffusion, model, 2, post=bad)
    pool = long_form.open_pool(diffusion, model, 2, post=ds)
    assert pool._post is None and pool._post_kind == ds
    with pool:
        pass
    res = long_form.open_pool(diffusion, model, 2, post=ds).close()
    assert len(res) == 3 and res[2] is None and res[1].tolist() == [0, 0]      # nothing was ever fed: no engine, no post-processing
    assert len(long_form.open_pool(diffusion, model, 2).close()) == 2


def test_post_stream_plan_on_its_edges_under_asan_and_ubsan(tmp_path):
    """tests/post_stream_plan_main.cpp with the plan's unit, as plain C++ with the host sanitizers linked statically: a child process of
    its own, nothing preloaded, nothing inside Python, no GPU."""
    exe = str(tmp_path / "post_stream_plan")
    made = subprocess.run([build.hipcc_path(), "-x", "c++", "-std=c++17", "-O1", "-g", "-fno-gpu-sanitize", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "post_stream_plan_main.cpp"),
                           os.path.join(ROOT, "livelyspeaker_amd", "csrc", "ls_post_stream_plan.cpp"), "-o", exe], capture_output=True, text=True)
    assert made.returncode == 0, made.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr
    assert run.stderr == "", run.stderr
