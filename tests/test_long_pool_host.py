"""Host side of ``long_form.open_pool``: the rounds a push runs (ls_long_pool_plan) against a restatement of the definition written
here, slot by slot against ``_lib.long_stream_plan``, the ABI of the two new structs, the refusals raised before an engine exists, and
tests/pool_plan_main.cpp -- a stand-alone program around the plan -- under the host sanitizers.  No GPU."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from livelyspeaker_amd import _lib, build, long_form, synth
from test_long_form_host import _no_engine, _parts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STRIDE = 32000
AUDIO_LENS = (synth.CONFIGS["ted"].audio_len, synth.CONFIGS["beat"].audio_len)


class _Cfg:
    nframes, n_pre_seq = 34, 4

    def __init__(self, audio_len):
        self.audio_len = audio_len


def _restated(fed, ran, new, closing, open_, AL):
    """The definition, restated: a window w of slot s is complete when 32000 w + AL <= fed + new; a closing slot also owes the windows
    that cover its total; round r holds, ascending, the open slots with more than r windows to run."""
    owed = []
    for f, r, n, c, o in zip(fed, ran, new, closing, open_):
        done = 0
        while STRIDE * done + AL <= f + n:
            done += 1
        last = max(done, long_form.plan_windows(f + n, _Cfg(AL))[0]) if (c and o) else done
        owed.append(last - r if o else 0)
    rounds = [[s for s, k in enumerate(owed) if k > r] for r in range(max(owed))]
    frames = [30 * k + (4 if k and r == 0 else 0) for k, r in zip(owed, ran)]
    return rounds, frames


def staggered(AL):
    """The staggered schedule of the issue as (event, payload) pairs: speakers A (slot 0), B (1), C (3, leaving a gap at 2), D (1 again).
    ``push`` payloads are per-slot lengths; the rounds it must give stand beside it."""
    return [("join", ("A", None)), ("join", ("B", None)),
            ("push", ([AL, AL - 1, 0, 0], [[0]])),
            ("join", ("C", 3)),
            ("push", ([STRIDE, 7001, 0, AL + STRIDE], [[0, 1, 3], [3]])),
            ("leave", ("B", [[1]])),
            ("join", ("D", None)),
            ("push", ([0, AL, 0, STRIDE], [[1, 3]])),
            ("close", [])]


class HostPool:
    """The pool's counters, kept on the host: what ``LongPool.slots`` reports after the same events."""

    def __init__(self, S, AL):
        self.S, self.AL = S, AL
        self.fed, self.ran, self.open = np.zeros(S, np.int64), np.zeros(S, np.int64), np.zeros(S, bool)

    def join(self, slot=None):
        slot = int(np.nonzero(~self.open)[0][0]) if slot is None else slot
        assert not self.open[slot]
        self.fed[slot] = self.ran[slot] = 0
        self.open[slot] = True
        return slot

    def push(self, new, closing=None):
        closing = np.zeros(self.S, np.int32) if closing is None else np.asarray(closing, np.int32)
        rounds, frames = _lib.long_pool_plan(self.fed, self.ran, new, closing, self.open, self.AL)
        assert (rounds, frames.tolist()) == _restated(self.fed, self.ran, new, closing, self.open, self.AL)
        for s in range(self.S):                         # per slot: the stream's plan on that slot alone
            if self.open[s]:
                first, k = _lib.long_stream_plan(int(self.fed[s]), int(new[s]), self.AL, bool(closing[s]))
                assert first == self.ran[s] and k == sum(s in r for r in rounds), s
        self.fed += np.asarray(new, np.int64)
        for r in rounds:
            self.ran[r] += 1
        self.open &= ~(closing.astype(bool))
        return rounds, frames


@pytest.mark.parametrize("AL", AUDIO_LENS)
def test_the_staggered_schedule_runs_the_rounds_the_issue_names(AL):
    pool, slot_of = HostPool(4, AL), {}
    for event, payload in staggered(AL):
        if event == "join":
            slot_of[payload[0]] = pool.join(payload[1])
        elif event == "push":
            rounds, frames = pool.push(payload[0])
            assert rounds == payload[1]
        elif event == "leave":
            closing = np.zeros(4, np.int32)
            closing[slot_of[payload[0]]] = 1
            rounds, frames = pool.push(np.zeros(4, np.int64), closing)
            assert rounds == payload[1] and frames.tolist() == [0, 30, 0, 0]
        else:
            rounds, frames = pool.push(np.zeros(4, np.int64), pool.open.astype(np.int32))
            assert rounds == payload
    assert slot_of == {"A": 0, "B": 1, "C": 3, "D": 1} and not pool.open.any()
    # A was fed AL + 32000 (two windows), D AL (one), C AL + 2 * 32000 (three): all end on a window's last sample, the close owes nothing
    assert pool.ran.tolist() == [2, 1, 0, 3] and pool.fed.tolist() == [AL + STRIDE, AL, 0, AL + 2 * STRIDE]


@pytest.mark.parametrize("AL", AUDIO_LENS)
def test_plan_cases(AL):
    plan = lambda *a: (lambda r, f: (r, f.tolist()))(*_lib.long_pool_plan(*a, AL))      # noqa: E731
    one = [1]
    # two windows in one push
    assert plan([0], [0], [AL + STRIDE], [0], one) == ([[0], [0]], [64])
    assert plan([AL - 1, 0], [0, 0], [1 + STRIDE, AL], [0, 0], [1, 1]) == ([[0, 1], [0]], [64, 34])
    # a closing slot with a padded window; one that ends exactly on audio_len + 32000 m gets no frame and still leaves
    assert plan([AL + 5], [1], [0], [1], one) == ([[0]], [30])
    assert plan([20000], [0], [0], [1], one) == ([[0]], [34])
    for m in range(3):
        assert plan([AL + STRIDE * m], [m + 1], [0], [1], one) == ([], [0])
    # an idle slot beside a busy one; a free slot's closing flag is ignored
    assert plan([AL, 100], [1, 0], [STRIDE, 0], [0, 0], [1, 1]) == ([[0]], [30, 0])
    assert plan([AL, 0], [1, 0], [0, 0], [0, 1], [1, 0]) == ([], [0, 0])
    # the refusals
    for bad in (([0], [0], [0], [1], one),                      # closing a slot that was fed no sample at all
                ([0, 0], [0, 0], [0, 5], [0, 0], [1, 0]),       # samples for a slot that is not open
                ([-1], [0], [0], [0], one), ([0], [-1], [0], [0], one), ([0], [0], [-1], [0], one),
                ([AL], [0], [0], [0], one)):                    # a window count that does not belong to the samples
        with pytest.raises(ValueError):
            plan(*bad)
    with pytest.raises(ValueError):
        plan([0, 0], [0], [0, 0], [0, 0], [1, 1])               # one entry per slot
    assert long_form.pool_plan([0], [0], [AL], [0], one, _Cfg(AL))[0] == [[0]]


def test_plan_agrees_with_the_restatement_on_random_pools():
    rng = np.random.default_rng(20261020)
    for AL in AUDIO_LENS:
        for _ in range(100):
            S = int(rng.integers(1, 6))
            open_ = rng.integers(0, 2, S).astype(bool)
            fed = rng.integers(0, 6 * STRIDE, S)
            ran = np.array([_lib.long_stream_plan(int(f), 0, AL)[0] for f in fed])
            new = np.where(open_, rng.choice([0, 1, 4000, 3 * STRIDE], S), 0)
            closing = rng.integers(0, 2, S) * (fed + new >= 1)
            rounds, frames = _lib.long_pool_plan(fed, ran, new, closing, open_, AL)
            assert (rounds, frames.tolist()) == _restated(fed, ran, new, closing, open_, AL)


JOIN_FIELDS = ("slot", "on_device", "seed_poses", "vid_index", "scale", "emo", "text_features")
PUSH_FIELDS = ("sampler", "noise_mode", "skip_timesteps", "on_device", "use_graph", "clip_denoised", "two_pass_always", "eta", "capacity",
               "reserved", "n_max", "audio", "lengths", "closing", "given", "emo", "sag", "text_features", "x_init", "eps_tape", "noise_tape",
               "seed", "sample_offset", "frames", "n_frames", "n_rounds")
NEW_EXPORTS = ("ls_long_pool_plan", "ls_long_pool_open", "ls_long_pool_join", "ls_long_pool_push", "ls_long_pool_info")


def test_pool_structs_match_the_header_and_the_abi_is_unchanged(tmp_path):
    lib = _lib.load_library()
    assert lib.ls_abi_version() == 5
    hdr = open(os.path.join(ROOT, "include", "ls_hip.h")).read()
    for name in NEW_EXPORTS:
        assert name in _lib.EXPORTS and f"int {name}(" in hdr and hasattr(lib, name), name
    assert [n for n, _ in _lib.LsLongPoolJoinArgs._fields_] == list(JOIN_FIELDS)
    assert [n for n, _ in _lib.LsLongPoolPushArgs._fields_] == list(PUSH_FIELDS)
    prints = "".join(f'    printf("%zu\\n", offsetof(ls_long_pool_join_args, {f}));\n' for f in JOIN_FIELDS)
    prints += "".join(f'    printf("%zu\\n", offsetof(ls_long_pool_push_args, {f}));\n' for f in PUSH_FIELDS)
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "ls_hip.h"\nint main(void) {\n'
                   '    printf("%zu %zu %zu %zu %zu %d\\n", sizeof(ls_long_pool_join_args), sizeof(ls_long_pool_push_args), sizeof(ls_long_stream_cond),\n'
                   '           sizeof(ls_long_stream_push_args), sizeof(ls_long_sample_args), LS_ABI_VERSION);\n' + prints + '    return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got[:6] == [ctypes.sizeof(_lib.LsLongPoolJoinArgs), ctypes.sizeof(_lib.LsLongPoolPushArgs), ctypes.sizeof(_lib.LsLongStreamCond),
                       ctypes.sizeof(_lib.LsLongStreamPushArgs), 104, 5]
    nj = len(JOIN_FIELDS)
    assert got[6:6 + nj] == [getattr(_lib.LsLongPoolJoinArgs, f).offset for f in JOIN_FIELDS]
    assert got[6 + nj:] == [getattr(_lib.LsLongPoolPushArgs, f).offset for f in PUSH_FIELDS]
    for name in ("long_pool_open", "long_pool_join", "long_pool_push", "long_pool_info"):
        assert hasattr(_lib.Engine, name)
    assert hasattr(_lib, "long_pool_plan")


def test_pool_plan_on_its_edges_under_asan_and_ubsan(tmp_path):
    """tests/pool_plan_main.cpp with the plan's unit, as plain C++ with the host sanitizers linked statically: a child process of its
    own, nothing preloaded, nothing inside Python, no GPU."""
    exe = str(tmp_path / "pool_plan")
    made = subprocess.run([build.hipcc_path(), "-x", "c++", "-std=c++17", "-O1", "-g", "-fno-gpu-sanitize", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "pool_plan_main.cpp"),
                           os.path.join(ROOT, "livelyspeaker_amd", "csrc", "ls_chain_plan.cpp"), "-o", exe], capture_output=True, text=True)
    assert made.returncode == 0, made.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr
    assert run.stderr == "", run.stderr


@pytest.mark.parametrize("ds", ["ted", "beat"])
def test_pool_refusals_come_before_any_engine(ds, monkeypatch):
    _no_engine(monkeypatch)
    cfg, model, diffusion = _parts(ds)
    y = synth.make_long_cond(cfg, 2, 2)
    with pytest.raises(TypeError):
        long_form.open_pool(diffusion, model.model, 4)                      # the bare RAG, not the CFG wrapper
    with pytest.raises(ValueError):
        long_form.open_pool(diffusion, model, 4, sampler="plms")
    with pytest.raises(ValueError):
        long_form.open_pool(diffusion, model, 4, skip_timesteps=diffusion.num_timesteps)
    with pytest.raises(ValueError):
        long_form.open_pool(diffusion, model, 0)
    diffusion.noise_source = "torch_device"
    with pytest.raises(NotImplementedError):
        long_form.open_pool(diffusion, model, 4)
    diffusion.noise_source = "torch_cpu"
    pool = long_form.open_pool(diffusion, model, 4)                         # opening touches no engine
    assert not pool.slots["open"].any() and pool.slots["samples_in"].tolist() == [0, 0, 0, 0]
    emo = {"emo": int(y["emo"][0, 0])} if ds == "beat" else {}
    with pytest.raises(ValueError, match="seed_poses"):
        pool.join(y["seed_poses"][0][..., :3], 1, 1.0, **emo)
    with pytest.raises(ValueError, match="text_features without sag"):
        pool.join(y["seed_poses"][0], 1, 1.0, text_features=np.zeros(512, np.float32), **emo)
    with pytest.raises(ValueError, match="slot"):
        pool.join(y["seed_poses"][0], 1, 1.0, slot=4, **emo)
    with pytest.raises(ValueError, match="BEAT"):
        pool.join(y["seed_poses"][0], 1, 1.0, **({} if ds == "beat" else {"emo": 0}))     # BEAT without emo, TED with one
    for bad in (np.zeros(100, np.float32), np.zeros((3, 100), np.float32)):
        with pytest.raises(ValueError, match="audio"):
            pool.push(bad, [0, 0, 0, 0])
    with pytest.raises(ValueError, match="lengths"):
        pool.push(np.zeros((4, 100), np.float32), [0, 0, 0, 101])
    with pytest.raises(ValueError):
        pool.push(np.zeros((4, 100), np.float32), [100, 0, 0, 0])           # samples for a slot that is not open
    with pytest.raises(ValueError, match="not open"):
        pool.leave(0)
    with pool as inside:
        assert inside is pool
    with pytest.raises(RuntimeError, match="closed"):
        pool.push(np.zeros((4, 0), np.float32), [0, 0, 0, 0])
    with pytest.raises(RuntimeError, match="closed"):
        pool.join(y["seed_poses"][0], 1, 1.0, **emo)
