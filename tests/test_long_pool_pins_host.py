"""Host side of pinned poses on a session (``open_pool(pins=H)``, ``LongPool.pin``): the sampling calls a push runs
(ls_long_pool_pin_plan) against a restatement of the rule written here, on the staggered schedule of tests/test_long_pool_host.py with
pins placed so that it yields every kind of call; the refusals raised before an engine exists; and tests/pool_pin_plan_main.cpp -- a
stand-alone program around the plan -- under the host sanitizers.  No GPU."""
import os
import subprocess

import numpy as np
import pytest

from livelyspeaker_amd import _lib, build, long_form, synth
from test_long_form_host import _no_engine, _parts
from test_long_pool_host import AUDIO_LENS, HostPool, _Cfg, staggered

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAP, HORIZON = 4, 64


def pinned_schedule(AL):
    """The staggered schedule with ``("pin", (speaker, frames, kind))`` events between its pushes; ``kind``: 'pose' pins the whole
    pose of every frame named, 'feature' one feature of one joint.  What the pushes then run, as (round, pinned, slots):

    * push 1: A's window 0 alone, pinned (frame 5, and frame 33: one of the frames 30-33 window 0 owns and window 1 starts from) --
      a round with only pinned rows;
    * push 2: round 0 is B plain, then A (frames 34 and 63: the first and the last frame its window 1 owns) and C (frame 3) pinned
      -- a round with both kinds; round 1 is C's window 1, pinned (frame 40);
    * push 3: D plain, then C's window 2 pinned at frame 67 = 3 + 64: the ring position frame 3 held, with fewer elements pinned, so
      a byte that window 0 had not cleared would show."""
    events = []
    for event, payload in staggered(AL):
        if event == "push" and payload[0][0] == AL:                 # ahead of the first push: A, frames_out 0
            events += [("pin", ("A", [33], "pose")), ("pin", ("A", [5], "feature"))]
        if event == "push" and payload[0][0] == 32000:              # ahead of the second: A at frames_out 34, C fresh
            events += [("pin", ("A", [34, 63], "pose")), ("pin", ("C", [3, 40], "pose"))]
        if event == "push" and payload[0][0] == 0:                  # ahead of the third: C at frames_out 64
            events += [("pin", ("C", [67], "feature"))]
        events.append((event, payload))
    return events


# what the pushes (and the leave, and the close) of pinned_schedule run: lists of (round, pinned, slots)
EXPECTED_CALLS = [[(0, True, [0])],
                  [(0, False, [1]), (0, True, [0, 3]), (1, True, [3])],
                  [(0, False, [1])],
                  [(0, False, [1]), (0, True, [3])],
                  []]


def owned(w):
    return (0, 34) if w == 0 else (30 * w + 4, 30 * w + 34)


def restated_calls(rounds, ran, pins):
    """The rule, restated: in round r slot s runs its window ran[s] + r; its row is pinned iff a pending frame of the slot is one that
    window owns; the round is its plain rows, ascending, then its pinned rows, ascending, an empty half skipped."""
    calls = []
    for r, slots in enumerate(rounds):
        is_pinned = {s: any(owned(int(ran[s]) + r)[0] <= n < owned(int(ran[s]) + r)[1] for n in pins[s]) for s in slots}
        for half in (False, True):
            rows = [s for s in slots if is_pinned[s] == half]
            if rows:
                calls.append((r, half, rows))
    return calls


def run_schedule(AL, events, with_pins=True):
    """The events through HostPool and the plan: the calls of every push, leave and close; the pending pins are spent as windows own them."""
    pool, who, pins, out = HostPool(CAP, AL), {}, [set() for _ in range(CAP)], []
    for event, payload in events:
        if event == "join":
            s = pool.join(payload[1])
            who[s] = payload[0]
            pins[s] = set()
            continue
        if event == "pin":
            if with_pins:
                s = next(s for s, k in who.items() if k == payload[0] and pool.open[s])
                frames_out = 0 if pool.ran[s] == 0 else 30 * int(pool.ran[s]) + 4
                assert all(frames_out <= n < frames_out + HORIZON for n in payload[1]), (payload, frames_out)
                pins[s] |= set(payload[1])
            continue
        lengths = payload[0] if event == "push" else [0] * CAP
        closing = [int(event == "close" or (event == "leave" and who.get(s) == payload[0])) * int(pool.open[s]) for s in range(CAP)]
        ran = pool.ran.copy()
        rounds, _ = pool.push(lengths, closing)
        n_windows = [sum(s in r for r in rounds) for s in range(CAP)]
        calls = _lib.long_pool_pin_plan(ran, n_windows, pins)
        assert calls == restated_calls(rounds, ran, pins) == long_form.pool_pin_plan(ran, n_windows, pins, _Cfg(AL))
        assert _lib.long_pool_pin_plan(ran, n_windows, None) == [(r, False, slots) for r, slots in enumerate(rounds)]
        for r, pinned, slots in calls:
            for s in slots if pinned else ():
                lo, hi = owned(int(ran[s]) + r)
                pins[s] = {n for n in pins[s] if not lo <= n < hi}
        for s in range(CAP):
            if closing[s]:
                pins[s] = set()
        out.append(calls)
    return out, pins


@pytest.mark.parametrize("AL", AUDIO_LENS)
def test_the_pinned_schedule_runs_the_calls_the_issue_names(AL):
    calls, left = run_schedule(AL, pinned_schedule(AL))
    assert calls == EXPECTED_CALLS
    assert left == [set()] * CAP                                        # every pin was spent by the window that owns it
    # a round with only pinned rows, a round with both kinds, and a pin on frames 30-33 that window 0 honours, not window 1
    assert calls[0] == [(0, True, [0])] and {p for _, p, _ in calls[1][:2]} == {False, True}
    assert _lib.long_pool_pin_plan([1], [1], [[33]]) == [(0, False, [0])] and _lib.long_pool_pin_plan([0], [2], [[33]]) == [(0, True, [0]), (1, False, [0])]
    # the first and the last frame a window owns
    for w in (1, 2, 7):
        for n, pinned in ((30 * w + 3, False), (30 * w + 4, True), (30 * w + 33, True), (30 * w + 34, False)):
            assert _lib.long_pool_pin_plan([w], [1], [[n]]) == [(0, pinned, [0])], (w, n)
    # no pins at all: pool_plan's rounds exactly
    plain, _ = run_schedule(AL, pinned_schedule(AL), with_pins=False)
    want = [payload[1] if event != "close" else payload for event, payload in staggered(AL) if event != "join"]
    assert [[slots for _, _, slots in c] for c in plain] == want and not any(p for c in plain for _, p, _ in c)


def test_plan_agrees_with_the_restatement_on_random_pools():
    rng = np.random.default_rng(20261021)
    for _ in range(200):
        S = int(rng.integers(1, 6))
        ran = rng.integers(0, 5, S)
        n_windows = rng.integers(0, 4, S)
        pins = [set(int(n) for n in rng.integers(0, 260, int(rng.integers(0, 4)))) for _ in range(S)]
        rounds = [[s for s in range(S) if n_windows[s] > r] for r in range(int(n_windows.max()))]
        assert _lib.long_pool_pin_plan(ran, n_windows, pins) == restated_calls(rounds, ran, pins)
    for bad in (([0], [-1], [[]]), ([-1], [1], [[]]), ([0], [1], [[-3]]), ([0, 0], [1], [[], []]), ([0], [1], [[], []])):
        with pytest.raises(ValueError):
            _lib.long_pool_pin_plan(*bad)


def test_exports_and_the_header():
    lib = _lib.load_library()
    assert lib.ls_abi_version() == 5                                    # new entries only: no struct moved
    hdr = open(os.path.join(ROOT, "include", "ls_hip.h")).read()
    for name in ("ls_long_pool_pin_plan", "ls_long_pool_pins", "ls_long_pool_pin", "ls_long_pool_unpin", "ls_long_pool_pin_tape", "ls_long_pool_pin_info"):
        assert name in _lib.EXPORTS and f"int {name}(" in hdr and hasattr(lib, name), name
    for name in ("long_pool_pins", "long_pool_pin", "long_pool_unpin", "long_pool_pin_info"):
        assert hasattr(_lib.Engine, name)


def test_pin_plan_on_its_edges_under_asan_and_ubsan(tmp_path):
    """tests/pool_pin_plan_main.cpp with the plan's unit, as plain C++ with the host sanitizers linked statically: a child process of
    its own, nothing preloaded, nothing inside Python, no GPU."""
    exe = str(tmp_path / "pool_pin_plan")
    made = subprocess.run([build.hipcc_path(), "-x", "c++", "-std=c++17", "-O1", "-g", "-fno-gpu-sanitize", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "pool_pin_plan_main.cpp"),
                           os.path.join(ROOT, "livelyspeaker_amd", "csrc", "ls_chain_plan.cpp"), "-o", exe], capture_output=True, text=True)
    assert made.returncode == 0, made.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr
    assert run.stderr == "", run.stderr


@pytest.mark.parametrize("ds", ["ted", "beat"])
def test_pin_refusals_come_before_any_engine(ds, monkeypatch):
    _no_engine(monkeypatch)
    cfg, model, diffusion = _parts(ds)
    J, F = cfg.njoints, cfg.nfeats
    y = synth.make_long_cond(cfg, 2, 2)
    for bad in (33, 0, -1, True, 64.0, "64", (1 << 20) + 1):
        with pytest.raises(ValueError, match="pins"):
            long_form.open_pool(diffusion, model, CAP, pins=bad)
        with pytest.raises(ValueError, match="pins"):
            long_form.open_stream(diffusion, model, y["seed_poses"], y["vid_indices"], y["scale"], emo=(y["emo"][:, 0] if ds == "beat" else None), pins=bad)
    diffusion.noise_source = "torch_device"
    with pytest.raises(NotImplementedError):
        long_form.open_pool(diffusion, model, CAP, pins=HORIZON)
    diffusion.noise_source = "torch_cpu"
    pose = lambda k: np.zeros((J, F, k), np.float32)        # noqa: E731
    plain = long_form.open_pool(diffusion, model, CAP)
    assert "pins" not in plain.slots
    plain._state["open"][0] = True                          # as after a join: the refusals below come ahead of the engine
    with pytest.raises(ValueError, match="pins=H"):
        plain.pin(0, [3], pose(1))
    with pytest.raises(ValueError, match="pins=H"):
        plain.unpin(0)
    pool = long_form.open_pool(diffusion, model, CAP, pins=HORIZON)     # opening touches no engine
    assert pool.slots["pins"].tolist() == [0] * CAP
    with pytest.raises(ValueError, match="not open"):
        pool.pin(0, [3], pose(1))                           # a slot that is not open
    with pytest.raises(ValueError, match="not open"):
        pool.pin(CAP, [3], pose(1))
    pool._state["open"][0] = True
    pool._state["frames_out"][0] = 34                       # as after the slot's window 0
    for frames in ([33], [34 + HORIZON], [40, 33], [-1]):   # below frames_out; at or beyond frames_out + horizon
        with pytest.raises(ValueError, match="outside"):
            pool.pin(0, frames, pose(len(frames)))
        with pytest.raises(ValueError, match="outside"):
            pool.unpin(0, frames)
    with pytest.raises(ValueError, match="twice"):
        pool.pin(0, [40, 41, 40], pose(3))                  # duplicate frames in one call
    for frames in ([], [[40]], [40.0], "40"):
        with pytest.raises(ValueError, match="frames"):
            pool.pin(0, frames, pose(1))
    with pytest.raises(ValueError, match="poses"):
        pool.pin(0, [40, 41], pose(1))
    with pytest.raises(ValueError, match="poses"):
        pool.pin(0, [40], np.zeros((J, F), np.float32))
    with pytest.raises(ValueError, match="mask"):
        pool.pin(0, [40], pose(1), mask=np.ones((J, F, 1), np.float32))        # not bool
    with pytest.raises(ValueError, match="mask"):
        pool.pin(0, [40], pose(1), mask=np.ones((J, 1), bool))
    pool._sag = object()                                    # as a pool opened with sag=: pins with it are not built
    with pytest.raises(ValueError, match="sag"):
        pool.pin(0, [40], pose(1))
    pool._sag = None
    assert pool.slots["pins"].tolist() == [0] * CAP and pool._pending == [set()] * CAP and pool._eng is None      # nothing was taken
    emo = {"emo": y["emo"][:, 0]} if ds == "beat" else {}
    st = long_form.open_stream(diffusion, model, y["seed_poses"], y["vid_indices"], y["scale"], pins=HORIZON, **emo)
    assert st.pins == 0
    with pytest.raises(ValueError, match="outside"):
        st.pin([HORIZON], np.zeros((2, J, F, 1), np.float32))
    with pytest.raises(ValueError, match="poses"):
        st.pin([3], pose(1))                                # one pose per clip: [B, J, F, K]
    with pytest.raises(ValueError, match="pins=H"):
        long_form.open_stream(diffusion, model, y["seed_poses"], y["vid_indices"], y["scale"], **emo).pin([3], np.zeros((2, J, F, 1), np.float32))
    pool._closed = True
    with pytest.raises(RuntimeError, match="closed"):
        pool.pin(0, [40], pose(1))
