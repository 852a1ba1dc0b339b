"""The host-only plans of the chained-window engine (csrc/ls_chain_plan.cpp) under the host sanitizers: tests/chain_plan_main.cpp links
that unit alone -- it includes no HIP header -- and walks ls_long_plan_drop, ls_long_edit_plan, ls_long_stream_plan and feed_copies over
their edges.  A stand-alone program run as a child process: nothing is preloaded, nothing runs inside Python, nothing touches a GPU.  It
is built with the project's compiler as plain C++ (clang links the sanitizer runtimes statically, so the program needs nothing from its
environment).  With arguments the same program prints feed_copies' answer, which is checked here against the definition restated."""
import os
import subprocess

import numpy as np
import pytest

from livelyspeaker_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("chain_plan") / "chain_plan")
    made = subprocess.run([build.hipcc_path(), "-x", "c++", "-std=c++17", "-O1", "-g", "-fno-gpu-sanitize", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "chain_plan_main.cpp"),
                           os.path.join(ROOT, "livelyspeaker_amd", "csrc", "ls_chain_plan.cpp"), "-o", path], capture_output=True, text=True)
    assert made.returncode == 0, made.stderr
    return path


def test_chain_planners_on_their_edges_under_asan_and_ubsan(exe):
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr
    assert run.stderr == "", run.stderr


def test_feed_copies_are_the_maximal_runs_of_slots_fed_alike(exe):
    """Random (position, take) vectors for up to eight slots, values from a small set so that neighbours often agree.  Restated: a
    copy's slots [first, first + n) all hold its (position, take); the runs -- the copies at offset 0 -- partition the slots with
    take > 0; no run could be longer; a run is one copy, or two that split its take at the ring's end."""
    R, rng = 100, np.random.default_rng(2025)
    cases = [(np.full(S, 37), np.full(S, 80)) for S in range(1, 9)]                      # lockstep, wrapping: one run each
    cases += [(rng.choice([0, 37, 90], S), rng.choice([0, 10, 63, 100], S)) for S in rng.integers(1, 9, 300)]
    args = [str(R)] + [str(v) for pos, take in cases for v in (len(pos), *pos, *take)]
    run = subprocess.run([exe] + args, capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and run.stderr == "", run.stderr
    lines = run.stdout.split("\n")[:-1]
    assert len(lines) == len(cases)
    for i, ((pos, take), line) in enumerate(zip(cases, lines)):
        copies = np.array(line.split(), dtype=int).reshape(-1, 5)
        runs = [c for c in copies if c[3] == 0]
        covered = [s for first, n, *_ in runs for s in range(first, first + n)]
        assert covered == [s for s in range(len(pos)) if take[s] > 0], (pos, take, copies)
        for first, n, p, off, length in runs:
            assert all((pos[s], take[s]) == (p, take[first]) for s in range(first, first + n))
            for s in (first - 1, first + n):                                             # maximal: the neighbours differ
                assert not (0 <= s < len(pos) and (pos[s], take[s]) == (pos[first], take[first])), (pos, take, copies)
            pieces = [tuple(c[2:]) for c in copies if c[0] == first]
            head = min(take[first], R - p)
            assert pieces == [(p, 0, head)] + ([(0, head, take[first] - head)] if take[first] > head else []), (pos, take, copies)
        if i < 8:
            assert len(runs) == 1 and len(copies) == 2
