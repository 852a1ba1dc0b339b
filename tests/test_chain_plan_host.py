"""The host-only plans of the chained-window engine (csrc/ls_chain_plan.cpp) under the host sanitizers: tests/chain_plan_main.cpp links
that unit alone -- it includes no HIP header -- and walks ls_long_plan_drop, ls_long_edit_plan and ls_long_stream_plan over their edges.
A stand-alone program run as a child process: nothing is preloaded, nothing runs inside Python, nothing touches a GPU.  It is built with
the project's compiler as plain C++ (clang links the sanitizer runtimes statically, so the program needs nothing from its environment)."""
import os
import subprocess

from livelyspeaker_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_chain_planners_on_their_edges_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "chain_plan")
    made = subprocess.run([build.hipcc_path(), "-x", "c++", "-std=c++17", "-O1", "-g", "-fno-gpu-sanitize", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "chain_plan_main.cpp"),
                           os.path.join(ROOT, "livelyspeaker_amd", "csrc", "ls_chain_plan.cpp"), "-o", exe], capture_output=True, text=True)
    assert made.returncode == 0, made.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr
    assert run.stderr == "", run.stderr
