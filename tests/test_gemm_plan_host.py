"""CPU: the dispatch decision of launch_gemm_tr (csrc/ls_gemm_plan.h: gemm_plan).  tests/gemm_plan_main.cpp is compiled with the project's
hipcc into a host-only program that prints the plan of every case of tools/gemm_cases.h -- the shapes tools/gemm_check.cpp runs on the
GPU -- and of the production shapes named in the comments of ls_gemm.hip.  The kind of every case is tests/gemm_cases.py, shared with
tests/test_gpu_gemm.py; the schedules, the re-derived split counts and the two rejected calls are asserted here."""
import os
import subprocess

import pytest

from conftest import ROOT
from gemm_cases import GROUP, KIND
from livelyspeaker_amd import build


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("gemm_plan") / "gemm_plan")
    cmd = [build.hipcc_path(), "--offload-arch=gfx950", "-O2", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-I" + build.CSRC,
           "-I" + os.path.join(ROOT, "tools"), os.path.join(ROOT, "tests", "gemm_plan_main.cpp"), "-o", exe]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    out = {}
    for line in run.stdout.splitlines():
        f = dict(kv.split("=", 1) for kv in line.split())
        for k in ("gx", "nbig", "splits", "kchunk", "nbatch", "fast", "ws_too_small", "split_epilogue"):
            f[k] = int(f[k])
        f["grid"] = tuple(int(v) for v in f["grid"].split(","))
        assert f["case"] not in out
        out[f["case"]] = f
    return out


def test_every_case_takes_the_kernel_it_was_written_for(plans):
    cases = {n: p for n, p in plans.items() if p["group"] != "production"}
    assert sorted(cases) == sorted(KIND)                # the table and the checker's case list name the same cases
    assert [(n, p["group"], p["kind"]) for n, p in cases.items() if (p["group"], p["kind"]) != (GROUP[n], KIND[n])] == []
    # every variant of the dispatch is reached by some case
    assert {p["kind"] for p in cases.values()} == {"general", "full128", "full64", "dma_halves", "dma_whole_halves", "dma_whole", "dma_3d"}


def test_production_shapes(plans):
    p = plans["p_17408x512x512"]                         # 1088 tiles on 768 slots: 768 whole tiles + 640 halves
    assert (p["kind"], p["gx"], p["nbig"], p["grid"]) == ("dma_whole_halves", 4, 768, (768 + 640, 1, 1))
    p = plans["p_384x512x512"]                           # 24 tiles: every one as two halves
    assert (p["kind"], p["gx"], p["nbig"], p["grid"]) == ("dma_halves", 4, 0, (48, 1, 1))
    p = plans["p_544_tiles"]                             # 544 tiles of 128 x 128 fill the chip badly: 64-row variant, 1088 workgroups
    assert (p["kind"], p["grid"], p["fast"]) == ("full64", (4, 272, 1), 1)
    p = plans["p_768_tiles"]                             # LS_GEMM_HALF_MAX itself still runs as halves ...
    assert (p["kind"], p["grid"]) == ("dma_halves", (1536, 1, 1))
    p = plans["p_776_tiles"]                             # ... the next grid as one full round and a short round of halves
    assert (p["kind"], p["nbig"], p["grid"]) == ("dma_whole_halves", 768, (768 + 16, 1, 1))
    p = plans["p_tokmix_long"]                           # the long path's token mixing: one problem per sequence on the 3-D grid
    assert (p["kind"], p["grid"], p["nbatch"], p["splits"]) == ("general", (1, 4, 12), 12, 1)


def test_the_schedules_of_the_checked_shapes(plans):
    p = plans["d_14464"]                                 # 904 tiles: 768 whole + 136 as 272 halves
    assert (p["gx"], p["nbig"], p["grid"]) == (4, 768, (768 + 272, 1, 1))
    p = plans["d_20352"]                                 # 1272 tiles: the last round of 504 is above 60 % of the slots, all whole
    assert (p["gx"], p["nbig"], p["grid"]) == (4, 1272, (1272, 1, 1))
    assert plans["ln_14464"]["nbig"] == 768 and plans["ln_14464"]["grid"] == (1040, 1, 1)
    assert plans["d_128_none"]["grid"] == (4, 1, 1) and plans["d_384x512x512"]["grid"] == (48, 1, 1)
    assert plans["d_batch3"]["grid"] == (1, 2, 3) and plans["d_split2"]["grid"] == (1, 2, 2) and plans["s_128_dma"]["grid"] == (1, 2, 4)
    assert plans["f_64row"]["grid"] == (4, 10, 1) and plans["f_256x128x64_rc"]["grid"] == (1, 2, 1)
    assert plans["s_tokmix_split"]["grid"] == (1, 4, 8) and plans["s_wgrad_batch"]["grid"] == (1, 1, 6)
    # whole 128-row tiles or the general kernel: the unpadded row counts never reach the LDS-DMA kernel
    assert [plans[n]["fast"] for n in ("d_64x128x32", "d_14400", "d_20288")] == [0, 0, 0]


def test_splits_are_re_derived_on_k_tile_boundaries(plans):
    p = plans["s_req5_k96"]                              # 5 requested over K = 96: 3 splits of 32
    assert (p["splits"], p["kchunk"], p["grid"][2]) == (3, 32, 3)
    p = plans["s_131x67x200_rr"]                         # 3 over 200: 96 + 96 + a tail of 8
    assert (p["splits"], p["kchunk"]) == (3, 96)
    p = plans["s_512x37x300"]
    assert (p["splits"], p["kchunk"]) == (2, 160)
    p = plans["s_tokmix_split"]                          # 2 over 37: 32 + 5
    assert (p["splits"], p["kchunk"], p["nbatch"]) == (2, 32, 4)
    assert all(p["splits"] == 1 and p["kchunk"] >= 1 for n, p in plans.items() if GROUP.get(n) in ("general", "fulltile", "dma_ln"))


def test_the_two_rejected_calls(plans):
    for name in ("s_reject_act", "s_reject_cpre", "s_reject_r"):        # splits > 1 with an epilogue the reduction cannot apply
        assert (plans[name]["split_epilogue"], plans[name]["ws_too_small"]) == (1, 0), name
    assert (plans["s_reject_ws"]["split_epilogue"], plans["s_reject_ws"]["ws_too_small"]) == (0, 1)      # one float short
    assert (plans["p_no_ws"]["split_epilogue"], plans["p_no_ws"]["ws_too_small"]) == (0, 1)              # no workspace at all
    flagged = {n for n, p in plans.items() if p["split_epilogue"] or p["ws_too_small"]}
    assert flagged == {"s_reject_act", "s_reject_cpre", "s_reject_r", "s_reject_ws", "p_no_ws"}          # an exact workspace is accepted
