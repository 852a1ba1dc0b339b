"""Hardware check of the strided MFMA GEMM (csrc/ls_gemm.hip) on its own, on every dispatch path, against fp64.

tools/gemm_check.cpp is compiled once, with the library's code-generation flags, together with ls_gemm.hip.  For every case of a group
(tools/gemm_cases.h) it embeds the operands in NaN, pre-fills the outputs with a NaN sentinel, launches through launch_gemm_tr twice
and compares EVERY output element with a double-precision evaluation under the derived bound
    |err| <= 2 (K + 8) 2^-24 (sum_k |a_k b_k| + |bias| + |R| + |C_old|)
carried through the activation's Lipschitz constant.  Asserted per case: the kind of kernel that ran (tests/gemm_cases.py, shared with
tests/test_gemm_plan_host.py), worst err / bound <= 1, no non-finite output, every byte outside the logical extents untouched, the two
launches bit-identical, and -- for the rows of the 14464-row product recomputed alone -- bit-identical across tile schedules.

Measured on the MI355X (profiles/r23_gemm_check.md): the worst ratio is 0.083 for a product (K = 7; a few percent, as the sqrt(K) growth
of the error against the bound's K predicts) and 0.062 with the fused LayerNorm.  The activation term is c = 32 ulp of the result: the
worst distance of C from act64 of the kernel's own pre-activation at K = 32 is 7.13 ulp (exact GELU; SiLU 2.35, exp 0.77, QuickGELU
2.82), times 4, rounded up to a power of two.  The reconstructed rstd of the LayerNorm epilogue is within 2.29e-7 of fp64 (relative);
the bound carries 4 x that, 9.2e-7."""
import os
import subprocess
import time

import pytest

from conftest import ROOT
from gemm_cases import GROUP, KIND
from livelyspeaker_amd import build

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("gemm_check") / "gemm_check")
    cmd = [build.hipcc_path()] + build.codegen_flags() + ["-I" + os.path.join(ROOT, "tools"), "-x", "hip",
           os.path.join(ROOT, "tools", "gemm_check.cpp"), os.path.join(build.CSRC, "ls_gemm.hip"), "-o", exe]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, (res.stdout + res.stderr)[-4000:]
    return exe


@pytest.mark.parametrize("group,limit", [("general", 60), ("fulltile", 60), ("dma", 90), ("dma_ln", 90), ("splitk", 60)])
def test_gemm_against_fp64(checker, group, limit):
    t0 = time.time()
    run = subprocess.run([checker, group], capture_output=True, text=True, timeout=limit)
    seconds = time.time() - t0
    assert run.returncode == 0, run.stdout[-4000:] + run.stderr[-2000:]
    lines = [dict(kv.split("=", 1) for kv in line.split()) for line in run.stdout.splitlines() if line.startswith("case=")]
    assert sorted(f["case"] for f in lines) == sorted(n for n, g in GROUP.items() if g == group), run.stdout
    worst = max(lines, key=lambda f: float(f["ratio"]))
    print(f"{group}: {len(lines)} cases in {seconds:.1f} s, worst err / bound {worst['ratio']} ({worst['case']})")
    bad = []
    for f in lines:
        ok = (f["kind"] == KIND[f["case"]] and float(f["ratio"]) <= 1.0 and int(f["nonfinite"]) == 0 and f["guard"] == "ok" and
              f["repeat"] == "ok" and f.get("same", "ok") == "ok" and f.get("rejected", "yes") == "yes")
        if not ok:
            bad.append(" ".join(f"{k}={v}" for k, v in f.items()) + f" (written for kind={KIND[f['case']]})")
    assert bad == [], "\n".join(bad)
    if group == "dma":          # the schedule-independence cases did compare, and the rejected calls were rejected
        assert sorted(f["case"] for f in lines if "same" in f) == ["d_rows0_128", "d_rows0_64", "d_rows12288_128", "d_rows12288_64"]
    if group == "splitk":
        assert sorted(f["case"] for f in lines if "rejected" in f) == ["s_reject_act", "s_reject_cpre", "s_reject_r", "s_reject_ws"]
