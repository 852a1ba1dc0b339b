"""Hardware check of the transformer towers' non-GEMM kernels on their own, against fp64: k_sag_attention<128,34,false> (dense and
compact rows), k_sag_attention<128,36,true> and k_sag_enc_attention_row0<128> (key masks), k_clip_attention<64> (ragged causal rows, both
sides of the 64 KB LDS switch), k_layernorm512 / k_layernorm512x2, k_sag_final, k_sag_queries and k_sag_enc_prepare.

tools/xfmr_check.cpp is compiled once with the library's code-generation flags together with ls_sag.hip, ls_sag_enc.hip and
ls_clip_text.hip, and started once per group as a child process.  For every case (tools/xfmr_cases.h, names in tests/xfmr_cases.py) it
embeds the operands in NaN guards, pre-fills the outputs with a NaN sentinel, launches twice and compares EVERY logical output element
with the double-precision reference under the per-element bound derived in tools/xfmr_ref.h.  Asserted per case: worst err / bound <= 1
(`ratio`, and `ratio0` / `ratiox` for the one-query encoder kernel against fp64 and against row 0 of the full kernel), no non-finite
output, every byte outside the logical extents untouched, the two launches bit-identical, and the bitwise claims (`same`): compact
decoder rows == dense rows; masked keys' K / V cannot reach the output; a CLIP row depends on its own index and its own keys alone
(len 80 relaunched with len 1 / 17 / 64, a sample alone against the same sample inside a batch, K / V above the row rewritten);
k_layernorm512x2 == two k_layernorm512 launches; qc rows == the q rows they copy; k_sag_enc_prepare == its fp32 statement; masked
k_sag_final outputs are exactly +0 (`zero`).  tests/test_xfmr_ref_host.py checks the references against torch float64 and shows that
the bounds reject every known-wrong form by a factor 4 or more.

Measured on the MI355X (profiles/r30_xfmr_check.md), worst err / bound per group:
    dec 0.0095 (dec_big_b2)    enc 0.0087 (enc_only01; one-query kernel 0.0023, against row 0 of the full kernel 0.0019)
    clip 0.039 (clip_probe; 0.014 otherwise, clip_l31)    ln 0.043 (ln_mixed_r103)    final 0.0013 (fin_jf282_b3_null)
    queries 0.042 (qry_n34_b1)    prepare: exact
The softmax constant: with exact scores (clip_probe: integer q and k, scale 1/8, positive v) the kernel's probabilities-times-V lie at
most 7.83 ulp of the result from fp64; kCexp = 4 x 7.83 = 31.3 rounded up to a power of two, 32.
k_layernorm512x2 against two k_layernorm512 launches: bit-identical at the first run, in all four cases; no kernel was changed.  So were
the compact decoder layout and the three CLIP row-independence checks."""
import os
import subprocess
import time

import pytest

from conftest import ROOT
from livelyspeaker_amd import build
from xfmr_cases import CASES, SAME, ZERO

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("xfmr_check") / "xfmr_check")
    cmd = [build.hipcc_path()] + build.codegen_flags() + ["-I" + os.path.join(ROOT, "tools"), "-x", "hip", os.path.join(ROOT, "tools", "xfmr_check.cpp")]
    cmd += [os.path.join(build.CSRC, s) for s in ("ls_sag.hip", "ls_sag_enc.hip", "ls_clip_text.hip")] + ["-o", exe]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, (res.stdout + res.stderr)[-4000:]
    return exe


# the limits: every group ran in under a second on the MI355X (the first run of a process pays the runtime's start-up, 1 - 2 s)
@pytest.mark.parametrize("group,limit", [("dec", 60), ("enc", 60), ("clip", 60), ("ln", 60), ("final", 60), ("queries", 60), ("prepare", 60)])
def test_xfmr_against_fp64(checker, group, limit):
    t0 = time.time()
    run = subprocess.run([checker, group], capture_output=True, text=True, timeout=limit)
    seconds = time.time() - t0
    assert run.returncode == 0, run.stdout[-4000:] + run.stderr[-2000:]
    lines = [dict(kv.split("=", 1) for kv in line.split()) for line in run.stdout.splitlines() if line.startswith("case=")]
    assert sorted(f["case"] for f in lines) == sorted(CASES[group]), run.stdout
    ratios = lambda f: [float(v) for k, v in f.items() if k.startswith("ratio")]
    worst = max(lines, key=lambda f: max(ratios(f)))
    print(f"{group}: {len(lines)} cases in {seconds:.1f} s, worst err / bound {max(ratios(worst)):.4g} ({worst['case']})")
    for f in lines:
        if "expulp" in f:
            print(f"{f['case']}: worst distance of P.V from fp64 with exact scores {f['expulp']} ulp")
    bad = []
    for f in lines:
        ok = (max(ratios(f)) <= 1.0 and int(f["nonfinite"]) == 0 and f["guard"] == "ok" and f["repeat"] == "ok" and
              f.get("same", "ok") == "ok" and f.get("zero", "ok") == "ok")
        if not ok:
            bad.append(" ".join(f"{k}={v}" for k, v in f.items()))
    assert bad == [], "\n".join(bad)
    # the bitwise claims did compare
    assert sorted(f["case"] for f in lines if "same" in f) == sorted(n for n in SAME if n in CASES[group])
    assert sorted(f["case"] for f in lines if "zero" in f) == sorted(n for n in ZERO if n in CASES[group])
    if group == "enc":
        assert all("ratio0" in f and "ratiox" in f for f in lines)
    if group == "clip":
        assert [f["case"] for f in lines if "expulp" in f] == ["clip_probe"]
