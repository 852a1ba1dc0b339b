"""CPU: the references and bounds that tests/test_gpu_xfmr.py holds the transformer kernels to are themselves checked here.

`xfmr_check --host <group> <dir>` (tools/xfmr_check.cpp; no HIP call) writes every case's inputs and double-precision references.
  * Reference agreement: every reference is compared with an independent float64 torch statement of the same operation
    (softmax(q k^T / sqrt(hd) + mask) v, F.layer_norm, plain matmuls), tolerance 1e-12 of max|ref|; k_sag_enc_prepare's outputs are
    copies and single fp32 additions and are compared exactly.
  * Sensitivity: for every known-wrong reference that applies to a case (tests/xfmr_cases.py: required_perturbations) the checker
    reports max |wrong - true| / bound; it must be at least 4.  With err / bound <= 1 on the GPU this proves the kernel's result cannot
    be the wrong one.  It depends on the references and the bounds only, never on a kernel."""
import os
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import ROOT
from livelyspeaker_amd import build
from xfmr_cases import CASES, GROUPS, required_perturbations

T, S_ENC, D = 34, 36, 512


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("xfmr_check") / "xfmr_check")
    cmd = [build.hipcc_path()] + build.codegen_flags() + ["-I" + os.path.join(ROOT, "tools"), "-x", "hip", os.path.join(ROOT, "tools", "xfmr_check.cpp")]
    cmd += [os.path.join(build.CSRC, s) for s in ("ls_sag.hip", "ls_sag_enc.hip", "ls_clip_text.hip")] + ["-o", exe]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, (res.stdout + res.stderr)[-4000:]
    return exe


class Dumped:
    """The files and printed lines of one group."""

    def __init__(self, exe, group, where):
        run = subprocess.run([exe, "--host", group, str(where)], capture_output=True, text=True, timeout=300)
        assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
        self.where = str(where)
        self.meta, self.sens = {}, {}
        for line in run.stdout.splitlines():
            f = dict(kv.split("=", 1) for kv in line.split()[1:])
            if line.startswith("host "):
                assert f["case"] not in self.meta
                self.meta[f["case"]] = f
            elif line.startswith("sens "):
                self.sens[(f["case"], f["pert"])] = float(f["ratio"])

    def load(self, case, name):
        kind = {"f32": "<f4", "f64": "<f8", "u8": "u1", "i32": "<i4"}[name.rsplit(".", 1)[1]]
        a = np.fromfile(os.path.join(self.where, f"{case}.{name}"), dtype=kind)
        return torch.from_numpy(a.astype(np.float64)) if kind in ("<f4", "<f8") else torch.from_numpy(a)


@pytest.fixture(scope="module", params=GROUPS)
def dumped(request, checker, tmp_path_factory):
    return request.param, Dumped(checker, request.param, tmp_path_factory.mktemp("xfmr_" + request.param))


def attention(qkv, heads, key_ok=None, causal=False):
    """qkv [S, 3 D] float64 -> softmax(q k^T / sqrt(hd) + mask) v, [S, D]"""
    s, d = qkv.shape[0], qkv.shape[1] // 3
    q, k, v = (qkv[:, i * d:(i + 1) * d].reshape(s, heads, d // heads).transpose(0, 1) for i in range(3))
    scores = q @ k.transpose(1, 2) / (d // heads) ** 0.5
    if key_ok is not None:
        scores = scores.masked_fill(~key_ok.bool()[None, None, :], float("-inf"))
    if causal:
        scores = scores + torch.full((s, s), float("-inf"), dtype=torch.float64).triu(1)
    return (torch.softmax(scores, dim=-1) @ v).transpose(0, 1).reshape(s, d)


def torch_reference(group, d, case):
    """{name of the dumped reference: the torch float64 statement}"""
    m = d.meta[case]
    if group in ("dec", "enc"):
        b, s, heads = int(m["B"]), int(m["S"]), int(m["heads"])
        qkv = d.load(case, "qkv.f32").reshape(b, s, 3 * D)
        ok = d.load(case, "mask.u8").reshape(b, s) if group == "enc" else [None] * b
        full = torch.stack([attention(qkv[i], heads, ok[i]) for i in range(b)])
        return {"ref.f64": full, "ref0.f64": full[:, 0]} if group == "enc" else {"ref.f64": full}
    if group == "clip":
        lens = [int(v) for v in m["lens"].split(",")]
        qkv = d.load(case, "qkv.f32").reshape(sum(lens), 3 * D)
        return {"ref.f64": torch.cat([attention(rows, int(m["heads"]), causal=True) for rows in qkv.split(lens)])}
    if group == "ln":
        rows, nbc = int(m["rows"]), int(m["bc"])
        x = d.load(case, "x.f32").reshape(rows, D)
        add = d.load(case, "bc.f32").reshape(nbc, D)[torch.arange(rows) // T] if nbc else 0.0
        if m["x2"] == "1":
            y1 = F.layer_norm(x, (D,), d.load(case, "w1.f32"), d.load(case, "b1.f32"), eps=1e-5)
            return {"ref.f64": F.layer_norm(y1 + add, (D,), d.load(case, "w2.f32"), d.load(case, "b2.f32"), eps=1e-5)}
        return {"ref.f64": F.layer_norm(x + add, (D,), d.load(case, "w1.f32"), d.load(case, "b1.f32"), eps=1e-5)}
    if group == "final":
        b, jf = int(m["B"]), int(m["JF"])
        xh, wf, bf = d.load(case, "xh.f32").reshape(b, T, D), d.load(case, "wf.f32").reshape(jf, D), d.load(case, "bf.f32")
        out = (xh @ wf.T + bf).transpose(1, 2)                     # [B, JF, T]
        if m["mask"] == "1":
            out = out * (d.load(case, "mask.u8").reshape(b, 1, T) != 0)
        return {"ref.f64": out}
    if group == "queries":
        b, jf, n_pre = int(m["B"]), int(m["JF"]), int(m["n_pre"])
        x, w = d.load(case, "x.f32").reshape(b, jf, T), d.load(case, "wmap.f32").reshape(D, jf + 1)
        mapped = x.transpose(1, 2) @ w[:, :jf].T + w[:, jf]       # [B, T, D]
        mapped = mapped * (torch.arange(T) < n_pre)[None, :, None]
        return {"ref.f64": mapped + d.load(case, "bmap.f32") + d.load(case, "pe.f32").reshape(T, D)}
    raise AssertionError(group)


def test_references_agree_with_torch_float64(dumped):
    group, d = dumped
    assert sorted(d.meta) == sorted(CASES[group])
    if group == "prepare":
        return check_prepare(d)
    worst = 0.0
    for case in CASES[group]:
        for name, want in torch_reference(group, d, case).items():
            got = d.load(case, name).reshape(want.shape)
            assert torch.isfinite(got).all() and torch.isfinite(want).all(), (case, name)
            rel = float((got - want).abs().max() / want.abs().max())
            worst = max(worst, rel)
            assert rel <= 1e-12, (case, name, rel)
    print(f"{group}: worst |ref - torch| / max|ref| = {worst:.3g}")


def check_prepare(d):
    """tok, xt and kmask are copies or single fp32 additions: the fp32 statement, compared exactly."""
    for case in CASES["prepare"]:
        m = d.meta[case]
        b, jf, kp = int(m["B"]), int(m["JF"]), int(m["KP"])
        f32 = lambda name: np.fromfile(os.path.join(d.where, f"{case}.{name}.f32"), dtype="<f4")
        x, pe = f32("x").reshape(b, jf, T), f32("pe").reshape(S_ENC, D)
        tok = np.broadcast_to(pe, (b, S_ENC, D)).copy()
        tok[:, 0] = pe[0] + f32("mu")                             # float32 + float32: the one addition the kernel makes
        tok[:, 1] = pe[1] + f32("sigma")
        xt = np.zeros((b, T, kp), dtype=np.float32)
        xt[:, :, :jf] = x.transpose(0, 2, 1)
        kmask = np.ones((b, S_ENC), dtype=np.uint8)
        if m["mask"] == "1":
            kmask[:, 2:] = d.load(case, "mask.u8").numpy().reshape(b, T) != 0
            assert (kmask == 0).any()
        assert np.array_equal(f32("tok").view(np.uint32), tok.reshape(-1).view(np.uint32)), case
        assert np.array_equal(f32("xt").view(np.uint32), xt.reshape(-1).view(np.uint32)), case
        assert np.array_equal(d.load(case, "kmask.u8").numpy(), kmask.reshape(-1)), case


def test_the_bounds_reject_the_known_wrong_references(dumped):
    group, d = dumped
    asked = {(case, p) for case in CASES[group] for p in required_perturbations(group, case)}
    assert asked <= set(d.sens), sorted(asked - set(d.sens))
    if asked:
        case, p = min(asked, key=lambda k: d.sens[k])
        print(f"{group}: {len(asked)} (case, wrong reference) pairs, the least detected is {p} on {case}: {d.sens[(case, p)]:.4g} bounds")
    assert [(k, d.sens[k]) for k in sorted(asked) if not d.sens[k] >= 4.0] == []


def test_the_inputs_are_what_the_cases_say(dumped):
    """The edges the cases are there for are in the data: score magnitudes, the masks, the low-variance and large-mean rows."""
    group, d = dumped
    if group == "dec":
        for case, lo, hi in (("dec_b3", 3.0, 8.0), ("dec_big_b2", 70.0, 140.0)):
            qkv = d.load(case, "qkv.f32").reshape(-1, T, 3, 4, 128)
            top = float(torch.einsum("bshd,bthd->bhst", qkv[:, :, 0], qkv[:, :, 1]).abs().max() / 128 ** 0.5)
            assert lo <= top <= hi, (case, top)
    if group == "clip":
        qkv = d.load("clip_big", "qkv.f32").reshape(-1, 3, 8, 64)[:77]
        top = float(torch.einsum("shd,thd->hst", qkv[:, 0], qkv[:, 1]).tril().abs().max() / 8.0)
        assert 70.0 <= top <= 140.0, top
        qk = d.load("clip_probe", "qkv.f32").reshape(-1, 3, D)[:, :2]
        assert set(qk.unique().tolist()) == {-1.0, 0.0, 1.0}        # integer q and k under the scale 1/8: exact scores
    if group == "enc":
        for k in (2, 15, 16, 17, 31, 32, 33, 35):
            mask = d.load(f"enc_m{k}", "mask.u8").reshape(2, S_ENC)
            assert (mask[0] == 0).nonzero().flatten().tolist() == [k] and (mask[1] != 0).all()
            kv = d.load(f"enc_m{k}", "qkv.f32").reshape(2, S_ENC, 3, D)[0, k, 1:]
            assert (kv.abs() == 7.0).all()
        assert (d.load("enc_only01", "mask.u8").reshape(2, S_ENC)[0] != 0).nonzero().flatten().tolist() == [0, 1]
        tail = d.load("enc_tail17", "mask.u8").reshape(3, S_ENC) != 0
        assert tail.sum(1).tolist() == [19, 7, 35]
    if group == "ln":
        x = d.load("ln_bigmean_r5", "x.f32").reshape(5, D)
        assert (x.mean(1) - 1000).abs().max() < 0.01 and 0.008 < float(x.std(1).min()) and float(x.std(1).max()) < 0.012
        assert float(d.load("ln_const_r5", "x.f32").reshape(5, D).var(1, unbiased=False).max()) == 0.0
        var = d.load("ln_lowvar_r5", "x.f32").reshape(5, D).var(1, unbiased=False)
        assert 0.7e-4 < float(var.min()) and float(var.max()) < 1.4e-4
