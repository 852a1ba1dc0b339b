"""The cases of tools/xfmr_cases.h by group, and the known-wrong references every case must reject (tools/xfmr_ref.h).  Shared by
tests/test_xfmr_ref_host.py (CPU: references against torch float64, sensitivity of the bounds) and tests/test_gpu_xfmr.py (GPU: the kernels
against the references), so a case that vanishes from the checker's table fails both."""

GROUPS = ("dec", "enc", "clip", "ln", "final", "queries", "prepare")

CLIP_LENGTHS = (1, 2, 15, 16, 17, 31, 32, 33, 48, 49, 64, 65, 77, 80)
ENC_MASKED_KEYS = (2, 15, 16, 17, 31, 32, 33, 35)
FINAL_JF = (1, 16, 17, 27, 32, 33, 282)

CASES = {
    "dec": ["dec_b1", "dec_b3", "dec_c4_b3", "dec_c1_b3", "dec_c4_b1", "dec_big_b2"],
    "enc": ["enc_ones", "enc_only01"] + [f"enc_m{k}" for k in ENC_MASKED_KEYS] + ["enc_tail17"],
    "clip": [f"clip_l{n}" for n in CLIP_LENGTHS] + ["clip_mix64", "clip_mix80", "clip_trunc80", "clip_kv_above", "clip_big", "clip_probe"],
    "ln": [f"ln_r{r}" for r in (1, 3, 4, 5, 103)] + ["ln_bigmean_r5", "ln_const_r5", "ln_lowvar_r5", "ln_times1e4_r5", "ln_times1em4_r5", "ln_mixed_r103",
                                                      "ln_bc512_r103", "ln_bc1536_r103", "ln_x2_bc512_r103", "ln_x2_bc1536_r5", "ln_x2_bc512_r4",
                                                      "ln_x2_mixed_r103"],
    "final": [f"fin_jf{jf}_b{b}_{m}" for jf in FINAL_JF for b in (1, 3) for m in ("null", "ones", "clr")],
    "queries": [f"qry_n{n}_b{b}{qc}" for n in (0, 4, 34) for b in (1, 3) for qc in ("", "_qc")] + ["qry_jf282_n4_b3_qc"],
    "prepare": ["prep_jf27_null", "prep_jf282_null", "prep_jf27_mask", "prep_jf282_mask"],
}

# the cases whose line must carry a bitwise claim (`same=ok`), and the masked outputs that must be exactly +0 (`zero=ok`)
SAME = (["dec_c4_b3", "dec_c1_b3", "dec_c4_b1"] + CASES["enc"] + ["clip_mix64", "clip_mix80", "clip_trunc80", "clip_kv_above"] +
        [n for n in CASES["ln"] if "_x2_" in n] + [n for n in CASES["queries"] if n.endswith("_qc")] + CASES["prepare"])
ZERO = [n for n in CASES["final"] if not n.endswith("_null")]


def required_perturbations(group, name):
    """The wrong references that apply to a case: each must lie at least 4 bounds away from the true one somewhere in the case.

    Where one does not apply, the operation cannot tell it from the true form: a single key has probability 1 under any scale; with
    scores near 80 (`big`) the dropped key's probability is far below fp64's own resolution of the result; all-ones shifted is all
    ones; eps is asked on the low-variance rows only, where it is a tenth of the variance; bc[r / 36] equals bc[r / 34] below row 34;
    the unbiased variance cannot show on a constant row (x - mean = 0), under a mean 1e5 times the spread (the honest error of the
    mean is larger than the spread) or where eps is 1000 times the variance."""
    if group == "dec":
        return ["q_unscaled", "scale_1_hd", "v_next_head"] + ([] if "_big" in name else ["drop_last", "drop_least"])
    if group == "enc":
        return ["q_unscaled", "scale_1_hd", "drop_last", "drop_least", "v_next_head"] + ([] if name == "enc_ones" else ["mask_shift"])
    if group == "clip":
        if name in ("clip_l1", "clip_probe"):
            return ["v_next_head"]
        if name == "clip_big":
            return ["q_unscaled", "scale_1_hd", "v_next_head"]
        return ["q_unscaled", "scale_1_hd", "drop_last", "drop_least", "causal_excl", "causal_incl", "v_next_head"]
    if group == "ln":
        need = [] if any(k in name for k in ("bigmean", "const", "times1em4")) else ["unbiased_var"]
        if "lowvar" in name:
            need += ["eps_1e-6", "eps_omitted"]
        if "_bc" in name and name.endswith("r103") or name == "ln_x2_mixed_r103":
            need += ["bc_div_36"]
        return need
    if group == "final":
        return ["no_bias"] + (["mask_shift"] if name.endswith("_clr") else [])
    if group == "queries":
        return ([] if "_n0_" in name else ["no_bit"]) + ["pe_next_row"]
    return []
