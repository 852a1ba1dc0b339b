"""The kind of kernel each case of tools/gemm_cases.h was written for (csrc/ls_gemm_plan.h: gemm_kind_name).  Shared by
tests/test_gemm_plan_host.py (CPU: the plan of every case) and tests/test_gpu_gemm.py (GPU: the kind the checker reports), so a change
of the dispatch heuristics that moves a case to another kernel fails both until the case is re-aimed.

The LDS-DMA kernel needs whole 128-row tiles, so the 64-, 14400- and 20288-row products of the `dma` group stay on the general
kernel; the three DMA schedules are reached at 128, 14464 and 20352 rows (the same row counts padded to a tile, as the long path pads
them)."""

GROUPS = ("general", "fulltile", "dma", "dma_ln", "splitk")

_BY_KIND = {
    "general": {
        "general": """
            g_131x67x45_rr_vec g_131x67x45_rr_ld g_131x67x45_rr_off g_131x67x45_rc_vec g_131x67x45_rc_ld g_131x67x45_rc_off
            g_131x67x45_cr_vec g_131x67x45_cr_ld g_131x67x45_cr_off g_131x67x45_cc_vec g_131x67x45_cc_ld g_131x67x45_cc_off
            g_129x129x33_rr_vec g_129x129x33_rr_ld g_129x129x33_rr_off g_129x129x33_rc_vec g_129x129x33_rc_ld g_129x129x33_rc_off
            g_129x129x33_cr_vec g_129x129x33_cr_ld g_129x129x33_cr_off g_129x129x33_cc_vec g_129x129x33_cc_ld g_129x129x33_cc_off
            g_1x1x1_rr_vec g_1x1x1_rr_ld g_1x1x1_rr_off g_1x1x1_rc_vec g_1x1x1_rc_ld g_1x1x1_rc_off g_1x1x1_cr_vec g_1x1x1_cr_ld
            g_1x1x1_cr_off g_1x1x1_cc_vec g_1x1x1_cc_ld g_1x1x1_cc_off g_3x512x512_rr_vec g_3x512x512_rr_ld g_3x512x512_rr_off
            g_3x512x512_rc_vec g_3x512x512_rc_ld g_3x512x512_rc_off g_3x512x512_cr_vec g_3x512x512_cr_ld g_3x512x512_cr_off
            g_3x512x512_cc_vec g_3x512x512_cc_ld g_3x512x512_cc_off g_200x130x7_rr_vec g_200x130x7_rr_ld g_200x130x7_rr_off
            g_200x130x7_rc_vec g_200x130x7_rc_ld g_200x130x7_rc_off g_200x130x7_cr_vec g_200x130x7_cr_ld g_200x130x7_cr_off
            g_200x130x7_cc_vec g_200x130x7_cc_ld g_200x130x7_cc_off g_cvec_tail3 g_cvec_tail1 g_c_off1 g_a_rows2 g_a_rows2_vec
            g_b_k2 g_ab_k2 g_a_k2 g_c_rows2 g_c_rows2_vec g_c_t g_c_t_ld g_ep67_none g_ep67_bias g_ep67_cpre g_ep67_r g_ep67_acc
            g_ep67_inplace g_ep67_all g_ep67_act1 g_ep67_act2 g_ep67_act3 g_ep67_act4 g_ep68_none g_ep68_bias g_ep68_cpre g_ep68_r
            g_ep68_acc g_ep68_inplace g_ep68_all g_ep68_act1 g_ep68_act2 g_ep68_act3 g_ep68_act4 g_k32_act1 g_k32_act2 g_k32_act3
            g_k32_act4
        """,
    },
    "fulltile": {
        "full128": """
            f_256x128x64_rc f_128x256x96_rc f_256x128x64_cr f_128x256x96_cr f_256x128x64_cc f_128x256x96_cc f_plain f_inplace
            f_bias_off f_c_t
        """,
        "full64": """
            f_64row f_64row_acc f_64row_bias_off
        """,
    },
    "dma": {
        "dma_halves": """
            d_128_none d_128_bias d_128_cpre d_128_r d_128_inplace d_128_acc d_128_bias_off d_128_all d_128_act1 d_128_act2
            d_128_act3 d_128_act4 d_384x512x512 d_384_lda d_rows12288_128 d_rows0_128
        """,
        "general": """
            d_64x128x32 d_14400 d_rows12288_64 d_rows0_64 d_20288
        """,
        "dma_whole_halves": """
            d_14464
        """,
        "dma_whole": """
            d_20352
        """,
        "dma_3d": """
            d_batch3 d_batch3_acc d_split2
        """,
    },
    "dma_ln": {
        "dma_halves": """
            ln_rstd_probe ln_256 ln_256_last
        """,
        "dma_whole_halves": """
            ln_14464
        """,
    },
    "splitk": {
        "general": """
            s_131x67x200_rr s_131x67x200_cc s_131x67x200_rc s_131x67x200_cr s_512x37x300 s_512x37x300_cc s_req5_k96 s_tokmix
            s_tokmix_split s_wgrad_batch s_reject_act s_reject_cpre s_reject_r s_reject_ws
        """,
        "dma_3d": """
            s_128_dma
        """,
        "full128": """
            s_128_full_rc s_128_full_cc s_128_full_t
        """,
    },
}

# case name -> kind, and case name -> group
KIND = {name: kind for kinds in _BY_KIND.values() for kind, names in kinds.items() for name in names.split()}
GROUP = {name: group for group, kinds in _BY_KIND.items() for names in kinds.values() for name in names.split()}
