// Host-only driver of tests/test_gemm_plan_host.py: prints the plan (csrc/ls_gemm_plan.h) that launch_gemm_tr follows for every case of
// tools/gemm_cases.h and for the production shapes named in ls_gemm.hip.  Pointers are made-up aligned addresses; nothing is dereferenced.
#include <cstdint>
#include <cstdio>
#include "ls_gemm_plan.h"
#include "gemm_cases.h"

using namespace gemm_cases;

static float* fake(int slot, int off) { return reinterpret_cast<float*>((uintptr_t)0x10000000u * (unsigned)(slot + 1)) + off; }

static void show(const Case& c) {
    Ptrs p{};
    p.A = fake(0, c.A.off); p.B = fake(1, c.B.off); p.C = fake(2, c.offc); p.Cpre = fake(3, c.offc); p.R = fake(4, c.offc);
    p.bias = fake(5, c.bias_off);
    p.ln_part = fake(7, 0); p.wsum = fake(8, 0); p.addn = fake(9, 0); p.part_out = fake(10, 0);
    ls::GemmArgs a = make_args(c, p);
    const ls::GemmPlan first = ls::gemm_plan(a, c.A.kc, c.B.kc, c.splits);       // the workspace is sized from the re-derived split count
    const size_t need = ws_need(c, first.splits);
    a.ws = need ? fake(6, 0) : nullptr;
    a.ws_floats = need - (size_t)c.ws_short;
    const ls::GemmPlan g = ls::gemm_plan(a, c.A.kc, c.B.kc, c.splits);
    std::printf("case=%s group=%s kind=%s grid=%u,%u,%u gx=%d nbig=%d splits=%d kchunk=%d nbatch=%d fast=%d ws_too_small=%d split_epilogue=%d\n",
                c.name.c_str(), c.group.c_str(), ls::gemm_kind_name(g.kind), g.grid.x, g.grid.y, g.grid.z, g.gx, g.nbig, g.splits, g.kchunk,
                g.nbatch, (int)g.fast, (int)g.ws_too_small, (int)g.split_epilogue);
}

int main() {
    for (const Case& c : all_cases()) show(c);
    // production shapes (comments of ls_gemm.hip / ls_gemm_plan.h)
    show(mk("production", "p_17408x512x512", 17408, 512, 512, true, true).with_bias().with_r());       // the SAG decoder's out-proj / FFN2
    show(mk("production", "p_384x512x512", 384, 512, 512, true, true).with_bias().with_act(1));         // a 4-clip batch's channel mixing
    show(mk("production", "p_544_tiles", 17408, 512, 512, true, true).a_rows2(34, 37));                 // 544 tiles of 128 x 128, no LDS-DMA
    show(mk("production", "p_768_tiles", 12288, 512, 512, true, true));                                  // exactly LS_GEMM_HALF_MAX tiles: all halves
    show(mk("production", "p_776_tiles", 12416, 512, 512, true, true));                                  // one 128-row step more: 768 whole + 16 halves
    show(mk("production", "p_tokmix_long", 512, 34, 34, false, true).lda(512).batch(12, true).c_t().c_ld(512).with_bias().in_place().with_act(1));
    // a workspace with no pointer at all
    {
        Case c = mk("production", "p_no_ws", 131, 67, 200, true, true).split(3);
        Ptrs p{};
        p.A = fake(0, 0); p.B = fake(1, 0); p.C = fake(2, 0);
        ls::GemmArgs a = make_args(c, p);
        a.ws = nullptr; a.ws_floats = (size_t)1 << 30;
        const ls::GemmPlan g = ls::gemm_plan(a, true, true, c.splits);
        std::printf("case=%s group=%s kind=%s grid=%u,%u,%u gx=%d nbig=%d splits=%d kchunk=%d nbatch=%d fast=%d ws_too_small=%d split_epilogue=%d\n",
                    c.name.c_str(), c.group.c_str(), ls::gemm_kind_name(g.kind), g.grid.x, g.grid.y, g.grid.z, g.gx, g.nbig, g.splits, g.kchunk,
                    g.nbatch, (int)g.fast, (int)g.ws_too_small, (int)g.split_epilogue);
    }
    return 0;
}
