"""tools/build_variant.py spec: the six-wave 64x64 plane kernel with a clock read at each
phase boundary of sl_planes64_step.inc (a private build, variants/w6_phase.so; never the
shipped library).

The unsplit instance k_env_planes64_w6 keeps eight s_memtime values (low 32 bits, in
scalar registers) and lane 0 writes them after the epilogue to the env's 32 bytes of
scratch words [4B, 8B), which that kernel uses for nothing else.  tools/w6_phase_timing.py
runs it (planes64_waves=-6) and prints the table kept as profiles/w6_phase_timing.txt.

  0 wave start | 1 loads done (record, planes, goals; a uint16 entry's transpose)
  2 action done | 3 rule done | 4 start planes arrived | 5 scores done
  6 plane stores and planes_ok issued | 7 epilogue and reset queue done
"""
INC = "sl_planes64_step.inc"
PHASE = ("    u32 tph[8];\n"
         "#define SL_PHASE(k) do { __builtin_amdgcn_sched_barrier(0); "
         "tph[k] = (u32)__builtin_amdgcn_s_memtime(); "
         "__builtin_amdgcn_sched_barrier(0); } while (0)\n"
         "    SL_PHASE(0);\n")

VARIANTS = {
    "w6_phase": [
        (INC, "    const int lane = threadIdx.x;\n    lds_u32 *buf",
         "    const int lane = threadIdx.x;\n" + PHASE + "    lds_u32 *buf"),
        (INC, "    // the action (lane 0) on the cells round the agent, gathered",
         "    SL_PHASE(1);\n    // the action (lane 0) on the cells round the agent, gathered"),
        (INC, "    u32 PB[32];\n#pragma unroll\n    for (int q = 0; q < 32; q++) PB[q] = ps.stored(q)",
         "    SL_PHASE(2);\n    u32 PB[32];\n#pragma unroll\n"
         "    for (int q = 0; q < 32; q++) PB[q] = ps.stored(q)"),
        (INC, "    u32 PS[32];\n    wait_vm();\n",
         "    SL_PHASE(3);\n    u32 PS[32];\n    wait_vm();\n    SL_PHASE(4);\n"),
        (INC, "    const ScoreTotals tot = score_totals(pts, scr, pos, side);\n"
              "    __builtin_amdgcn_sched_barrier(0);\n",
         "    const ScoreTotals tot = score_totals(pts, scr, pos, side);\n"
         "    __builtin_amdgcn_sched_barrier(0);\n    SL_PHASE(5);\n"),
        (INC, "    if (ok != pok_all && lane == 0) st.planes_ok[b] = ok;\n",
         "    if (ok != pok_all && lane == 0) st.planes_ok[b] = ok;\n    SL_PHASE(6);\n"),
        (INC, "    if (fx.fuse_reset && reset && lane == 0) queue_reset(fx.scratch, st.B, a.step, b);\n    }\n",
         "    if (fx.fuse_reset && reset && lane == 0) queue_reset(fx.scratch, st.B, a.step, b);\n    }\n"
         "    SL_PHASE(7);\n"
         "    if (W6 && !SPLIT_EPI && lane == 0) {\n"
         "        u32 *tp = reinterpret_cast<u32 *>(fx.scratch + 4 * st.B + 4 * b);\n"
         "#pragma unroll\n"
         "        for (int k = 0; k < 8; k++) tp[k] = tph[k];\n"
         "    }\n"),
    ],
}
