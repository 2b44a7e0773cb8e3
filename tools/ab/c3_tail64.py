# (timing record; applies to commit f82e1ae, the parent of the change that took the exit
# stores and the ring gather out of k_env_epilogue_reset64)
# C3 tail kernel: where k_env_epilogue_reset64's time goes (timing-only variants: all but
# t64_head compute wrong results).
#   t64_head     as committed
#   t64_noreset  no env is reset (the ballot is dropped; the epilogue still decides)
#   t64_noexit   no exit-colour stores into the uint16 board (nor their loads)
#   t64_noring   the ring entry is not read: the distance is taken from the agent itself
#   t64_nox_nor  t64_noexit and t64_noring together
H = "sl_bits.h"
K = "sl_bits.hip"
END = """    __device__ int agent_y() const { return ay; }
};

}  // namespace bits"""
NOEXIT = "    __device__ int exit_count() const { return 0; }\n"
NORING = ("    __device__ int prior_x(int) const { return ax; }\n"
          "    __device__ int prior_y(int) const { return ay; }\n")


def hand(extra):
    return [(H, END, END.replace("};", extra + "};", 1))]


VARIANTS = {
    "t64_head": [],
    "t64_noreset": [(K, "const uint64_t mine = __ballot(reset);",
                     "const uint64_t mine = __ballot(reset) & 0ull;")],
    "t64_noexit": hand(NOEXIT),
    "t64_noring": hand(NORING),
    "t64_nox_nor": hand(NOEXIT + NORING),
}
