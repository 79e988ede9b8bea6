// tests/ks_group_emul/resource_probe.hip -- instantiates the kernels of the grouped key switch (csrc/ks_group_core.h) the way
// tfhe_keyswitch_grouped launches them -- k_ks_group_digits<G, V> for G = 1..4 residues in registers and G = 0, the run-time loop,
// k_ks_group_tail<K, V> for K = 1..4 special primes, each with one and with two coefficients per thread -- so that
// tests/test_ks_grouped_cpu.py can read their register and scratch figures from
// `hipcc --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage`.  TEST INFRASTRUCTURE ONLY.
#include "../../toyfhe.jl_amd/csrc/kernels.h"

#define PROBE_DIGITS(G, V) \
    template __global__ void k_ks_group_digits<G, V>(const u64*, u64*, const conv_tab_t*, ks_group_arg_t, u32, u32);
#define PROBE_TAIL(K, V) \
    template __global__ void k_ks_group_tail<K, V>(const u64*, const u64*, u64*, const ntt_limb_t*, ks_group_arg_t, u32, u32, u32);
PROBE_DIGITS(1, 1) PROBE_DIGITS(2, 1) PROBE_DIGITS(3, 1) PROBE_DIGITS(4, 1) PROBE_DIGITS(0, 1)
PROBE_DIGITS(1, 2) PROBE_DIGITS(2, 2) PROBE_DIGITS(3, 2) PROBE_DIGITS(4, 2) PROBE_DIGITS(0, 2)
PROBE_TAIL(1, 1) PROBE_TAIL(2, 1) PROBE_TAIL(3, 1) PROBE_TAIL(4, 1)
PROBE_TAIL(1, 2) PROBE_TAIL(2, 2) PROBE_TAIL(3, 2) PROBE_TAIL(4, 2)
