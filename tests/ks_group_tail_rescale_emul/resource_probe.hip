// tests/ks_group_tail_rescale_emul/resource_probe.hip -- instantiates the tail of tfhe_mul_relin_grouped (csrc/ks_group_core.h) the
// way ksg_chunk launches it -- k_ks_group_tail_rescale<K, V> for K = 1..4 special primes, each with one and with two coefficients per
// thread -- so that tests/test_mul_relin_grouped_cpu.py can read their register and scratch figures from
// `hipcc --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage`.  TEST INFRASTRUCTURE ONLY.
#include "../../toyfhe.jl_amd/csrc/kernels.h"

#define PROBE_TAIL_RESCALE(K, V)                                                                                                         \
    template __global__ void k_ks_group_tail_rescale<K, V>(const u64*, const u64*, u64*, const ntt_limb_t*, ks_group_arg_t, ks_group_rescale_t, \
                                                           u32, u32);
PROBE_TAIL_RESCALE(1, 1) PROBE_TAIL_RESCALE(2, 1) PROBE_TAIL_RESCALE(3, 1) PROBE_TAIL_RESCALE(4, 1)
PROBE_TAIL_RESCALE(1, 2) PROBE_TAIL_RESCALE(2, 2) PROBE_TAIL_RESCALE(3, 2) PROBE_TAIL_RESCALE(4, 2)
