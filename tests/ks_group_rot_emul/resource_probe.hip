// tests/ks_group_rot_emul/resource_probe.hip -- instantiates k_ks_group_rot_tail<K> (csrc/ks_group_core.h), the tail of the hoisted
// rotations on grouped-digit keys, for K = 0..4 special primes the way tfhe_rotate_many_grouped launches it, so that
// tests/test_rotate_many_grouped_cpu.py can read its register, scratch and LDS figures from
// `hipcc --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage`.  TEST INFRASTRUCTURE ONLY.
#include "../../toyfhe.jl_amd/csrc/kernels.h"

#define PROBE_ROT_TAIL(K) \
    template __global__ void k_ks_group_rot_tail<K>(const u64*, const u64*, u64*, const ntt_limb_t*, ks_group_arg_t, ks_group_rot_t, u32, u32, u32);
PROBE_ROT_TAIL(0) PROBE_ROT_TAIL(1) PROBE_ROT_TAIL(2) PROBE_ROT_TAIL(3) PROBE_ROT_TAIL(4)
