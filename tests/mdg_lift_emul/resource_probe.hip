// tests/mdg_lift_emul/resource_probe.hip -- instantiates k_mdg_lift<K, V> and k_mdg_special_perm (csrc/ks_group_core.h), the kernels the
// evaluation-domain rotation phase on grouped-digit keys adds, the way mdg_rotations launches them, so that
// tests/test_matmul_bsgs_grouped_cpu.py can read their register, scratch and LDS figures from
// `hipcc --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage`.  TEST INFRASTRUCTURE ONLY.
#include "../../toyfhe.jl_amd/csrc/kernels.h"

#define PROBE_LIFT(K, V) template __global__ void k_mdg_lift<K, V>(const u64*, u64*, const ntt_limb_t*, ks_group_arg_t, u32, u32);
PROBE_LIFT(1, 1) PROBE_LIFT(2, 1) PROBE_LIFT(3, 1) PROBE_LIFT(4, 1)
PROBE_LIFT(1, 2) PROBE_LIFT(2, 2) PROBE_LIFT(3, 2) PROBE_LIFT(4, 2)
// (k_mdg_special_perm is no template: the code object holds it as it is)
