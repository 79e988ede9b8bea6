// tests/mdg_fold_emul/resource_probe.hip -- instantiates k_mdg_fold_finish<K, V> and k_mdg_fold_gather (csrc/ks_group_core.h), the
// kernels one evaluation-domain fold step on grouped-digit keys adds, the way mdg_fold_run launches them, so that
// tests/test_rotate_sum_grouped_cpu.py can read their register, scratch and LDS figures from
// `hipcc --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage`.  TEST INFRASTRUCTURE ONLY.
#include "../../toyfhe.jl_amd/csrc/kernels.h"

#define PROBE_FINISH(K, V) \
    template __global__ void k_mdg_fold_finish<K, V>(const u64*, const u64*, const u64*, u64*, const ntt_limb_t*, ks_group_arg_t, u32, u32, u32, u32);
#if !defined(PROBE_K)
#define PROBE_K 0
#endif
#if PROBE_K == 0 || PROBE_K == 1
PROBE_FINISH(1, 1) PROBE_FINISH(1, 2)
#endif
#if PROBE_K == 0 || PROBE_K == 2
PROBE_FINISH(2, 1) PROBE_FINISH(2, 2)
#endif
#if PROBE_K == 0 || PROBE_K == 3
PROBE_FINISH(3, 1) PROBE_FINISH(3, 2)
#endif
#if PROBE_K == 0 || PROBE_K == 4
PROBE_FINISH(4, 1) PROBE_FINISH(4, 2)
#endif
// (k_mdg_fold_gather is no template: every code object holds it as it is)
