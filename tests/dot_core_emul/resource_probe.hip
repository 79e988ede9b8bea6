// tests/dot_core_emul/resource_probe.hip -- instantiates every fused kernel tfhe_dot_plain launches, so that
// tests/test_dot_plain_cpu.py can read their register, scratch and LDS figures from
// `hipcc --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage`.  TEST INFRASTRUCTURE ONLY.
// -DPROBE_LB=<12|13|14> picks the ring degree and -DPROBE_FP=<0|1> the policy, so that the test can compile the pieces side by side.
// The set mirrors the dispatch of csrc/dot_api.inc (dot_launch_fused).
#include "../../toyfhe.jl_amd/csrc/kernels.h"
#include "../../toyfhe.jl_amd/csrc/dot_core.h"

#if PROBE_FP
typedef ArithFp PA;
#else
typedef ArithInt PA;
#endif
template __global__ void k_dot_plain_fused<PA, PROBE_LB, logt_for(PROBE_LB)>(dot_view_arg_t, const u64*, u64, u64*, u64, u64*, u32, u32, const ntt_limb_t*,
                                                                            limb_sel_t, limb_sel_t, u32);
