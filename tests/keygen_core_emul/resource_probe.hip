// tests/keygen_core_emul/resource_probe.hip -- instantiates every fused kernel tfhe_evalkey_gen launches, so that
// tests/test_keygen_cpu.py can read their register, scratch and LDS figures from
// `hipcc --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage`.  TEST INFRASTRUCTURE ONLY.
// -DPROBE_LB=<12|13|14> picks the ring degree and -DPROBE_FP=<0|1> the policy, so that the test can compile the pieces side by side.
// The set mirrors the dispatch of csrc/keygen_api.inc (key_launch_fused).
#include "../../toyfhe.jl_amd/csrc/kernels.h"
#include "../../toyfhe.jl_amd/csrc/keygen_core.h"

#if PROBE_FP
typedef ArithFp PA;
#else
typedef ArithInt PA;
#endif
#define KEY_(LB, RAND) template __global__ void k_evalkey_fused<PA, LB, logt_for(LB), RAND>(const ntt_limb_t*, limb_sel_t, u32, key_arg_t, key_rand_t);
KEY_(PROBE_LB, false) KEY_(PROBE_LB, true)
