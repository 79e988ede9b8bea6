// tests/mul_core_emul/resource_probe.hip -- instantiates every kernel tfhe_mul_relin adds (the u64 fused core, and the packed /
// squaring / NTT-input forms of k_bfv_core_fused), so that tests/test_mul_relin_cpu.py can read their register, scratch and LDS
// figures from `hipcc --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage`.  TEST INFRASTRUCTURE ONLY.
// -DPROBE_LB=<12|13|14> picks the ring degree and -DPROBE_FP=<0|1> the policy, so that the test can compile the pieces side by side.
// The set mirrors the dispatch of csrc/mul_api.inc (mr_core_fp / mr_core_int).
#include "../../toyfhe.jl_amd/csrc/kernels.h"
#include "../../toyfhe.jl_amd/csrc/mul_core.h"

#define INT_(LB, M) template __global__ void k_mul_core_int<LB, logt_for(LB), M>(u64*, u64*, const ntt_limb_t*, limb_sel_t, u32, core_alt_t);
#define FP_(LB, M) \
    template __global__ void k_bfv_core_fused<ArithFp, LB, logt_for(LB), false, M>(const u64*, const u64*, u64*, u64*, const ntt_limb_t*, limb_sel_t, u32, core_alt_t);
#if PROBE_FP
FP_(PROBE_LB, CORE_PACKED | CORE_SQUARE) FP_(PROBE_LB, CORE_PACKED | CORE_NTTIN) FP_(PROBE_LB, CORE_PACKED | CORE_SQUARE | CORE_NTTIN)
#if PROBE_LB < 14   // (the general form of a mixed ring at 2^14 is not fused: mul_api.inc)
FP_(PROBE_LB, CORE_PACKED)
#endif
#else
INT_(PROBE_LB, CORE_PACKED) INT_(PROBE_LB, CORE_PACKED | CORE_SQUARE) INT_(PROBE_LB, CORE_PACKED | CORE_NTTIN)
INT_(PROBE_LB, CORE_PACKED | CORE_SQUARE | CORE_NTTIN)
#endif
