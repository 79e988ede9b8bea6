// tests/enc_core_emul/resource_probe.hip -- instantiates every fused kernel tfhe_encrypt / tfhe_decrypt_phase launch, so that
// tests/test_encrypt_cpu.py can read their register, scratch and LDS figures from
// `hipcc --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage`.  TEST INFRASTRUCTURE ONLY.
// -DPROBE_LB=<12|13|14> picks the ring degree and -DPROBE_FP=<0|1> the policy, so that the test can compile the pieces side by side.
// The set mirrors the dispatch of csrc/enc_api.inc (enc_launch_fused / dec_launch_fused).
#include "../../toyfhe.jl_amd/csrc/kernels.h"
#include "../../toyfhe.jl_amd/csrc/enc_core.h"

#if PROBE_FP
typedef ArithFp PA;
#else
typedef ArithInt PA;
#endif
#define ENC_(LB, RAND) \
    template __global__ void k_encrypt_fused<PA, LB, logt_for(LB), RAND>(u64*, const u64*, const u64*, const ntt_limb_t*, limb_sel_t, u32, u32, u32, enc_rand_t);
#define DEC_(LB, P, NI) \
    template __global__ void k_decrypt_fused<PA, LB, logt_for(LB), P, NI>(u64*, const u64*, const u64*, const ntt_limb_t*, limb_sel_t, u32, u32, u64);
#ifndef PROBE_ONLY   // (-DPROBE_ONLY=<1: encrypt | 2: decrypt>: one kernel family, for a quicker look)
#define PROBE_ONLY 0
#endif
#if PROBE_ONLY != 2
ENC_(PROBE_LB, false) ENC_(PROBE_LB, true)
#endif
#if PROBE_ONLY != 1
DEC_(PROBE_LB, 2, false) DEC_(PROBE_LB, 2, true) DEC_(PROBE_LB, 3, false)
#if PROBE_LB < 14   // (three NTT-domain components at 2^14 take the composed path: enc_api.inc)
DEC_(PROBE_LB, 3, true)
#endif
#endif
