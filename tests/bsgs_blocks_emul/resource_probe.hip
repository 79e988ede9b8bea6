// tests/bsgs_blocks_emul/resource_probe.hip -- instantiates the SEEDED accumulation kernels tfhe_matmul_bsgs_blocks launches for the
// inputs after the first of a chunk, so that tests/test_matmul_bsgs_blocks_cpu.py can read their register and scratch figures from
// `hipcc --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage`.  TEST INFRASTRUCTURE ONLY.
// The set mirrors the dispatch of csrc/md_api.inc (matmul_bsgs_run: output tiles of 1, 2 and 4 giant steps, both lift forms); the
// unseeded forms of input 0 are those of tests/bsgs_emul/resource_probe.hip.
#include "../../toyfhe.jl_amd/csrc/kernels.h"

#define PROBE_ACC(US, NG)                                                                                                                    \
    template __global__ void k_md_acc<US, NG, true>(const u64*, const u64*, const u64*, const u64*, u64*, const ntt_limb_t*, limb_sel_t, \
                                                    rot_tail_arg_t, rescale_arg_t, u32, u32, u32, u32, u32);
PROBE_ACC(false, 1) PROBE_ACC(false, 2) PROBE_ACC(false, 4) PROBE_ACC(true, 1) PROBE_ACC(true, 2) PROBE_ACC(true, 4)
#define PROBE_DENSE(NG) \
    template __global__ void k_md_acc_dense<NG, true>(const u64*, const u64*, const u64*, u64*, const ntt_limb_t*, limb_sel_t, u32, u32, u32, u32);
PROBE_DENSE(1) PROBE_DENSE(2) PROBE_DENSE(4)
