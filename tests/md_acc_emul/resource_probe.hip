// tests/md_acc_emul/resource_probe.hip -- instantiates the accumulation kernels tfhe_matmul_diag, tfhe_matmul_bsgs and
// tfhe_matmul_bsgs_blocks launch, so that tests/test_matmul_bsgs_cpu.py (-DPROBE_SEED=0: the unseeded forms, input 0 of a chunk) and
// tests/test_matmul_bsgs_blocks_cpu.py (-DPROBE_SEED=1: the SEEDED forms of the inputs after the first) can read their register and
// scratch figures from `hipcc --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage`.  TEST INFRASTRUCTURE ONLY.
// The set mirrors the dispatch of csrc/md_api.inc (matmul_bsgs_run: output tiles of 1, 2 and 4 giant steps, both lift forms;
// tfhe_matmul_diag: tile 1).
#include "../../toyfhe.jl_amd/csrc/kernels.h"

#define PROBE_ACC(US, NG)                                                                                                            \
    template __global__ void k_md_acc<US, NG, PROBE_SEED != 0>(const u64*, const u64*, const u64*, const u64*, u64*, const ntt_limb_t*, \
                                                               limb_sel_t, rot_tail_arg_t, rescale_arg_t, u32, u32, u32, u32, u32);
PROBE_ACC(false, 1) PROBE_ACC(false, 2) PROBE_ACC(false, 4) PROBE_ACC(true, 1) PROBE_ACC(true, 2) PROBE_ACC(true, 4)
#define PROBE_DENSE(NG)                                                                                                                    \
    template __global__ void k_md_acc_dense<NG, PROBE_SEED != 0>(const u64*, const u64*, const u64*, u64*, const ntt_limb_t*, limb_sel_t, \
                                                                 u32, u32, u32, u32);
PROBE_DENSE(1) PROBE_DENSE(2) PROBE_DENSE(4)
