// tests/md_fold_emul/resource_probe.hip -- instantiates the two forms of the rotate-and-sum fold kernel (k_md_fold<USCALE>: the lifts
// scaled by P^-1 already, or in the term) that tfhe_rotate_sum and tfhe_matmul_bsgs_fold launch, so that tests/test_matmul_rect_cpu.py
// can read their register and scratch figures from `hipcc --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage`.
// TEST INFRASTRUCTURE ONLY.
#include "../../toyfhe.jl_amd/csrc/kernels.h"

#define PROBE_FOLD(US)                                                                                                                  \
    template __global__ void k_md_fold<US>(const u64*, const u64*, const u64*, u64*, const ntt_limb_t*, limb_sel_t, rot_tail_arg_t, \
                                           rescale_arg_t, u32, u32, u32, u32);
PROBE_FOLD(false) PROBE_FOLD(true)
