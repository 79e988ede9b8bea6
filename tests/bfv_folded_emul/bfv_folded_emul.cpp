// tests/bfv_folded_emul/bfv_folded_emul.cpp -- host build of the narrow BFV conversion bodies (csrc/bfv_fast.h) for
// tests/test_bfv_folded_cpu.py: the folded, three-product contraction next to the unfolded forms, the expansion, the
// constants kappa the producer folds in, the lane maxima that reached acc52_redc and the exact-alpha counts per conversion.
// TEST INFRASTRUCTURE ONLY: never loaded by the product package.
#include <cstdint>
#include <cstring>
#include <vector>

#define TFHE_EMUL_TRACK_NARROW 1
static unsigned long long g_narrow_lane_max[4];
static long g_narrow_exact_hits[17];
#include "../../toyfhe.jl_amd/csrc/bfv_tables.h"

namespace {

template <int S, int P_>
void run(const bfv_fast_tab_t& B, int mode, int64_t n, const u64* src, u64* dst) {
    u64 col[TFHE_FAST_MAX];
    for (int64_t k = 0; k < n; k++) {
        const u64* s = src + k;
        u64* d = dst + k;
        switch (mode) {
            case 0: bfv_expand_narrow<S, P_>(B, s, n, d, n, col, 1); break;
            case 1: bfv_contract_narrow<S, P_>(B, s, n, d, n, col, 1); break;
            case 2: bfv_contract_narrow<S, P_, true>(B, s, n, d, n, col, 1); break;
            case 3: bfv_contract_narrow<S, P_, true, true>(B, s, n, d, n, col, 1); break;
            case 4: bfv_contract_narrow<S, P_, true, true>(B, s, n, d, n, col, 1, true); break;   // c2's form: centred doubles out
        }
    }
}

}  // namespace

extern "C" {

// mode 0: expansion, src [ns][n] words -> dst [nb][n];  1 / 2 / 3 / 4: contraction of src [nb][n] -> dst [ns][n] from words / reduced
// doubles / folded doubles / folded doubles with lifted output.  lane_max[4], exact_hits[17] (indexed by the source limb count).
// Returns 0, -7 when the pair is outside the narrow fast path, -9 when (ns, np) is not one of the pairs built here.
int bfvf_run(const uint64_t* qs, int ns, const uint64_t* pb, int nb, uint64_t t, int mode, int64_t n, const uint64_t* src, uint64_t* dst,
             uint64_t* lane_max, int64_t* exact_hits) {
    bfv_fast_host_t* H = new bfv_fast_host_t();
    if (!build_bfv_fast_host(std::vector<u64>(qs, qs + ns), std::vector<u64>(pb, pb + nb), t, H) || !H->tab.narrow) { delete H; return -7; }
    memset(g_narrow_lane_max, 0, sizeof g_narrow_lane_max);
    memset(g_narrow_exact_hits, 0, sizeof g_narrow_exact_hits);
    int rc = -9;
    if (H->tab.ns == 2 && H->tab.np == 3) { run<2, 3>(H->tab, mode, n, src, dst); rc = 0; }
    if (H->tab.ns == 8 && H->tab.np == 9) { run<8, 9>(H->tab, mode, n, src, dst); rc = 0; }
    for (int i = 0; i < 4; i++) lane_max[i] = g_narrow_lane_max[i];
    for (int i = 0; i < 17; i++) exact_hits[i] = g_narrow_exact_hits[i];
    delete H;
    return rc;
}

// kappa[l] for the limbs of ℛbig in buffer order (bfv_fold_kappa), and what bfv_fold_limb makes of a limb's closing constants:
// folded[l] = ninv[l] kappa[l] mod pb[l] as the double the table holds
int bfvf_kappa(const uint64_t* qs, int ns, const uint64_t* pb, int nb, uint64_t t, const uint64_t* ninv, uint64_t* kappa, double* folded) {
    bfv_fast_host_t* H = new bfv_fast_host_t();
    if (!build_bfv_fast_host(std::vector<u64>(qs, qs + ns), std::vector<u64>(pb, pb + nb), t, H) || !H->tab.narrow) { delete H; return -7; }
    bfv_fold_kappa(H->tab, kappa);
    struct limb { u64 q; tw_t ninv, w1inv_ninv; ftw_t ninv_d, w1inv_ninv_d; };
    for (int l = 0; l < nb; l++) {
        limb L{pb[l], tw_t{}, tw_t{}, ftw_t{0}, ftw_t{0}};
        L.ninv.w = ninv[l];
        L.w1inv_ninv.w = ninv[l];
        bfv_fold_limb(&L, kappa[l]);
        folded[l] = L.ninv_d.w;
    }
    delete H;
    return 0;
}

}  // extern "C"
