// tests/plain_emul/plain_emul.cpp -- CPU emulation of the plaintext-codec bodies (toyfhe.jl_amd/csrc/plain_core.h).
//
// TEST INFRASTRUCTURE ONLY: never loaded by the product package.  The same per-coefficient bodies and the same host table the
// HIP kernels of plain_api.inc use, run one coefficient at a time with the compile-time limb bound the device dispatch picks
// (plain_km), so the oracle comparisons of tests/test_plain_codec_cpu.py cover the code that runs on the MI355X.
#include <cstdint>
#include <string>
#include <vector>

static long g_plain_hits[4] = {0, 0, 0, 0};
static double g_fp_max_ratio = 0;  // fp64arith.h TFHE_TRACK (bfv_tables.h pulls it in)
#include "../../toyfhe.jl_amd/csrc/plain_tables.h"

namespace {

template <int KM>
void run(const plain_tab_t& P, int op, const uint64_t* in, uint64_t* out, long count) {
    const int k = P.cv.k;
    for (long c = 0; c < count; c++) {
        switch (op) {
            case 0: out[c] = plain_bfv_decode_coeff<KM>(P, in + c * k, 1); break;
            case 1: out[c] = plain_bgv_decode_coeff<KM>(P, in + c * k, 1); break;
            case 2: {
                u64 w[KM];
                plain_noise_coeff<KM>(P, in + c * k, 1, w);
                for (int i = 0; i < KM; i++) out[c * TFHE_MAX_LIMBS + i] = w[i];
                for (int i = KM; i < TFHE_MAX_LIMBS; i++) out[c * TFHE_MAX_LIMBS + i] = 0;
                break;
            }
            case 3: plain_encode_coeff(P, 0, in[c], out + c * k, 1); break;
            case 4: plain_encode_coeff(P, 1, in[c], out + c * k, 1); break;
        }
    }
}

}  // namespace

extern "C" {

// the compile-time limb bound the device dispatch uses for k limbs (plain_api.inc plain_km)
int plain_emul_km(int k) { return k <= 1 ? 1 : k <= 2 ? 2 : k <= 4 ? 4 : k <= 8 ? 8 : k <= 16 ? 16 : TFHE_MAX_LIMBS; }

// op 0 BFV decode, 1 BGV decode: in [count][k] residues -> out [count]
// op 2 noise remainder: in [count][k] -> out [count][TFHE_MAX_LIMBS] words
// op 3 BFV encode, 4 BGV encode: in [count] plaintext words -> out [count][k] residues
// km: the compile-time bound (0 = the dispatch's choice).  Returns 0, or -1 for a rejected (qs, t); hits[4] counts the
// rare branches (quotient corrected down / up, exact tie, exact-α decision).
int plain_emul_run(const uint64_t* qs, int k, uint64_t t, int op, int km, const uint64_t* in, uint64_t* out, long count, long* hits) {
    plain_host_t* H = new plain_host_t();
    std::string err;
    if (build_plain_host(std::vector<u64>(qs, qs + k), t, H, &err)) { delete H; return -1; }
    H->tab.cv = H->cv.tab;
    for (int i = 0; i < 4; i++) g_plain_hits[i] = 0;
    if (km == 0) km = plain_emul_km(k);
    if (km < k) { delete H; return -2; }
    switch (km) {
        case 1: run<1>(H->tab, op, in, out, count); break;
        case 2: run<2>(H->tab, op, in, out, count); break;
        case 4: run<4>(H->tab, op, in, out, count); break;
        case 8: run<8>(H->tab, op, in, out, count); break;
        case 16: run<16>(H->tab, op, in, out, count); break;
        case TFHE_MAX_LIMBS: run<TFHE_MAX_LIMBS>(H->tab, op, in, out, count); break;
        default: delete H; return -2;
    }
    if (hits)
        for (int i = 0; i < 4; i++) hits[i] = g_plain_hits[i];
    delete H;
    return 0;
}

}  // extern "C"
