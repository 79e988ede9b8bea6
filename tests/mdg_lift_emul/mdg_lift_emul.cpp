// tests/mdg_lift_emul/mdg_lift_emul.cpp -- CPU emulation of what the evaluation-domain rotation phase on grouped-digit keys adds to
// toyfhe.jl_amd/csrc/ks_group_core.h: the per-coefficient body of k_mdg_lift<K, V> (mdg_lift_coeff) over whole rows, the factor
// Pinv_j = prod_t p_t^-1 mod q_j the key sums' epilogue multiplies by (as mdg_plan builds it), and the host checks of
// tfhe_matmul_bsgs_grouped (ks_group_bsgs_check) on plain numbers.  TEST INFRASTRUCTURE ONLY.
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../toyfhe.jl_amd/csrc/bfv_tables.h"
#include "../../toyfhe.jl_amd/csrc/ntt_core.h"
#include "../../toyfhe.jl_amd/csrc/ks_group_core.h"

namespace {

template <int K>
void lift_rows(int level, size_t n, const barrett_t* lb, const tw_t (*inv)[TFHE_MAX_LIMBS], const u64* p, u64* u) {
    for (size_t i = 0; i < n; i++) mdg_lift_coeff<K>(p + i, u + i, n, level, lb, inv);
}

}  // namespace

extern "C" {

// One row group through the lift with K special primes: w [level + K] working moduli (the special primes last), p [K][n] the special
// words (coefficient domain, canonical), u [level][n] out, pinv [level] out (Pinv_j).  Returns 0, or -1 for a bad shape.
int mdg_lift_emul_rows(int K, int level, const uint64_t* w, long n, const uint64_t* p, uint64_t* u, uint64_t* pinv) {
    if (K < 1 || K > TFHE_KSG_MAX_SPECIAL || level < 1 || level + K > TFHE_MAX_LIMBS || n < 1) return -1;
    static tw_t inv[TFHE_KSG_MAX_SPECIAL][TFHE_MAX_LIMBS];
    barrett_t lb[TFHE_MAX_LIMBS];
    for (int j = 0; j < level + K; j++) lb[j] = hostmath::make_barrett(w[j]);
    for (int t = 0; t < K; t++)
        for (int j = 0; j < level + t; j++) inv[t][j] = hostmath::make_tw(hostmath::invmod_prime(w[level + t] % w[j], w[j]), w[j]);
    for (int j = 0; j < level; j++) {
        u64 x = 1 % w[j];
        for (int t = 0; t < K; t++) x = hostmath::mulmod_slow(x, inv[t][j].w, w[j]);
        pinv[j] = x;
    }
    switch (K) {
        case 1: lift_rows<1>(level, (size_t)n, lb, inv, p, u); break;
        case 2: lift_rows<2>(level, (size_t)n, lb, inv, p, u); break;
        case 3: lift_rows<3>(level, (size_t)n, lb, inv, p, u); break;
        default: lift_rows<4>(level, (size_t)n, lb, inv, p, u); break;
    }
    return 0;
}

// the host checks of tfhe_matmul_bsgs_grouped on a ring of L limbs and degree N: baby_null [n_baby] / giant_null [n_giant] flag the
// null keys, diag_addr / ct_addr [n_in] are the operands' addresses as numbers (0: null); bias / out are addresses as numbers.
// *nothing_to_do: the call returns TFHE_OK without work.
int mdg_lift_emul_check(int any_null, int L, int64_t N, int Lk, int level, int k, int group, int n_digits, int64_t batch, const int* baby_null,
                        const uint64_t* baby_galois, int n_baby, const int* giant_null, const uint64_t* giant_galois, int n_giant,
                        const uint64_t* diag_addr, const uint64_t* ct_addr, int n_in, uint64_t bias, uint64_t out, int* nothing_to_do, char* msg,
                        size_t cap) {
    static const uint64_t some_key = 0;
    const auto count = [](int n) { return (size_t)(n < 0 ? 0 : (n > 64 ? 64 : n)); };
    std::vector<const uint64_t*> bk(count(n_baby) + 1), gk(count(n_giant) + 1), dg(count(n_in) + 1), ct(count(n_in) + 1);
    for (size_t r = 0; r < count(n_baby); r++) bk[r] = baby_null[r] ? nullptr : &some_key;
    for (size_t r = 0; r < count(n_giant); r++) gk[r] = giant_null[r] ? nullptr : &some_key;
    for (size_t m = 0; m < count(n_in); m++) {
        dg[m] = (const uint64_t*)(uintptr_t)diag_addr[m];
        ct[m] = (const uint64_t*)(uintptr_t)ct_addr[m];
    }
    bool nothing = false;
    const int rc = ks_group_bsgs_check(any_null != 0, L, N, Lk, level, k, group, n_digits, batch, bk.data(), baby_galois, n_baby, gk.data(),
                                       giant_galois, n_giant, dg.data(), ct.data(), n_in, (uintptr_t)bias, (uintptr_t)out, &nothing, msg, cap);
    *nothing_to_do = nothing ? 1 : 0;
    return rc;
}

}  // extern "C"
