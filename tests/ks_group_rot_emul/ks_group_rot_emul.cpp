// tests/ks_group_rot_emul/ks_group_rot_emul.cpp -- CPU emulation of what the hoisted rotations on grouped-digit keys add to
// toyfhe.jl_amd/csrc/ks_group_core.h: the per-coefficient body of k_ks_group_rot_tail<K> (ks_group_rot_tail_coeff) over whole rows in
// the kernel's order -- coefficient i read in place, stored at g i mod N with the sign of floor(g i / N) --, the digit bodies
// (ks_group_prepare / ks_group_eval) over a whole polynomial for the commutation identity, and the host checks of
// tfhe_rotate_many_grouped / tfhe_matmul_diag_grouped (ks_group_many_check) on plain numbers.  TEST INFRASTRUCTURE ONLY.
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../toyfhe.jl_amd/csrc/bfv_tables.h"
#include "../../toyfhe.jl_amd/csrc/ntt_core.h"
#include "../../toyfhe.jl_amd/csrc/ks_group_core.h"

namespace {

template <int K>
void rot_tail(int level, size_t n, uint64_t g, const barrett_t* lb, const tw_t (*inv)[TFHE_MAX_LIMBS], const u64* t, const u64* c, u64* out) {
    const u64 mask2n = 2 * (u64)n - 1;
    for (size_t i = 0; i < n; i++) {
        const u64 p = ((u64)i * g) & mask2n;
        ks_group_rot_tail_coeff<K>(t + i, c ? c + i : nullptr, out, n, (u32)(p & (n - 1)), p >= n, level, lb, inv);
    }
}

template <int G>
void digit(const conv_tab_t& T, const u64* x, size_t stride, u64* out, size_t ostride) {
    ks_group_digit_t<G> D;
    constexpr int GG = G ? G : TFHE_MAX_LIMBS;
    for (int j = 0; j < GG; j++) D.xi[j] = x[(size_t)(j < T.k ? j : T.k - 1) * stride];
    ks_group_prepare<G>(T, D);
    for (int i = 0; i < T.m; i++) out[(size_t)i * ostride] = ks_group_eval<G>(T, D, i);
}

}  // namespace

extern "C" {

// One row group through the tail of a hoisted rotation with K special primes: w [level + K] working moduli (the special primes
// last), t [level + K][n] = INTT(S'), c [level][n] the addend or null, out [level][n]; n a power of two, g odd and below 2 n.
// Returns 0, or -1 for a bad shape.
int ks_group_rot_emul_tail(int K, int level, const uint64_t* w, long n, uint64_t g, const uint64_t* t, const uint64_t* c, uint64_t* out) {
    if (K < 0 || K > TFHE_KSG_MAX_SPECIAL || level < 1 || level + K > TFHE_MAX_LIMBS || n < 1 || (n & (n - 1)) || !(g & 1) || g >= 2 * (uint64_t)n) return -1;
    static tw_t inv[TFHE_KSG_MAX_SPECIAL][TFHE_MAX_LIMBS];
    barrett_t lb[TFHE_MAX_LIMBS];
    for (int j = 0; j < level + K; j++) lb[j] = hostmath::make_barrett(w[j]);
    for (int u = 0; u < K; u++)
        for (int j = 0; j < level + u; j++) inv[u][j] = hostmath::make_tw(hostmath::invmod_prime(w[level + u] % w[j], w[j]), w[j]);
    switch (K) {
        case 0: rot_tail<0>(level, (size_t)n, g, lb, inv, t, c, out); break;
        case 1: rot_tail<1>(level, (size_t)n, g, lb, inv, t, c, out); break;
        case 2: rot_tail<2>(level, (size_t)n, g, lb, inv, t, c, out); break;
        case 3: rot_tail<3>(level, (size_t)n, g, lb, inv, t, c, out); break;
        default: rot_tail<4>(level, (size_t)n, g, lb, inv, t, c, out); break;
    }
    return 0;
}

// The digit of one group over a whole polynomial, as k_ks_group_digits<G> strings the bodies together: source moduli a [k], targets
// tq [m], x [k][n] -> out [m][n].  Returns 0, or -1 for a bad shape.
int ks_group_rot_emul_digits(int G, int k, const uint64_t* a, int m, const uint64_t* tq, long n, const uint64_t* x, uint64_t* out) {
    if (k < 1 || k > TFHE_MAX_LIMBS || m < 1 || m > TFHE_MAX_LIMBS || G < 0 || G > 4 || (G && k > G)) return -1;
    conv_host_t H;
    build_conv_host(std::vector<u64>(a, a + k), std::vector<u64>(tq, tq + m), &H);
    for (long i = 0; i < n; i++) {
        switch (G) {
            case 0: digit<0>(H.tab, x + i, (size_t)n, out + i, (size_t)n); break;
            case 1: digit<1>(H.tab, x + i, (size_t)n, out + i, (size_t)n); break;
            case 2: digit<2>(H.tab, x + i, (size_t)n, out + i, (size_t)n); break;
            case 3: digit<3>(H.tab, x + i, (size_t)n, out + i, (size_t)n); break;
            default: digit<4>(H.tab, x + i, (size_t)n, out + i, (size_t)n); break;
        }
    }
    return 0;
}

// the host checks of tfhe_rotate_many_grouped (product = 0) / tfhe_matmul_diag_grouped on a ring of L limbs and degree N:
// key_null [n_rot] flags the null keys, galois [n_rot] the elements (both may be null when n_rot <= 0), ct / out / diags are
// addresses as numbers.  *nothing_to_do: the call returns TFHE_OK without work.
int ks_group_rot_emul_check(int product, int any_null, int L, int64_t N, int Lk, int level, int k, int group, int n_digits, int64_t batch,
                            const int* key_null, const uint64_t* galois, int n_rot, uint64_t ct, uint64_t out, uint64_t diags, int* nothing_to_do,
                            char* msg, size_t cap) {
    static const uint64_t some_key = 0;
    std::vector<const uint64_t*> evks((size_t)(n_rot > 0 ? n_rot : 0));
    for (size_t r = 0; r < evks.size(); r++) evks[r] = key_null[r] ? nullptr : &some_key;
    bool nothing = false;
    const int rc = ks_group_many_check(product != 0, any_null != 0, L, N, Lk, level, k, group, n_digits, batch, evks.data(), galois, n_rot,
                                       (uintptr_t)ct, (uintptr_t)out, (uintptr_t)diags, &nothing, msg, cap);
    *nothing_to_do = nothing ? 1 : 0;
    return rc;
}

}  // extern "C"
