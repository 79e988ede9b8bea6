// tests/ks_group_emul/ks_group_emul.cpp -- CPU emulation of the per-coefficient bodies of the grouped key switch
// (toyfhe.jl_amd/csrc/ks_group_core.h): the digit body (ks_group_prepare / ks_group_eval over the tables build_conv_host makes, the way
// k_ks_group_digits<G> strings them together, a group cut short included), the tail body (ks_group_tail_special / ks_group_tail_limb in
// the order of k_ks_group_tail<K>), lift_digit and the k_ks_rescale_add formula to compare them with, and the entry points' host checks.
// TEST INFRASTRUCTURE ONLY.
#include <cstdint>
#include <cstring>
#include <vector>

#define TFHE_EMUL_COUNT_SLOW 1
static long g_slow_hits = 0;
#include "../../toyfhe.jl_amd/csrc/bfv_tables.h"
#include "../../toyfhe.jl_amd/csrc/ntt_core.h"
#include "../../toyfhe.jl_amd/csrc/ks_group_core.h"

namespace {

// one coefficient: x [k] -> out [m]
template <int G>
void digit(const conv_tab_t& T, const u64* x, u64* out) {
    ks_group_digit_t<G> D;
    constexpr int GG = G ? G : TFHE_MAX_LIMBS;
    for (int j = 0; j < GG; j++) D.xi[j] = x[j < T.k ? j : T.k - 1];   // spare registers repeat the last limb, as the kernel's do
    ks_group_prepare<G>(T, D);
    for (int i = 0; i < T.m; i++) out[i] = ks_group_eval<G>(T, D, i);
}

template <int K>
void tail(int level, const barrett_t* qb, const barrett_t* pb, const tw_t (*inv)[TFHE_MAX_LIMBS], const u64* t, u64* out) {
    u64 y[K];
    for (int u = 0; u < K; u++) y[u] = t[level + u];
    ks_group_tail_special<K>(y, pb, inv, level);
    for (int j = 0; j < level; j++) out[j] = ks_group_tail_limb<K>(t[j], y, qb[j], inv, j);
}

}  // namespace

extern "C" {

// The digit body with G residues in registers (0: the run-time loop) on `count` coefficients: source moduli a [k] (k <= G unless
// G = 0), targets t [m], x [count][k] -> out [count][m].  Returns the number of times conv_prepare took its exact multi-word
// branch, or -1 for a bad shape.
long ks_group_emul_digits(int G, int k, const uint64_t* a, int m, const uint64_t* t, long count, const uint64_t* x, uint64_t* out) {
    if (k < 1 || k > TFHE_MAX_LIMBS || m < 1 || m > TFHE_MAX_LIMBS || G < 0 || G > 4 || (G && k > G)) return -1;
    conv_host_t H;
    build_conv_host(std::vector<u64>(a, a + k), std::vector<u64>(t, t + m), &H);
    g_slow_hits = 0;
    for (long c = 0; c < count; c++) {
        const u64* xc = x + (size_t)c * k;
        u64* oc = out + (size_t)c * m;
        switch (G) {
            case 0: digit<0>(H.tab, xc, oc); break;
            case 1: digit<1>(H.tab, xc, oc); break;
            case 2: digit<2>(H.tab, xc, oc); break;
            case 3: digit<3>(H.tab, xc, oc); break;
            default: digit<4>(H.tab, xc, oc); break;
        }
    }
    return g_slow_hits;
}

// lift_digit of x mod qi into qj (the per-limb digit of tfhe_keyswitch)
uint64_t ks_group_emul_lift_digit(uint64_t x, uint64_t qi, uint64_t qj) {
    lift_t lf{};
    lf.qi = qi; lf.half = qi >> 1; lf.qj = qj; lf.bj = hostmath::make_barrett(qj);
    return lift_digit(x, lf);
}

// The tail body with K special primes on `count` coefficients: w [level + K] working moduli (the special primes last),
// t [count][level + K] -> out [count][level].  Returns 0, or -1 for a bad shape.
int ks_group_emul_tail(int K, int level, const uint64_t* w, long count, const uint64_t* t, uint64_t* out) {
    if (K < 1 || K > TFHE_KSG_MAX_SPECIAL || level < 1 || level + K > TFHE_MAX_LIMBS) return -1;
    static tw_t inv[TFHE_KSG_MAX_SPECIAL][TFHE_MAX_LIMBS];
    barrett_t qb[TFHE_MAX_LIMBS], pb[TFHE_KSG_MAX_SPECIAL];
    for (int j = 0; j < level; j++) qb[j] = hostmath::make_barrett(w[j]);
    for (int u = 0; u < K; u++) {
        pb[u] = hostmath::make_barrett(w[level + u]);
        for (int j = 0; j < level + u; j++) inv[u][j] = hostmath::make_tw(hostmath::invmod_prime(w[level + u] % w[j], w[j]), w[j]);
    }
    for (long c = 0; c < count; c++) {
        const u64* tc = t + (size_t)c * (level + K);
        u64* oc = out + (size_t)c * level;
        switch (K) {
            case 1: tail<1>(level, qb, pb, inv, tc, oc); break;
            case 2: tail<2>(level, qb, pb, inv, tc, oc); break;
            case 3: tail<3>(level, qb, pb, inv, tc, oc); break;
            default: tail<4>(level, qb, pb, inv, tc, oc); break;
        }
    }
    return 0;
}

// the words of k_ks_rescale_add for one coefficient and limb, without the addend: (tj - [tl] mod q) P^-1 mod q
uint64_t ks_group_emul_rescale_add(uint64_t tj, uint64_t tl, uint64_t q, uint64_t p) {
    const barrett_t br = hostmath::make_barrett(q);
    const tw_t pinv = hostmath::make_tw(hostmath::invmod_prime(p % q, q), q);
    return shoup_full(submod(tj, barrett_reduce128(tl, 0, br), q), pinv, q);
}

// the host checks of tfhe_keyswitch_grouped (rotate = 0) / tfhe_rotate_grouped on a ring of L limbs and degree N
int ks_group_emul_check(int any_null, int L, int64_t N, int Lk, int level, int k, int group, int n_digits, int polys, int64_t batch, int rotate,
                        uint64_t galois, char* msg, size_t cap) {
    return ks_group_check(any_null != 0, L, N, Lk, level, k, group, n_digits, polys, batch, rotate != 0, galois, msg, cap);
}

}  // extern "C"
