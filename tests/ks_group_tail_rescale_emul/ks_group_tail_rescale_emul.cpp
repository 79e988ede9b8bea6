// tests/ks_group_tail_rescale_emul/ks_group_tail_rescale_emul.cpp -- CPU emulation of the per-coefficient body of the tail of
// tfhe_mul_relin_grouped (toyfhe.jl_amd/csrc/ks_group_core.h): ks_group_tail_special, ks_group_tail_last and
// ks_group_tail_rescale_limb in the order of k_ks_group_tail_rescale<K> -- the K special words, the rescale's `last` from limb
// level - 1, then the limbs below it one at a time -- and the entry point's host checks on plain numbers.  TEST INFRASTRUCTURE ONLY.
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../toyfhe.jl_amd/csrc/bfv_tables.h"
#include "../../toyfhe.jl_amd/csrc/ntt_core.h"
#include "../../toyfhe.jl_amd/csrc/ks_group_core.h"

namespace {

// one coefficient of one component: t [level + K] (the inverse-transformed key sums), c [level] (the addends) -> out [level - 1]
template <int K>
void tail_rescale(int level, const barrett_t* qb, const barrett_t* pb, const tw_t (*inv)[TFHE_MAX_LIMBS], const tw_t* qlinv, const u64* t, const u64* c,
                  u64* out) {
    u64 y[K];
    for (int u = 0; u < K; u++) y[u] = t[level + u];
    ks_group_tail_special<K>(y, pb, inv, level);
    const u64 last = ks_group_tail_last<K>(t[level - 1], c[level - 1], y, qb[level - 1], inv, level);
    for (int j = 0; j < level - 1; j++) out[j] = ks_group_tail_rescale_limb<K>(t[j], c[j], y, last, qb[j], inv, qlinv[j], j);
}

}  // namespace

extern "C" {

// The body with K special primes on `count` coefficients: w [level + K] working moduli (the special primes last),
// t [count][level + K], c [count][level] -> out [count][level - 1].  Returns 0, or -1 for a bad shape.
int ks_group_tail_rescale_emul(int K, int level, const uint64_t* w, long count, const uint64_t* t, const uint64_t* c, uint64_t* out) {
    if (K < 1 || K > TFHE_KSG_MAX_SPECIAL || level < 2 || level + K > TFHE_MAX_LIMBS) return -1;
    static tw_t inv[TFHE_KSG_MAX_SPECIAL][TFHE_MAX_LIMBS];
    barrett_t qb[TFHE_MAX_LIMBS], pb[TFHE_KSG_MAX_SPECIAL];
    ks_group_rescale_t R{};
    for (int j = 0; j < level; j++) qb[j] = hostmath::make_barrett(w[j]);
    for (int j = 0; j < level - 1; j++) R.qlinv[j] = hostmath::make_tw(hostmath::invmod_prime(w[level - 1] % w[j], w[j]), w[j]);
    for (int u = 0; u < K; u++) {
        pb[u] = hostmath::make_barrett(w[level + u]);
        for (int j = 0; j < level + u; j++) inv[u][j] = hostmath::make_tw(hostmath::invmod_prime(w[level + u] % w[j], w[j]), w[j]);
    }
    for (long i = 0; i < count; i++) {
        const u64* ti = t + (size_t)i * (level + K);
        const u64* ci = c + (size_t)i * level;
        u64* oi = out + (size_t)i * (level - 1);
        switch (K) {
            case 1: tail_rescale<1>(level, qb, pb, inv, R.qlinv, ti, ci, oi); break;
            case 2: tail_rescale<2>(level, qb, pb, inv, R.qlinv, ti, ci, oi); break;
            case 3: tail_rescale<3>(level, qb, pb, inv, R.qlinv, ti, ci, oi); break;
            default: tail_rescale<4>(level, qb, pb, inv, R.qlinv, ti, ci, oi); break;
        }
    }
    return 0;
}

// the host checks of tfhe_mul_relin_grouped on a ring of L limbs and degree N = 2^logN; c1 / c2 / out: addresses, never followed.
// *nothing: 1 where the call returns TFHE_OK without work.
int ks_group_tail_rescale_emul_check(int any_null, int L, int64_t N, int logN, int Lk, int level, int k, int group, int n_digits, int64_t batch, int ntt_in,
                                     int rescale, uint64_t c1, uint64_t c2, uint64_t out, int* nothing, char* msg, size_t cap) {
    bool nd = false;
    const int rc = ks_group_mul_check(any_null != 0, L, N, logN, Lk, level, k, group, n_digits, batch, ntt_in, rescale, (uintptr_t)c1, (uintptr_t)c2,
                                      (uintptr_t)out, &nd, msg, cap);
    *nothing = nd ? 1 : 0;
    return rc;
}

}  // extern "C"
