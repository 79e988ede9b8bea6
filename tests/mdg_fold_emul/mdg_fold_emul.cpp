// tests/mdg_fold_emul/mdg_fold_emul.cpp -- CPU emulation of what one evaluation-domain fold step on grouped-digit keys adds to
// toyfhe.jl_amd/csrc/ks_group_core.h: the sum of k_mdg_fold_gather over the kernel's own layouts (the key sums in the EPI layout, row pairs of X and E), the
// per-coefficient body of k_mdg_fold_finish<K, V> (mdg_fold_finish_coeff) in the kernel's order -- blocks of JB limbs, the rotations
// inside, the bias last -- over whole rows, and the host checks of tfhe_rotate_sum_grouped / tfhe_matmul_bsgs_fold_grouped
// (ks_group_fold_check) on plain numbers.  TEST INFRASTRUCTURE ONLY.
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../toyfhe.jl_amd/csrc/bfv_tables.h"
#include "../../toyfhe.jl_amd/csrc/ntt_core.h"
#include "../../toyfhe.jl_amd/csrc/ks_group_core.h"

namespace {

template <int K, int JB>
void finish_rows(int level, size_t n, int nrot, const barrett_t* lb, const tw_t (*inv)[TFHE_MAX_LIMBS], const u64* pb, const u64* e, const u64* bias,
                 u64* dst) {
    for (size_t i = 0; i < n; i++) {
        for (int j0 = 0; j0 < level; j0 += JB) {
            const int nj = level - j0 < JB ? level - j0 : JB;
            u64 acc[JB];
            for (int r = 0; r < JB; r++) acc[r] = e[(size_t)(j0 + (r < nj ? r : nj - 1)) * n + i];
            for (int r = 0; r < nrot; r++) {
                u64 y[K];
                for (int t = 0; t < K; t++) y[t] = pb[((size_t)r * K + t) * n + i];
                mdg_fold_finish_coeff<K, JB>(acc, y, j0, nj, level, lb, inv);
            }
            for (int r = 0; r < nj; r++) {
                u64 x = acc[r];
                if (bias) x = addmod(x, bias[(size_t)(j0 + r) * n + i], lb[j0 + r].q);
                dst[(size_t)(j0 + r) * n + i] = x;
            }
        }
    }
}
template <int K>
void finish_jb(int jb, int level, size_t n, int nrot, const barrett_t* lb, const tw_t (*inv)[TFHE_MAX_LIMBS], const u64* pb, const u64* e,
               const u64* bias, u64* dst) {
    if (jb == 2) finish_rows<K, 2>(level, n, nrot, lb, inv, pb, e, bias, dst);
    else finish_rows<K, TFHE_MDG_FOLD_JB>(level, n, nrot, lb, inv, pb, e, bias, dst);
}

}  // namespace

extern "C" {

int mdg_fold_emul_jb() { return TFHE_MDG_FOLD_JB; }

// The gather over a whole chunk, in the layouts the kernel reads and writes: X, E [batch][2][level][n]; V the key sums as the EPI
// epilogue leaves them (kernels.h epi_pair: ciphertext ci = r batch + b, working limb j, position k, component s at word
// ((ci nw + j) n + k) 2 + s), nrot batch nw rows of 2 n words.  q [level]: the ciphertext limbs' moduli.  Per row pair (b, j), as the
// kernel walks them:  E[b][s][j][k] = X[b][s][j][k] + sum_r V[r batch + b][j][pi_r k].{s},  pi_r = galois_ntt_pos(., gs[r], n).
int mdg_fold_emul_gather(const uint64_t* q, long n, int nrot, int batch, int level, int nw, const uint64_t* gs, const uint64_t* x, const uint64_t* v,
                         uint64_t* e) {
    if (n < 1 || (n & (n - 1)) || nrot < 0 || batch < 1 || level < 1 || nw < level) return -1;
    for (int pr = 0; pr < batch * level; pr++) {
        const int j = pr % level, b = pr / level;
        const size_t row0 = ((size_t)b * 2 * level + j) * n, row1 = row0 + (size_t)level * n;
        for (long k = 0; k < n; k++) {
            u64 a0 = x[row0 + k], a1 = x[row1 + k];
            for (int r = 0; r < nrot; r++) {
                const uint64_t* pv = v + (((size_t)r * batch + b) * nw + j) * 2 * n + 2 * (size_t)galois_ntt_pos((u32)k, gs[r], (u32)n);
                a0 = addmod(a0, pv[0], q[j]);
                a1 = addmod(a1, pv[1], q[j]);
            }
            e[row0 + k] = a0;
            e[row1 + k] = a1;
        }
    }
    return 0;
}

// One (ciphertext, component) through the finish with K special primes and blocks of jb limbs (2, or the kernel's TFHE_MDG_FOLD_JB):
// w [level + K] working moduli (the special primes last), pb [nrot][K][n] the special words (coefficient domain, canonical),
// e [level][n], bias [level][n] or null, dst [level][n] out, pinv [level] out (Pinv_j).  Returns 0, or -1 for a bad shape.
int mdg_fold_emul_finish(int K, int jb, int level, const uint64_t* w, long n, int nrot, const uint64_t* pb, const uint64_t* e, const uint64_t* bias,
                         uint64_t* dst, uint64_t* pinv) {
    if (K < 1 || K > TFHE_KSG_MAX_SPECIAL || level < 1 || level + K > TFHE_MAX_LIMBS || n < 1 || nrot < 0 || (jb != 2 && jb != TFHE_MDG_FOLD_JB)) return -1;
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
        case 1: finish_jb<1>(jb, level, (size_t)n, nrot, lb, inv, pb, e, bias, dst); break;
        case 2: finish_jb<2>(jb, level, (size_t)n, nrot, lb, inv, pb, e, bias, dst); break;
        case 3: finish_jb<3>(jb, level, (size_t)n, nrot, lb, inv, pb, e, bias, dst); break;
        default: finish_jb<4>(jb, level, (size_t)n, nrot, lb, inv, pb, e, bias, dst); break;
    }
    return 0;
}

// the host checks of tfhe_rotate_sum_grouped (product = 0) / tfhe_matmul_bsgs_fold_grouped on a ring of L limbs and degree N: *_null
// flag the null keys, diag_addr / ct_addr [n_in] are the operands' addresses as numbers (0: null); bias / out are addresses as numbers.
// *nothing_to_do: the call returns TFHE_OK without work.
int mdg_fold_emul_check(int product, int any_null, int L, int64_t N, int Lk, int level, int k, int group, int n_digits, int64_t batch,
                        const int* baby_null, const uint64_t* baby_galois, int n_baby, const int* giant_null, const uint64_t* giant_galois, int n_giant,
                        const uint64_t* diag_addr, const uint64_t* ct_addr, int n_in, const int* fold_null, const uint64_t* fold_galois,
                        const int* fold_sizes, int n_fold_steps, uint64_t bias, uint64_t out, int* nothing_to_do, char* msg, size_t cap) {
    static const uint64_t some_key = 0;
    const auto count = [](int n) { return (size_t)(n < 0 ? 0 : (n > 64 ? 64 : n)); };
    std::vector<const uint64_t*> bk(count(n_baby) + 1), gk(count(n_giant) + 1), dg(count(n_in) + 1), ct(count(n_in) + 1), fk(65);
    for (size_t r = 0; r < count(n_baby); r++) bk[r] = baby_null[r] ? nullptr : &some_key;
    for (size_t r = 0; r < count(n_giant); r++) gk[r] = giant_null[r] ? nullptr : &some_key;
    for (size_t m = 0; m < count(n_in); m++) {
        dg[m] = (const uint64_t*)(uintptr_t)diag_addr[m];
        ct[m] = (const uint64_t*)(uintptr_t)ct_addr[m];
    }
    for (size_t r = 0; r < 64; r++) fk[r] = fold_null[r] ? nullptr : &some_key;   // (fold_null: 64 flags)
    bool nothing = false;
    const int rc = ks_group_fold_check(product != 0, any_null != 0, L, N, Lk, level, k, group, n_digits, batch, bk.data(), baby_galois, n_baby,
                                       gk.data(), giant_galois, n_giant, dg.data(), ct.data(), n_in, fk.data(), fold_galois, fold_sizes, n_fold_steps,
                                       (uintptr_t)bias, (uintptr_t)out, &nothing, msg, cap);
    *nothing_to_do = nothing ? 1 : 0;
    return rc;
}

}  // extern "C"
