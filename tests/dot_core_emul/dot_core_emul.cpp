// tests/dot_core_emul/dot_core_emul.cpp -- CPU emulation of the fused ciphertext x plaintext sum (toyfhe.jl_amd/csrc/dot_core.h):
// the body of k_dot_plain_fused on the harness of tests/row_emul.h, range tracking on.  TEST INFRASTRUCTURE ONLY.
#define TFHE_EMUL_TRACK_RANGE 1
#include "../row_emul.h"
#include "../../toyfhe.jl_amd/csrc/dot_core.h"

namespace {

template <class A, int LOGB>
struct emul : row_emul<A, LOGB> {
    typedef row_emul<A, LOGB> H;
    typedef dot_core<A, LOGB, H::LOGT> M;
    using H::T; using H::br; using H::at; using H::forward_row;

    // one (item, limb) row: acc [N] or null, a [n_terms][N], b [n_terms][N] -> dst [N] (dst may be acc)
    void dot(const u64* acc, const u64* a, const uint8_t* a_ntt, const u64* b, int n_terms, u64* dst) {
        const size_t n = H::N;
        typename H::regs_t sum = H::regs(), x = H::regs();
        for (u32 t = 0; t < T; t++) M::acc_init(at(sum, t), acc, t);
        for (int k = 0; k < n_terms; k++) {
            const u64 *arow = a + (size_t)k * n, *brow = b + (size_t)k * n;
            if (a_ntt[k]) {
                for (u32 t = 0; t < T; t++) M::mac_ntt(at(sum, t), arow, brow, br, t);
            } else {
                forward_row(arow, x);
                for (u32 t = 0; t < T; t++) M::mac_regs(at(sum, t), at(x, t), brow, br, t);
            }
        }
        for (u32 t = 0; t < T; t++) M::park_row(dst, at(sum, t), t);
    }
    // the same row the way a launch with few rows runs it (k_dot_plain_fused with ni = 1, one limb; k_dot_join): dot_split over
    // `fill` workgroup slots, split s over its terms into dst (s = 0, from acc) or its row of `part`, then the join.  Returns the splits.
    int dot_splits(long long fill, const u64* acc, const u64* a, const uint8_t* a_ntt, const u64* b, int n_terms, u64* dst) {
        const size_t n = H::N;
        int tps;
        const int nsplit = dot_split(fill, 1, n_terms, &tps);
        std::vector<u64> part((size_t)(nsplit > 1 ? nsplit - 1 : 1) * n);
        for (int s = 0; s < nsplit; s++) {
            int k0, k1;
            M::split_terms((u32)s, (u32)tps, n_terms, k0, k1);
            u64* out = s == 0 ? dst : part.data() + M::part_row((u32)s, 1, 0, 1, 0);
            dot(s == 0 ? acc : nullptr, a + (size_t)k0 * n, a_ntt + k0, b + (size_t)k0 * n, k1 - k0, out);
        }
        for (u32 i = 0; i < (u32)n; i++) dst[i] = dot_join_word(dst[i], part.data(), (u32)nsplit, 1, 0, 1, 0, (u32)n, i, br.q);
        return nsplit;
    }
};

}  // namespace

extern "C" {

// one (item, limb) row of k_dot_plain_fused.  Returns 0, -1 bad psi, -2 unsupported size, -3 fp64 policy asked for a modulus above
// TFHE_FP_QMAX.  *max_ratio: the range tracker's reading (0 for the u64 policy).
int dot_core_emul_dot(int logn, uint64_t q, int fp, const uint64_t* acc, const uint64_t* a, const uint8_t* a_ntt, const uint64_t* b,
                      int n_terms, uint64_t* dst, double* max_ratio) {
    return row_emul_run<emul>(logn, q, 0, fp, max_ratio, [&](auto& e) { e.dot(acc, a, a_ntt, b, n_terms, dst); });
}

// the same through the split over terms and the join, for `fill` workgroup slots; *nsplit: the splits taken
int dot_core_emul_dot_split(int logn, uint64_t q, int fp, long long fill, const uint64_t* acc, const uint64_t* a, const uint8_t* a_ntt,
                            const uint64_t* b, int n_terms, uint64_t* dst, int* nsplit) {
    return row_emul_run<emul>(logn, q, 0, fp, nullptr, [&](auto& e) { *nsplit = e.dot_splits(fill, acc, a, a_ntt, b, n_terms, dst); });
}

}  // extern "C"
