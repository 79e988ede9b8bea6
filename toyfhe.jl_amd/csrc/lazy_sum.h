// lazy_sum.h -- sums of 128-bit products under the Barrett window: how many products fit between two reductions (lazy_chunk, the
// one place in csrc/ where that rule is written: k_dot, k_lincomb, k_lincomb_many and k_dot_view take their chunk from it), and the
// accumulation bodies of the diagonal products -- NO running sums of ONE value each, tfhe_matmul_diag with NO = 1, tfhe_matmul_bsgs
// with a tile of up to four giant steps, tfhe_matmul_bsgs_blocks the same seeded with the sums of its earlier inputs.  Plain host /
// device functions: the kernels (kernels.h: k_md_acc, k_md_acc_dense) string them together with their loads, tests/md_acc_emul/
// runs them on the CPU against exact sums.
//
// inner_j[k] = sum_{i = 0 .. n_baby} diag[j][i][k] * r_i[k] for the giant steps j of one tile: every r_i[k] is formed once and
// multiplied into the tile's NO sums; only the diagonal words differ between them.
#pragma once
#include "modarith.h"

// products that may be summed onto a reduced word between two Barrett reductions: chunk q^2 + q < 2^(bits(q) + 62), the window of
// barrett_reduce128 (at most 64: TFHE_DOT_MAX terms)
TFHE_HD u32 lazy_chunk(u64 q) {
    int bits = 0;
    while ((q >> bits) != 0) bits++;
    return bits >= 62 ? 1u : (62 - bits >= 6 ? 64u : (1u << (62 - bits)));
}
// the giant step lane o of the tile at j0 works on; the lanes past the last step of a ragged tile repeat it and are not stored
TFHE_HD u32 bsgs_tile_step(u32 j0, u32 o, u32 ngiant1) { return j0 + o < ngiant1 ? j0 + o : ngiant1 - 1u; }

template <int NO>
struct lazy_sums {
    acc128 a[NO];
    TFHE_HD void clear() {
#pragma unroll
        for (int o = 0; o < NO; o++) a[o] = acc128{0, 0};
    }
    // the seeded start (tfhe_matmul_bsgs_blocks, inputs m >= 1): every sum continues from a reduced word w[o] < q instead of from
    // zero.  That word is the "reduced word" of lazy_chunk's window, not one of its products: `pend` starts where it starts after clear()
    TFHE_HD void seed(const u64* w) {
#pragma unroll
        for (int o = 0; o < NO; o++) a[o] = acc128{w[o], 0};
    }
    // x into every sum, each against its own diagonal word
    TFHE_HD void mac(u64 x, const u64* d) {
#pragma unroll
        for (int o = 0; o < NO; o++) acc_mac(a[o], x, d[o]);
    }
    TFHE_HD void fold(const barrett_t& br) {
#pragma unroll
        for (int o = 0; o < NO; o++) a[o] = acc128{barrett_reduce128(a[o].lo, a[o].hi, br), 0};
    }
    TFHE_HD u64 word(int o, const barrett_t& br) const { return barrett_reduce128(a[o].lo, a[o].hi, br); }
};
// the bookkeeping of the lazy reduction: true when `chunk` products are pending, i.e. the sums must be folded before the next one
TFHE_HD bool lazy_fold_due(u32& pend, u32 chunk) {
    if (pend != chunk) return false;
    pend = 0;
    return true;
}
// the rotated value of the evaluation-domain form (k_md_acc): V[pi_r k] - U[k], U scaled by P^-1 here where the lift left that out
template <bool USCALE>
TFHE_HD u64 gather_term(u64 v, u64 u, tw_t pinv, u64 q) {
    if (USCALE) u = shoup_full(u, pinv, q);
    return submod(v, u, q);
}
// one step of the rotate-and-sum fold (k_md_fold): the running sum of a coefficient plus the rotated value of one rotation.  Plain
// modular additions on canonical residues -- there is no plaintext factor, so nothing is summed lazily
template <bool USCALE>
TFHE_HD u64 fold_term(u64 acc, u64 v, u64 u, tw_t pinv, u64 q) {
    return addmod(acc, gather_term<USCALE>(v, u, pinv, q), q);
}
