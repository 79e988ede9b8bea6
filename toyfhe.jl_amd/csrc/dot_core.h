// dot_core.h -- tfhe_dot_plain: dst_i = (acc_i +) sum_k T_k(a[k]_i) .* b[k]_i, the accumulation of the diagonal matrix product
// (infer.jl:140-149: `result += rotated_k * diagonal_k` over rotated ciphertexts that are still in the coefficient domain), with
// the forward transforms of the terms inside the sum.
//   k_dot_plain_fused   N = 2^12 .. 2^14, both arithmetic policies: one (item, limb) row per workgroup pass.  The running sum is E
//                       canonical words per thread in the register map of the NTT image (row_core G3); a coefficient-domain term goes
//                       through the three-pass forward transform of row_core.h, which leaves its image in that very map, a term
//                       that is transformed already is read where it lies; either is multiplied by the plaintext row and added.
//                       A term's source row and plaintext row are read once.  A batch with few rows is split over the terms as
//                       well (partial sums, joined by k_dot_join), so that the launch covers the chip.
//   k_dot_view          every other size: the stride-aware sibling of k_dot (kernels.h) over operands that are transformed already
//                       (dot_api.inc gathers and transforms the others first); the same lazily reduced 128-bit sums.
// Every operand is a VIEW: item i is [limbs][N] words at base + i * stride.  The per-thread PHASES are plain TFHE_HD functions, so
// that the CPU emulation under tests/dot_core_emul/ runs the very code of the kernel.
//
// Ranges.  u64 policy (ArithInt): as row_core.h; the last forward pass canonicalises (out_fwd).  fp64 policy (ArithFp): a term's
// source words are canonical residues and enter the forward transform at its plain-transform entry, the one the forward sweep plan
// (fp_fwd_sweep_before) is made for, and nowhere else; the last pass canonicalises.  Under either policy the products x .* b are
// Barrett products of canonical words (ntt_limb_t::br, valid for every limb) and their sums are canonical: no double ever holds a
// product of two data words, and the largest |operand| / p that enters an fp64 product or reduction is that of a plain transform
// (< TFHE_FP_LIMIT; tests/test_dot_plain_cpu.py runs the phases at TFHE_FP_QMAX with every word q - 1 and range tracking on).
// The words are those of tfhe_nntt followed by tfhe_mad term by term.
#pragma once
#include <algorithm>
#include "lazy_sum.h"
#include "row_core.h"

// How a fused pass of n terms over `rows` (item, limb) rows is split over its terms: *tps terms per split, the number of splits
// returned.  One split when the rows fill the chip; otherwise as many as fill it, of at least four terms each (a split costs one more
// row written and read back, a term two rows read).
inline int dot_split(long long fill, long long rows, int n, int* tps) {
    const long long want = rows < fill ? fill / rows : 1;
    *tps = (int)std::max<long long>(std::min(n, 4), (n + want - 1) / want);
    return (n + *tps - 1) / *tps;
}

template <class A, int LOGB, int LOGT>
struct dot_core : row_core<A, LOGB, LOGT> {
    typedef row_core<A, LOGB, LOGT> B;
    using B::E;
    using B::nat_of;

    // the running sum: the accumulator row's words (canonical) or zero.  (acc may be the row dst is stored to: a thread reads
    // here exactly the words it stores at the end.)
    static TFHE_HD void acc_init(u64* acc, const u64* arow, u32 tid) {
#pragma unroll
        for (int e = 0; e < E; e++) acc[e] = arow ? arow[nat_of(tid, e)] : 0;
    }
    // acc += x .* b for an image in registers (a forward transform's result).  Eight registers per piece, as enc_core's
    // dec_acc_ntt: one loop over all E is left rolled by the compiler and indexes `acc` dynamically (scratch memory), and the
    // plaintext words of a whole row requested at once do not fit beside the sum and the image at N = 2^14.
    template <int E0 = 0>
    static TFHE_HD void mac_regs(u64* acc, const u64* x, const u64* brow, const barrett_t& br, u32 tid) {
#pragma unroll
        for (int i = 0; i < 8; i++) acc[E0 + i] = addmod(acc[E0 + i], mulmod(x[E0 + i], brow[nat_of(tid, E0 + i)], br), br.q);
        TFHE_SCHED_FENCE();   // the next piece's loads stay behind this one's
        if constexpr (E0 + 8 < E) mac_regs<E0 + 8>(acc, x, brow, br, tid);
    }
    // acc += a .* b for a term that is an NTT image already, from the rows as they lie
    template <int E0 = 0>
    static TFHE_HD void mac_ntt(u64* acc, const u64* arow, const u64* brow, const barrett_t& br, u32 tid) {
#pragma unroll
        for (int i = 0; i < 8; i++) {
            const u32 nat = nat_of(tid, E0 + i);
            acc[E0 + i] = addmod(acc[E0 + i], mulmod(arow[nat], brow[nat], br), br.q);
        }
        TFHE_SCHED_FENCE();
        if constexpr (E0 + 8 < E) mac_ntt<E0 + 8>(acc, arow, brow, br, tid);
    }
    static_assert(E % 8 == 0, "the products run in pieces of eight registers");
    // ---- the split over terms: split s of a pass of n terms takes [k0, k1); split 0 stores to dst, split s > 0 its partial sum to
    // row (s - 1, item i, buffer limb p) of part [nsplit - 1][ni][limbs][N]; join_word adds those onto a word of dst ----
    static TFHE_HD void split_terms(u32 s, u32 tps, int n, int& k0, int& k1) {
        k0 = (int)(s * tps);
        k1 = k0 + (int)tps < n ? k0 + (int)tps : n;
    }
    static TFHE_HD size_t part_row(u32 s, u32 ni, size_t i, u32 limbs, u32 p) { return (((size_t)(s - 1) * ni + i) * limbs + p) << LOGB; }
};

// one word of k_dot_join: r + the words at `at` of the rows (s - 1, item, limb j) of part, s = 1 .. nsplit - 1, n words per row
TFHE_HD u64 dot_join_word(u64 r, const u64* part, u32 nsplit, u32 ni, size_t item, u32 limbs, u32 j, u32 n, u32 at, u64 q) {
    for (u32 s = 1; s < nsplit; s++) r = addmod(r, part[((((size_t)(s - 1) * ni + item) * limbs + j) * n) + at], q);
    return r;
}

#if defined(__HIPCC__)
// The term table of one launch: up to TFHE_DOT_MAX views (bases of the launch's first item, strides in words; b_stride 0: one
// plaintext for the whole batch).  Bit k of a_ntt: term k is an NTT image already.
struct dot_view_arg_t {
    const u64* a[TFHE_DOT_MAX];
    const u64* b[TFHE_DOT_MAX];
    u64 a_stride[TFHE_DOT_MAX];
    u64 b_stride[TFHE_DOT_MAX];
    u64 a_ntt;
    int n;
};

// `pos` lists the buffer limbs (rows of an item) of this launch's policy, sel.idx[p] is the context modulus of buffer limb p.  A work
// item is (split s, item i, listed limb): split s takes the terms [s tps, (s + 1) tps) of row (i, limb), so that a batch with fewer
// rows than the chip has workgroup slots still fills it (63 terms of 16 x 3 rows: 48 rows, each a chain of 63 transforms, otherwise).
// Split 0 starts from acc and stores to dst; split s > 0 starts from zero and stores its partial sum to part [nsplit - 1][ni][limbs][N],
// which k_dot_join adds onto dst.  acc (nullptr: none) may be the same view as dst: neither is __restrict__.
template <class A, int LOGB, int LOGT>
__global__ __launch_bounds__(1 << LOGT) void k_dot_plain_fused(dot_view_arg_t D, const u64* acc, u64 acc_stride, u64* dst, u64 dst_stride,
                                                                u64* part, u32 ni, u32 tps, const ntt_limb_t* __restrict__ LT, limb_sel_t sel,
                                                                limb_sel_t pos, u32 nitems) {
    extern __shared__ __attribute__((aligned(16))) u64 lds[];
    typedef dot_core<A, LOGB, LOGT> M;
    constexpr int E = M::E;
    const u32 nb = (u32)pos.n;
    bool first = true;
    for (u32 it = 0, item; row_item(it, nb, nitems, item); it++) {
        const u32 p = (u32)pos.idx[item % nb], v = item / nb, s = v / ni;
        const size_t i = v - s * ni, off = (size_t)p << LOGB;
        int k0, k1;
        M::split_terms(s, tps, D.n, k0, k1);
        const ntt_limb_t& L = LT[sel.idx[p]];
        const typename A::ctx C = A::make(L);
        const barrett_t br = L.br;
        u64 sum[E];
        M::acc_init(sum, (acc && s == 0) ? acc + i * acc_stride + off : nullptr, fresh_tid());
        for (int k = k0; k < k1; k++) {
            const u64* const arow = D.a[k] + i * D.a_stride[k] + off;
            const u64* const brow = D.b[k] + i * D.b_stride[k] + off;
            if ((D.a_ntt >> k) & 1u) {
                M::mac_ntt(sum, arow, brow, br, fresh_tid());
            } else {
                u64 x[E];
                {
                    u64 raw[E];
                    M::fwd_load(raw, arow, fresh_tid());
                    row_forward<A, LOGB, LOGT>(lds, raw, C, first, x);
                }
                M::mac_regs(sum, x, brow, br, fresh_tid());
            }
        }
        u64* const out = s == 0 ? dst + i * dst_stride + off : part + M::part_row(s, ni, i, (u32)sel.n, p);
        M::park_row(out, sum, fresh_tid());
    }
}
// dst += the partial sums of the splits s = 1 .. nsplit - 1 (part [nsplit - 1][ni][limbs][N], canonical words).  One row per
// blockIdx.x (row_grid).
__global__ __launch_bounds__(256) void k_dot_join(u64* __restrict__ dst, u64 dst_stride, const u64* __restrict__ part, u32 ni, u32 nsplit,
                                                   const ntt_limb_t* __restrict__ LT, limb_sel_t sel, u32 n) {
    const u32 row = blockIdx.x, j = row % (u32)sel.n;
    const size_t item = row / (u32)sel.n;
    const u64 q = LT[sel.idx[j]].q;
    u64* const drow = dst + item * dst_stride + (size_t)j * n;
    for (u32 i = blockIdx.y * blockDim.x + threadIdx.x; i < n; i += gridDim.y * blockDim.x) {
        drow[i] = dot_join_word(drow[i], part, nsplit, ni, item, (u32)sel.n, j, n, i, q);
    }
}

// dst = (acc +) sum_k a_k .* b_k over views of NTT images: k_dot with strides.  Exact: full 128-bit products are summed and
// reduced (Barrett) every `chunk` terms, chunk = 2^(62 - bits(q)) capped at the term count -- the canonical residues of the
// one-by-one mulmod / addmod sequence.  One row per blockIdx.x (row_grid).
__global__ __launch_bounds__(256) void k_dot_view(dot_view_arg_t D, const u64* acc, u64 acc_stride, u64* dst, u64 dst_stride,
                                                   const ntt_limb_t* __restrict__ LT, limb_sel_t sel, u32 n) {
    const u32 row = blockIdx.x, j = row % (u32)sel.n;
    const size_t item = row / (u32)sel.n, off = (size_t)j * n;
    const ntt_limb_t L = LT[sel.idx[j]];
    const int chunk = (int)lazy_chunk(L.q);   // products summed between two reductions
    const u64* const arow = acc ? acc + item * acc_stride + off : nullptr;
    u64* const drow = dst + item * dst_stride + off;
    for (u32 i = blockIdx.y * blockDim.x + threadIdx.x; i < n; i += gridDim.y * blockDim.x) {
        u64 r = arow ? arow[i] : 0;
        for (int k0 = 0; k0 < D.n; k0 += chunk) {
            acc128 s{r, 0};
            const int k1 = k0 + chunk < D.n ? k0 + chunk : D.n;
            for (int k = k0; k < k1; k++) acc_mac(s, D.a[k][item * D.a_stride[k] + off + i], D.b[k][item * D.b_stride[k] + off + i]);
            r = barrett_reduce128(s.lo, s.hi, L.br);
        }
        drow[i] = r;
    }
}
#endif  // __HIPCC__
