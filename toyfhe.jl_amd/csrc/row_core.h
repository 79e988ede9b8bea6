// row_core.h -- one limb row through registers: the three-pass forward transform that leaves the canonical NTT image in the
// workgroup's registers and the three-pass inverse transform that starts from them, N = 2^12 .. 2^14, both arithmetic policies,
// built from the policy-templated passes of ntt_core.h.  The fused row kernels -- k_mul_core_int (mul_core.h), k_encrypt_fused /
// k_decrypt_fused (enc_core.h), k_evalkey_fused (keygen_core.h) -- are these two sequences with their own products in between, one
// (item, limb) row per workgroup pass.  (k_bfv_core_fused / k_ks_fused keep their tuned fused_fwd_to_regs / fused_inv_from_regs,
// kernels.h.)
//
// The per-thread PHASES (everything between two barriers) are plain TFHE_HD functions, so that the CPU emulations under tests/
// (row_emul.h) run the very code of the kernels: one loop over the thread ids per phase.  The barrier sequences and the item walk
// are device code (they need kernels.h) and are compiled only under hipcc.
//
// Ranges, u64 policy (ArithInt): the forward passes keep Harvey's [0, 4q); the last one canonicalises (out_fwd).  Barrett products
// of canonical words and their sums are canonical, which is inside the [0, 2q) the inverse butterflies take; the final store is
// canonical.  The fp64 policy's entries are stated where a kernel makes them (enc_core.h, keygen_core.h).
#pragma once
#include "ntt_core.h"

template <class A, int LOGB, int LOGT>
struct row_core {
    static constexpr int K1 = pass_k_fwd(LOGB, LOGT, 0), K2 = pass_k_fwd(LOGB, LOGT, K1), K3 = LOGB - K1 - K2;
    static constexpr int KI1 = pass_k_inv(LOGB, LOGT, LOGB), S1 = LOGB - KI1, KI2 = pass_k_inv(LOGB, LOGT, S1), S2 = S1 - KI2;
    static_assert(K3 >= 1 && pass_k_fwd(LOGB, LOGT, K1 + K2) == K3, "three-pass forward schedule expected");
    static_assert(KI1 == K3, "forward last pass and inverse first pass must share the register map");
    static_assert(S2 >= 1 && pass_k_inv(LOGB, LOGT, S2) == S2, "three-pass inverse schedule expected");
    typedef pgeom<LOGB, LOGT, 0, K1> G1;            // forward first pass: where a thread's source words lie
    typedef pgeom<LOGB, LOGT, LOGB - K3, K3> G3;    // the shared register map of the NTT image
    typedef pgeom<LOGB, LOGT, 0, S2> GL;            // inverse last pass: where a thread's result words go
    static constexpr int E = G3::E;
    typedef typename A::elem elem;
    typedef typename A::ctx actx;

    static TFHE_HD u32 nat_of(u32 tid, int e) {      // natural-order position (NTT domain) of register e
        u32 c0, hi, base;
        G3::template coords<true>(tid, e / G3::R, c0, hi, base);
        return (brev_bits((u32)(e % G3::R), K3) << (LOGB - K3)) + c0;
    }
    static TFHE_HD u32 src_of(u32 tid, int e) {      // coefficient the forward transform's raw word e holds
        u32 c0, hi, base;
        G1::template coords<false>(tid, e / G1::R, c0, hi, base);
        return base + ((u32)(e % G1::R) << G1::LO);
    }
    static TFHE_HD u32 dst_of(u32 tid, int e) {      // coefficient the inverse transform's result word e is
        u32 c0, hi, base;
        GL::template coords<false>(tid, e / GL::R, c0, hi, base);
        return base + ((u32)(e % GL::R) << GL::LO);
    }

    // ---- forward transform: load (or form) | barrier | first | barrier | mid | barrier | last (canonical, in registers) ----
    static TFHE_HD void fwd_load(u64* raw, const u64* grow, u32 tid) { fwd_load_data<LOGB, LOGT, 0, K1, true, false>(raw, nullptr, grow, tid); }
    // a row a kernel formed in the LDS words the thread's own first pass reads (no barrier between the two: a thread reads back
    // what it wrote)
    static TFHE_HD void u_load(u64* raw, const u64* lds, u32 tid) { fwd_load_data<LOGB, LOGT, 0, K1, false, false>(raw, lds, nullptr, tid); }
    // (v: the pass's work row -- a caller's row that is dead until the last pass fills it, or a local one)
    static TFHE_HD void fwd_first(const u64* raw, u64* lds, const actx& C, u32 tid, elem* v) {
        fwd_compute<A, LOGB, LOGT, 0, K1, true, false, 0>(v, raw, nullptr, C, tid, 1u);
        fwd_store<A, LOGB, LOGT, 0, K1, false>(v, lds, nullptr, C, tid, 0, 0u);
    }
    static TFHE_HD void fwd_first(const u64* raw, u64* lds, const actx& C, u32 tid) {
        elem v[E];
        fwd_first(raw, lds, C, tid, v);
    }
    static TFHE_HD void fwd_mid(u64* lds, const actx& C, u32 tid) {
        ntt_fwd_pass<A, LOGB, LOGT, K1, K2, false, false>(lds, nullptr, nullptr, C, tid, 1u, 0, 0u);
    }
    static TFHE_HD void fwd_last(const u64* lds, const actx& C, u32 tid, u64* out) {
        u64 r3[E];
        elem v[E];
        fwd_load_data<LOGB, LOGT, K1 + K2, K3, false, true>(r3, lds, nullptr, tid);
        fwd_compute<A, LOGB, LOGT, K1 + K2, K3, false, true, 0>(v, r3, nullptr, C, tid, 1u);
#pragma unroll
        for (int e = 0; e < E; e++) out[e] = A::out_fwd(v[e], C);
    }
    // ---- inverse transform from registers: barrier | first | barrier | mid | barrier | last ----
    static TFHE_HD void to_elem(elem* v, const u64* acc, const actx& C) {   // canonical words -> the inverse transform's operand
#pragma unroll
        for (int e = 0; e < E; e++) v[e] = A::from_global(acc[e], C);
    }
    static TFHE_HD void inv_first(u64* lds, const actx& C, u32 tid, elem* v) {
        inv_compute<A, LOGB, LOGT, S1, KI1, true, true, 0, -1, no_hook, true>(v, nullptr, nullptr, C, tid, 1u);
        inv_store<A, LOGB, LOGT, S1, KI1, true, true>(v, lds, nullptr, C, tid);
    }
    static TFHE_HD void inv_mid(u64* lds, const actx& C, u32 tid) {
        ntt_inv_pass<A, LOGB, LOGT, S2, KI2, false, false, true>(lds, nullptr, nullptr, C, tid, 1u, 0, 0u);
    }
    // last pass, canonical words to gdst (+ the addend row, if any)
    static TFHE_HD void inv_last(u64* lds, u64* gdst, const actx& C, u32 tid, const u64* addend = nullptr) {
        ntt_inv_pass<A, LOGB, LOGT, 0, S2, false, true, true>(lds, nullptr, gdst, C, tid, 1u, 0, 0u, addend);
    }
    // an NTT image from registers to a row in memory, natural order; a thread reads back its own words only
    static TFHE_HD void park_row(u64* park, const u64* v, u32 tid) {
#pragma unroll
        for (int e = 0; e < E; e++) park[nat_of(tid, e)] = v[e];
    }
};

#if defined(__HIPCC__)
// `first`: no transform of this workgroup has run yet, so nothing has read the LDS image and the opening barrier is not needed
template <class A, int LOGB, int LOGT>
__device__ __forceinline__ void row_forward(u64* lds, const u64* raw, const typename A::ctx& C, bool& first, u64* out) {
    typedef row_core<A, LOGB, LOGT> M;
    const u32 tid = fresh_tid();
    if (!first) __syncthreads();  // the previous transform's last pass has read LDS
    first = false;
    M::fwd_first(raw, lds, C, tid);
    __syncthreads();
    M::fwd_mid(lds, C, tid);
    __syncthreads();
    M::fwd_last(lds, C, tid, out);
}
// the caller's last pass follows (inv_last, or one that adds something of its own in the store)
template <class A, int LOGB, int LOGT>
__device__ __forceinline__ void row_inverse_head(u64* lds, typename A::elem* v, const typename A::ctx& C, bool& first) {
    typedef row_core<A, LOGB, LOGT> M;
    const u32 tid = fresh_tid();
    if (!first) __syncthreads();  // the previous transform's last pass has read LDS
    first = false;
    M::inv_first(lds, C, tid, v);
    __syncthreads();
    M::inv_mid(lds, C, tid);
    __syncthreads();
}
// The (item, limb) rows of this workgroup, in the XCD limb walk over `nitems` rows of `nb` limbs per item:
//     for (u32 it = 0, item; row_item(it, nb, nitems, item); it++)
__device__ __forceinline__ bool row_item(u32 it, u32 nb, u32 nitems, u32& item) {
    if (it >= xcd_limb_niter(gridDim.x, nitems)) return false;
    // (workgroup-uniform, but the walk's divisions run on the vector unit: say so, or every row pointer derived from it lives
    // in vector registers across the whole item)
    item = (u32)__builtin_amdgcn_readfirstlane((int)xcd_limb_walk(it, blockIdx.x, gridDim.x, nb, nitems));
    return item != ~0u;
}
#endif  // __HIPCC__
