// mul_core.h -- the fused product core of tfhe_mul_relin for the u64 policy (ArithInt: moduli from TFHE_FP_QMAX up to 2^62),
// N = 2^12 .. 2^14:   T_k[b][j] = INTT_j( tensor_k( NTT_j(a0), NTT_j(a1), NTT_j(b0), NTT_j(b1) ) ),  k = 0, 1, 2
// (enc_mul, rlwe_she.jl:255-258, with mul_expand / mul_contract the identity: CKKS, BGV) for one (ciphertext b, limb j) per
// workgroup pass -- the u64 counterpart of k_bfv_core_fused (kernels.h), built from the policy-templated passes of ntt_core.h.
//
// The per-thread PHASES (everything between two barriers) are plain TFHE_HD functions, so that the CPU emulation under
// tests/mul_core_emul/ runs the very code of the kernel: one loop over the thread ids per phase.  The kernel itself is device
// code (needs kernels.h) and is compiled only under hipcc.
//
// Ranges: the forward passes keep Harvey's [0, 4q); the last one canonicalises (out_fwd), because a data x data product goes
// through Barrett (ntt_limb_t::br), whose window z < 2^(k+62) admits q^2 but not (4q) q at 61- and 62-bit moduli.  Products
// and their sum are canonical, which is inside the [0, 2q) the inverse butterflies take; the final store is canonical.
#pragma once
#include "ntt_core.h"

template <int LOGB, int LOGT>
struct mul_core_int {
    typedef ArithInt A;
    static constexpr int K1 = pass_k_fwd(LOGB, LOGT, 0), K2 = pass_k_fwd(LOGB, LOGT, K1), K3 = LOGB - K1 - K2;
    static constexpr int KI1 = pass_k_inv(LOGB, LOGT, LOGB), S1 = LOGB - KI1, KI2 = pass_k_inv(LOGB, LOGT, S1), S2 = S1 - KI2;
    static_assert(K3 >= 1 && pass_k_fwd(LOGB, LOGT, K1 + K2) == K3, "three-pass forward schedule expected");
    static_assert(KI1 == K3, "forward last pass and inverse first pass must share the register map");
    static_assert(S2 >= 1 && pass_k_inv(LOGB, LOGT, S2) == S2, "three-pass inverse schedule expected");
    typedef pgeom<LOGB, LOGT, LOGB - K3, K3> G3;
    static constexpr int E = G3::E;

    // natural-order position (NTT domain) of register e of thread tid in the shared register map
    static TFHE_HD u32 nat_of(u32 tid, int e) {
        u32 c0, hi, base;
        G3::template coords<true>(tid, e / G3::R, c0, hi, base);
        return (brev_bits((u32)(e % G3::R), K3) << (LOGB - K3)) + c0;
    }

    // ---- forward transform of one row: load | barrier | first | barrier | mid | barrier | last (canonical, in registers) ----
    static TFHE_HD void fwd_load(u64* raw, const u64* grow, u32 tid) { fwd_load_data<LOGB, LOGT, 0, K1, true, false>(raw, nullptr, grow, tid); }
    static TFHE_HD void fwd_first(const u64* raw, u64* lds, const A::ctx& C, u32 tid, u64* v) {
        fwd_compute<A, LOGB, LOGT, 0, K1, true, false, 0>(v, raw, nullptr, C, tid, 1u);
        fwd_store<A, LOGB, LOGT, 0, K1, false>(v, lds, nullptr, C, tid, 0, 0u);
    }
    static TFHE_HD void fwd_mid(u64* lds, const A::ctx& C, u32 tid) {
        ntt_fwd_pass<A, LOGB, LOGT, K1, K2, false, false>(lds, nullptr, nullptr, C, tid, 1u, 0, 0u);
    }
    static TFHE_HD void fwd_last(const u64* lds, const A::ctx& C, u32 tid, u64* v) {
        u64 r3[E];
        fwd_load_data<LOGB, LOGT, K1 + K2, K3, false, true>(r3, lds, nullptr, tid);
        fwd_compute<A, LOGB, LOGT, K1 + K2, K3, false, true, 0>(v, r3, nullptr, C, tid, 1u);
#pragma unroll
        for (int e = 0; e < E; e++) v[e] = A::out_fwd(v[e], C);
    }
    // ---- products (canonical operands, canonical results) ----
    // b0 in v:  park[.] <- a1 b0,  v <- a0 b0      (park: the workgroup's scratch row; a thread reads back its own words only)
    static TFHE_HD void prod_b0(u64* v, const u64* A0, const u64* A1, u64* park, const barrett_t& br, u32 tid) {
#pragma unroll
        for (int e = 0; e < E; e++) {
            park[nat_of(tid, e)] = mulmod(v[e], A1[e], br);
            v[e] = mulmod(v[e], A0[e], br);
        }
    }
    // b1 in v:  A0 <- a0 b1 + a1 b0,  A1 <- a1 b1
    static TFHE_HD void prod_b1(const u64* v, u64* A0, u64* A1, const u64* park, const barrett_t& br, u32 tid) {
#pragma unroll
        for (int e = 0; e < E; e++) {
            A0[e] = addmod(mulmod(v[e], A0[e], br), park[nat_of(tid, e)], br.q);
            A1[e] = mulmod(v[e], A1[e], br);
        }
    }
    // squaring: k = 0: a0^2, 1: 2 a0 a1, 2: a1^2 into v (A0, A1 survive)
    static TFHE_HD void prod_sq(u64* v, const u64* A0, const u64* A1, int k, const barrett_t& br) {
#pragma unroll
        for (int e = 0; e < E; e++) {
            const u64 m = mulmod(k == 2 ? A1[e] : A0[e], k == 0 ? A0[e] : A1[e], br);
            v[e] = k == 1 ? addmod(m, m, br.q) : m;
        }
    }

    // NTT-image operands (natural order, canonical): row k of the tensor formed from the operand rows as they lie -- nothing
    // held, nothing parked; each operand word is read twice (the second time from L2)
    static TFHE_HD void prod_ntt(u64* v, const u64* a0, const u64* a1, const u64* b0, const u64* b1, int k, bool square, const barrett_t& br,
                                 u32 tid) {
#pragma unroll
        for (int e = 0; e < E; e++) {
            const u32 nat = nat_of(tid, e);
            const u64 m = mulmod((k == 2 ? a1 : a0)[nat], (k == 0 ? b0 : b1)[nat], br);
            v[e] = k != 1 ? m : addmod(m, square ? m : mulmod(a1[nat], b0[nat], br), br.q);
        }
    }
    // Two parking rows (N = 2^14, where three rows of 32 words do not fit the 256 registers of a 512-thread workgroup next to a
    // running transform): NTT(a1) goes to p1 as soon as it exists and is streamed back by the products, a1 b0 goes to p2.
    static TFHE_HD void park_row(u64* park, const u64* v, u32 tid) {
#pragma unroll
        for (int e = 0; e < E; e++) park[nat_of(tid, e)] = v[e];
    }
    static TFHE_HD void prod_b0_parked(u64* v, const u64* A0, const u64* p1, u64* p2, const barrett_t& br, u32 tid) {
#pragma unroll
        for (int e = 0; e < E; e++) {
            const u32 nat = nat_of(tid, e);
            p2[nat] = mulmod(v[e], p1[nat], br);
            v[e] = mulmod(v[e], A0[e], br);
        }
    }
    static TFHE_HD void prod_b1_parked(const u64* v, u64* A0, u64* A1, const u64* p1, const u64* p2, const barrett_t& br, u32 tid) {
#pragma unroll
        for (int e = 0; e < E; e++) {
            const u32 nat = nat_of(tid, e);
            A0[e] = addmod(mulmod(v[e], A0[e], br), p2[nat], br.q);
            A1[e] = mulmod(v[e], p1[nat], br);
        }
    }
    // ---- inverse transform from registers: barrier | first | barrier | mid | barrier | last (canonical words to gdst) ----
    static TFHE_HD void inv_first(u64* lds, const A::ctx& C, u32 tid, u64* v) {
        inv_compute<A, LOGB, LOGT, S1, KI1, true, true, 0, -1, no_hook, true>(v, nullptr, nullptr, C, tid, 1u);
        inv_store<A, LOGB, LOGT, S1, KI1, true, true>(v, lds, nullptr, C, tid);
    }
    static TFHE_HD void inv_mid(u64* lds, const A::ctx& C, u32 tid) {
        ntt_inv_pass<A, LOGB, LOGT, S2, KI2, false, false, true>(lds, nullptr, nullptr, C, tid, 1u, 0, 0u);
    }
    static TFHE_HD void inv_last(u64* lds, u64* gdst, const A::ctx& C, u32 tid) {
        ntt_inv_pass<A, LOGB, LOGT, 0, S2, false, true, true>(lds, nullptr, gdst, C, tid, 1u, 0, 0u);
    }
};

#if defined(__HIPCC__)
// u64 counterparts of fused_fwd_to_regs / fused_inv_from_regs (kernels.h), phase by phase
template <int LOGB, int LOGT>
__device__ __forceinline__ void mul_core_forward(u64* lds, const u64* grow, const ArithInt::ctx& C, bool& first, u64* v) {
    typedef mul_core_int<LOGB, LOGT> M;
    const u32 tid = fresh_tid();
    {
        u64 raw[M::E];
        M::fwd_load(raw, grow, tid);
        if (!first) __syncthreads();  // the previous transform's last pass has read LDS
        first = false;
        M::fwd_first(raw, lds, C, tid, v);
    }
    __syncthreads();
    M::fwd_mid(lds, C, tid);
    __syncthreads();
    M::fwd_last(lds, C, tid, v);
}
template <int LOGB, int LOGT>
__device__ __forceinline__ void mul_core_inverse(u64* lds, u64* v, u64* gdst, const ArithInt::ctx& C) {
    typedef mul_core_int<LOGB, LOGT> M;
    const u32 tid = fresh_tid();
    __syncthreads();  // the previous transform's last pass has read LDS
    M::inv_first(lds, C, tid, v);
    __syncthreads();
    M::inv_mid(lds, C, tid);
    __syncthreads();
    M::inv_last(lds, gdst, C, tid);
}

// `sel` lists the u64-policy limbs of the ring (context moduli), alt.idx[j] their positions in the packed ciphertexts
// alt.a / alt.b ([nct][2][alt.ns][N]) and in T ([nct][3][alt.ns][N]); the other limbs' rows are not touched.
// MODE: CORE_SQUARE (alt.b == alt.a: two forward transforms, nothing parked), CORE_NTTIN (operands are NTT images: streamed).
// Registers (tfhe_mul_relin): N <= 2^13 -- two held rows and the running one, a1 b0 parked in the workgroup's
// scratch row (L2) between the third and the fourth forward transform, the allocation of k_bfv_core_fused; N = 2^14 -- ONE
// held row and the running one, NTT(a1) and a1 b0 in two parking rows (scratch: two rows per workgroup); squaring holds two
// rows and parks nothing at every size.
template <int LOGB, int LOGT, int MODE>
__global__ __launch_bounds__(1 << LOGT) void k_mul_core_int(u64* __restrict__ T, u64* __restrict__ scratch, const ntt_limb_t* __restrict__ LT,
                                                             limb_sel_t sel, u32 nitems, core_alt_t alt) {
    extern __shared__ __attribute__((aligned(16))) u64 lds[];
    typedef mul_core_int<LOGB, LOGT> M;
    constexpr int E = M::E;
    constexpr bool SQUARE = (MODE & CORE_SQUARE) != 0, PARK2 = LOGB >= 14;
    const u32 nb = (u32)sel.n, onb = (u32)alt.ns;
    u64* const p1 = scratch + (((size_t)blockIdx.x * (PARK2 ? 2u : 1u)) << LOGB);
    u64* const p2 = p1 + ((size_t)1 << LOGB);
    bool first = true;
    const u32 niter = xcd_limb_niter(gridDim.x, nitems);
    for (u32 it = 0; it < niter; it++) {
        const u32 item = xcd_limb_walk(it, blockIdx.x, gridDim.x, nb, nitems);
        if (item == ~0u) break;
        const u32 b = item / nb, j = item % nb, oj = (u32)alt.idx[j];
        const ntt_limb_t& L = LT[sel.idx[j]];
        const ArithInt::ctx C = ArithInt::make(L);
        const barrett_t br = L.br;
        const size_t s0 = ((size_t)(b * 2 + 0) * onb + oj) << LOGB, s1 = ((size_t)(b * 2 + 1) * onb + oj) << LOGB;
        u64* const t0 = T + (((size_t)(b * 3 + 0) * onb + oj) << LOGB);
        u64* const t1 = T + (((size_t)(b * 3 + 1) * onb + oj) << LOGB);
        u64* const t2 = T + (((size_t)(b * 3 + 2) * onb + oj) << LOGB);
        if constexpr ((MODE & CORE_NTTIN) != 0) {
            u64 v[E];
#pragma unroll
            for (int k = 0; k < 3; k++) {
                M::prod_ntt(v, alt.a + s0, alt.a + s1, alt.b + s0, alt.b + s1, k, SQUARE, br, fresh_tid());
                mul_core_inverse<LOGB, LOGT>(lds, v, k == 0 ? t0 : k == 1 ? t1 : t2, C);
            }
        } else if constexpr (SQUARE) {
            u64 A0[E], A1[E], v[E];
            mul_core_forward<LOGB, LOGT>(lds, alt.a + s0, C, first, A0);
            mul_core_forward<LOGB, LOGT>(lds, alt.a + s1, C, first, A1);
#pragma unroll
            for (int k = 0; k < 3; k++) {
                M::prod_sq(v, A0, A1, k, br);
                mul_core_inverse<LOGB, LOGT>(lds, v, k == 0 ? t0 : k == 1 ? t1 : t2, C);
            }
        } else if constexpr (PARK2) {
            u64 A0[E], v[E];
            mul_core_forward<LOGB, LOGT>(lds, alt.a + s0, C, first, A0);
            mul_core_forward<LOGB, LOGT>(lds, alt.a + s1, C, first, v);
            M::park_row(p1, v, fresh_tid());
            mul_core_forward<LOGB, LOGT>(lds, alt.b + s0, C, first, v);
            M::prod_b0_parked(v, A0, p1, p2, br, fresh_tid());
            mul_core_inverse<LOGB, LOGT>(lds, v, t0, C);
            mul_core_forward<LOGB, LOGT>(lds, alt.b + s1, C, first, v);
            u64 A1[E];
            M::prod_b1_parked(v, A0, A1, p1, p2, br, fresh_tid());
            mul_core_inverse<LOGB, LOGT>(lds, A0, t1, C);
            mul_core_inverse<LOGB, LOGT>(lds, A1, t2, C);
        } else {
            u64 A0[E], A1[E], v[E];
            mul_core_forward<LOGB, LOGT>(lds, alt.a + s0, C, first, A0);
            mul_core_forward<LOGB, LOGT>(lds, alt.a + s1, C, first, A1);
            mul_core_forward<LOGB, LOGT>(lds, alt.b + s0, C, first, v);
            M::prod_b0(v, A0, A1, p1, br, fresh_tid());
            mul_core_inverse<LOGB, LOGT>(lds, v, t0, C);
            mul_core_forward<LOGB, LOGT>(lds, alt.b + s1, C, first, v);
            M::prod_b1(v, A0, A1, p1, br, fresh_tid());
            mul_core_inverse<LOGB, LOGT>(lds, A0, t1, C);
            mul_core_inverse<LOGB, LOGT>(lds, A1, t2, C);
        }
    }
}
#endif  // __HIPCC__
