// mul_core.h -- the fused product core of tfhe_mul_relin for the u64 policy (ArithInt: moduli from TFHE_FP_QMAX up to 2^62),
// N = 2^12 .. 2^14:   T_k[b][j] = INTT_j( tensor_k( NTT_j(a0), NTT_j(a1), NTT_j(b0), NTT_j(b1) ) ),  k = 0, 1, 2
// (enc_mul, rlwe_she.jl:255-258, with mul_expand / mul_contract the identity: CKKS, BGV) for one (ciphertext b, limb j) per
// workgroup pass -- the u64 counterpart of k_bfv_core_fused (kernels.h).  The transform through registers -- schedule, register
// map, passes, the two barrier sequences -- is row_core<ArithInt, LOGB, LOGT> (row_core.h); this file holds the product phases,
// the kernel with its four branches and the parking-row layout.
//
// The per-thread PHASES (everything between two barriers) are plain TFHE_HD functions, so that the CPU emulation under
// tests/mul_core_emul/ runs the very code of the kernel: one loop over the thread ids per phase.  The kernel itself is device
// code (needs kernels.h) and is compiled only under hipcc.
//
// Ranges: as row_core.h.  The forward transform's last pass canonicalises because a data x data product goes through Barrett
// (ntt_limb_t::br), whose window z < 2^(k+62) admits q^2 but not (4q) q at 61- and 62-bit moduli.
#pragma once
#include "row_core.h"

template <int LOGB, int LOGT>
struct mul_core_int : row_core<ArithInt, LOGB, LOGT> {
    typedef row_core<ArithInt, LOGB, LOGT> B;
    using B::E;
    using B::nat_of;

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
};

#if defined(__HIPCC__)
// a row from memory to its canonical NTT image in registers / a row of canonical products back to memory (row_core.h)
template <int LOGB, int LOGT>
__device__ __forceinline__ void mul_core_forward(u64* lds, const u64* grow, const ArithInt::ctx& C, bool& first, u64* v) {
    u64 raw[mul_core_int<LOGB, LOGT>::E];
    mul_core_int<LOGB, LOGT>::fwd_load(raw, grow, fresh_tid());
    row_forward<ArithInt, LOGB, LOGT>(lds, raw, C, first, v);
}
template <int LOGB, int LOGT>
__device__ __forceinline__ void mul_core_inverse(u64* lds, u64* v, u64* gdst, const ArithInt::ctx& C) {
    bool first = false;   // always the opening barrier: only the NTT-input forms could ever skip it, once per workgroup
    row_inverse_head<ArithInt, LOGB, LOGT>(lds, v, C, first);
    mul_core_int<LOGB, LOGT>::inv_last(lds, gdst, C, fresh_tid());
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
    // (row_item's walk without its readfirstlane: this kernel's register figures were taken with the item number as it is)
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
