// enc_core.h -- the two ends of a pipeline as fused row kernels, N = 2^12 .. 2^14, both arithmetic policies:
//   tfhe_encrypt        out_b = ( INTT(masked . NTT(u_b)) + e1_b (+ msg_b),  INTT(mask . NTT(u_b)) + e2_b )      (rlwe_she.jl:176-195)
//   tfhe_decrypt_phase  out_b = c1_b + INTT( s . NTT(c2_b) (+ s^2 . NTT(c3_b)) )                                 (rlwe_she.jl:199-212)
// for one (ciphertext b, limb j) per workgroup pass.  The transform through registers -- schedule, register map, passes, the two
// barrier sequences, the item walk -- is row_core.h; enc_core adds the phases that are encryption's own (u_form, the key products,
// the decryption sums, the last pass with the noise in its store).  The per-thread PHASES (everything between two barriers) are
// plain TFHE_HD functions, so that the CPU emulation under tests/enc_core_emul/ runs the very code of the kernels.
//
// Ranges.  u64 policy (ArithInt): as row_core.h; a data x data product goes through Barrett and is canonical.
// fp64 policy (ArithFp, moduli up to TFHE_FP_QMAX; the plan of fp64arith.h is entered at its stated points and nowhere else):
//   u        enters the forward transform as the canonical residue of the signed integer, |v| <= 1 p: the entry the forward
//            sweep plan (fp_fwd_sweep_before) is made for; the last pass canonicalises (out_fwd);
//   products NTT(u) x key word, s x NTT(c), s x s are Barrett products of canonical words (ntt_limb_t::br, valid for every
//            limb) and their sums are canonical: no double ever holds a product of two data words;
//   inverse  takes the centred double of that canonical word, |v| <= p / 2: the entry (0.502) of make_inv_plan;
//   noise and message are added to the CANONICAL result of the inverse in integers (addmod), after the final reduction.
// So the largest |operand| / p that enters an fp64 product or reduction is that of a plain transform (< TFHE_FP_LIMIT);
// tests/test_encrypt_cpu.py runs the phases at TFHE_FP_QMAX with growth-maximising operands and range tracking on.
//
// Randomness: `u`, `e1`, `e2` of ciphertext b are the polynomials first_poly + b, first_poly + batch + b, first_poly + 2 batch + b
// of the Gaussian stream of sample_kernels.h (the words three tfhe_sample_gaussian calls would have written), regenerated
// where they are needed -- in place of the forward transform's load for u, at the last inverse pass's store for e -- or read
// from a caller's int32 [batch][3][N] buffer.  No source row exists in memory: the words pass through the workgroup's LDS image.
#pragma once
#include "row_core.h"
#include "sample_kernels.h"

struct enc_rand_t {
    const int32_t* rand;   // != nullptr: [batch][3][N] signed (u, e1, e2); the stream below is not used
    double sigma_u, sigma_e;
    u64 mult_e, seed, first_poly;
    u32 stream;
    u64 batch;             // of the whole call (the counter convention), b0: first ciphertext of this launch
    u64 b0;
};
// the signed integer of polynomial k (0: u, 1: e1, 2: e2) of ciphertext b (index in the whole call) at coefficient pos
template <bool RAND>
TFHE_HD long long enc_small(const enc_rand_t& R, u64 b, int k, u32 pos, u32 logn) {
    if (RAND) return (long long)R.rand[(((size_t)b * 3 + (size_t)k) << logn) + pos];
    return sample_gauss_int(((R.first_poly + (u64)k * R.batch + b) << 32) | pos, R.stream, R.seed, k == 0 ? R.sigma_u : R.sigma_e);
}

template <class A, int LOGB, int LOGT>
struct enc_core : row_core<A, LOGB, LOGT> {
    typedef row_core<A, LOGB, LOGT> B;
    using B::E;
    using B::nat_of;
    using B::src_of;
    using B::dst_of;
    using B::S2;
    typedef typename B::elem elem;
    typedef typename B::actx actx;

    // u of ciphertext b as canonical residues mod q, written to the LDS words the thread's own first pass reads (no barrier between
    // the two: a thread reads back what it wrote).  A ROLLED loop: a Gaussian draw is a Philox block plus log, sqrt and cos in
    // doubles, and E (16 or 32) of them unrolled side by side do not fit the registers; the LDS word takes the dynamic index.
    template <bool RAND>
    static TFHE_HD void u_form(u64* lds, const enc_rand_t& R, u64 b, const barrett_t& br, u32 tid) {
#pragma unroll 2
        for (int e = 0; e < E; e++) {
            const u32 pos = src_of(tid, e);
            lds[lds_phi<LOGB, LOGT>(pos)] = gauss_residue(enc_small<RAND>(R, b, 0, pos, LOGB), 1, br);
        }
    }
    // ---- products: canonical words in, the inverse transform's operand out ----
    static TFHE_HD void prod_key(elem* v, const u64* uh, const u64* key, const barrett_t& br, const actx& C, u32 tid) {
#pragma unroll
        for (int e = 0; e < E; e++) v[e] = A::from_global(mulmod(uh[e], key[nat_of(tid, e)], br), C);
    }
    // acc <- s ch (FIRST) or acc + s^2 ch, with s^2 formed from the s word in hand
    template <bool FIRST>
    static TFHE_HD void dec_acc(u64* acc, const u64* ch, const u64* s, const barrett_t& br, u32 tid) {
#pragma unroll
        for (int e = 0; e < E; e++) {
            const u64 sw = s[nat_of(tid, e)];
            acc[e] = FIRST ? mulmod(ch[e], sw, br) : addmod(acc[e], mulmod(ch[e], mulmod(sw, sw, br), br), br.q);
        }
    }
    // NTT-image ciphertexts: c1 + s c2 (+ s^2 c3) from the rows as they lie.  Eight registers per instantiation: one loop over all E
    // with three Barrett products in its body is past the size up to which the compiler unrolls completely, and a loop left
    // rolled indexes `acc` dynamically (scratch memory).
    template <int POLYS, int E0 = 0>
    static TFHE_HD void dec_acc_ntt(u64* acc, const u64* c1, const u64* c2, const u64* c3, const u64* s, const barrett_t& br, u32 tid) {
#pragma unroll
        for (int i = 0; i < 8; i++) {
            const u32 nat = nat_of(tid, E0 + i);
            const u64 sw = s[nat];
            u64 r = addmod(c1[nat], mulmod(c2[nat], sw, br), br.q);
            if (POLYS == 3) r = addmod(r, mulmod(c3[nat], mulmod(sw, sw, br), br), br.q);
            acc[E0 + i] = r;
        }
        TFHE_SCHED_FENCE();   // the next piece's loads stay behind this one's: 8 words of each row in flight, not E
        if constexpr (E0 + 8 < E) dec_acc_ntt<POLYS, E0 + 8>(acc, c1, c2, c3, s, br, tid);
    }
    // last pass of an encryption: + mult_e e_k (sampled or read here) + msg in the store.  The canonical results go back to the LDS
    // words the pass read them from (a thread's own), and a rolled loop -- see u_form -- finishes and stores them.
    template <bool RAND>
    static TFHE_HD void inv_last_noise(u64* lds, u64* gdst, const u64* msg, const actx& C, const enc_rand_t& R, u64 b, int k, u64 mq,
                                       const barrett_t& br, u32 tid) {
        {
            u64 raw[E], o[E];
            elem v[E];
            inv_load_data<LOGB, LOGT, 0, S2, false>(raw, lds, nullptr, tid, 0, 0u);
            inv_compute<A, LOGB, LOGT, 0, S2, false, true, 0>(v, raw, nullptr, C, tid, 1u);
            inv_store<A, LOGB, LOGT, 0, S2, false, true>(v, nullptr, nullptr, C, tid, nullptr, o);
#pragma unroll
            for (int e = 0; e < E; e++) lds[lds_phi<LOGB, LOGT>(dst_of(tid, e))] = o[e];
        }
#pragma unroll 2
        for (int e = 0; e < E; e++) {
            const u32 pos = dst_of(tid, e);
            u64 r = addmod(lds[lds_phi<LOGB, LOGT>(pos)], gauss_residue(enc_small<RAND>(R, b, k, pos, LOGB), mq, br), br.q);
            if (msg) r = addmod(r, msg[pos], br.q);
            gdst[pos] = r;
        }
    }
    // N = 2^14: NTT(u) waits in the second component's output row (which the last store overwrites) between the two products,
    // not in registers next to a running inverse transform; a thread reads back its own words only
    static constexpr bool PARK = LOGB >= 14;
    static TFHE_HD void prod_key_parked(elem* v, const u64* park, const u64* key, const barrett_t& br, const actx& C, u32 tid) {
#pragma unroll
        for (int e = 0; e < E; e++) {
            const u32 nat = nat_of(tid, e);
            v[e] = A::from_global(mulmod(park[nat], key[nat], br), C);
        }
    }
};

#if defined(__HIPCC__)
// `sel` lists the limbs of this launch's policy (positions in the ring = context moduli: the ring is a prefix of its context);
// items are (ciphertext, selected limb).  pk [2][key_limbs][N] (mask, masked), msg [batch][level][N] or nullptr,
// out [batch][2][level][N]; the pointers are those of the whole call, R.b0 is the launch's first ciphertext.
template <class A, int LOGB, int LOGT, bool RAND>
__global__ __launch_bounds__(1 << LOGT) void k_encrypt_fused(u64* __restrict__ out, const u64* __restrict__ pk, const u64* __restrict__ msg,
                                                              const ntt_limb_t* __restrict__ LT, limb_sel_t sel, u32 nitems, u32 key_limbs,
                                                              u32 level, enc_rand_t R) {
    extern __shared__ __attribute__((aligned(16))) u64 lds[];
    typedef enc_core<A, LOGB, LOGT> M;
    constexpr int E = M::E;
    const u32 nb = (u32)sel.n;
    bool first = true;
    for (u32 it = 0, item; row_item(it, nb, nitems, item); it++) {
        const u32 j = (u32)sel.idx[item % nb];
        const u64 b = R.b0 + item / nb;
        const ntt_limb_t& L = LT[j];
        const typename A::ctx C = A::make(L);
        const barrett_t br = L.br;
        const u64 mq = R.mult_e % br.q;
        u64* const o0 = out + (((b * 2 + 0) * level + j) << LOGB);
        u64* const o1 = out + (((b * 2 + 1) * level + j) << LOGB);
        const u64* const masked = pk + (((size_t)key_limbs + j) << LOGB);
        const u64* const mask = pk + ((size_t)j << LOGB);
        u64 uh[E];
        {
            if (!first) __syncthreads();  // the previous transform's last pass has read LDS
            M::template u_form<RAND>(lds, R, b, br, fresh_tid());
            u64 raw[E];
            M::u_load(raw, lds, fresh_tid());
            first = true;                 // (that barrier is done)
            row_forward<A, LOGB, LOGT>(lds, raw, C, first, uh);
        }
        typename A::elem v[E];
        M::prod_key(v, uh, masked, br, C, fresh_tid());
        if constexpr (M::PARK) M::park_row(o1, uh, fresh_tid());
        row_inverse_head<A, LOGB, LOGT>(lds, v, C, first);
        M::template inv_last_noise<RAND>(lds, o0, msg ? msg + ((b * level + j) << LOGB) : nullptr, C, R, b, 1, mq, br, fresh_tid());
        if constexpr (M::PARK) M::prod_key_parked(v, o1, mask, br, C, fresh_tid());
        else M::prod_key(v, uh, mask, br, C, fresh_tid());
        row_inverse_head<A, LOGB, LOGT>(lds, v, C, first);
        M::template inv_last_noise<RAND>(lds, o1, nullptr, C, R, b, 2, mq, br, fresh_tid());
    }
}

// (POLYS = 3 with NTTIN is not built at N = 2^14: four streamed rows next to the held sums and a running inverse transform leave the
// registers -- 80 B of scratch per lane -- so that form runs the composed path, enc_api.inc.)
// ct [batch][POLYS][level][N] (NTTIN: NTT images), secret [key_limbs][N] (NTT image), out [batch][level][N]; whole-call pointers
template <class A, int LOGB, int LOGT, int POLYS, bool NTTIN>
__global__ __launch_bounds__(1 << LOGT) void k_decrypt_fused(u64* __restrict__ out, const u64* __restrict__ ct, const u64* __restrict__ secret,
                                                              const ntt_limb_t* __restrict__ LT, limb_sel_t sel, u32 nitems, u32 level, u64 b0) {
    extern __shared__ __attribute__((aligned(16))) u64 lds[];
    typedef enc_core<A, LOGB, LOGT> M;
    constexpr int E = M::E;
    const u32 nb = (u32)sel.n;
    bool first = true;
    for (u32 it = 0, item; row_item(it, nb, nitems, item); it++) {
        const u32 j = (u32)sel.idx[item % nb];
        const u64 b = b0 + item / nb;
        const ntt_limb_t& L = LT[j];
        const typename A::ctx C = A::make(L);
        const barrett_t br = L.br;
        const u64* const s = secret + ((size_t)j << LOGB);
        const u64* const c1 = ct + (((b * POLYS + 0) * level + j) << LOGB);
        const u64* const c2 = ct + (((b * POLYS + 1) * level + j) << LOGB);
        const u64* const c3 = ct + (((b * POLYS + (POLYS - 1)) * level + j) << LOGB);
        u64 acc[E];
        if constexpr (NTTIN) {
            M::template dec_acc_ntt<POLYS>(acc, c1, c2, c3, s, br, fresh_tid());
        } else {
            u64 ch[E];
            {
                u64 raw[E];
                M::fwd_load(raw, c2, fresh_tid());
                row_forward<A, LOGB, LOGT>(lds, raw, C, first, ch);
            }
            M::template dec_acc<true>(acc, ch, s, br, fresh_tid());
            if constexpr (POLYS == 3) {
                u64 raw[E];
                M::fwd_load(raw, c3, fresh_tid());
                row_forward<A, LOGB, LOGT>(lds, raw, C, first, ch);
                M::template dec_acc<false>(acc, ch, s, br, fresh_tid());
            }
        }
        typename A::elem v[E];
        M::to_elem(v, acc, C);
        row_inverse_head<A, LOGB, LOGT>(lds, v, C, first);
        M::inv_last(lds, out + ((b * level + j) << LOGB), C, fresh_tid(), NTTIN ? nullptr : c1);
    }
}

// ---- the composed form (every other size): three streaming kernels around the batched transforms ---------------------------------
// u [nb][level][N]: the residues of u_b in every limb (b = b0 + blockIdx.y)
template <bool RAND>
__global__ __launch_bounds__(256) void k_enc_fill(u64* __restrict__ u, const ntt_limb_t* __restrict__ LT, u32 level, u32 logn, enc_rand_t R) {
    const u32 k = blockIdx.x * 256 + threadIdx.x, n = 1u << logn;
    const u64 p = blockIdx.y;
    if (k >= n) return;
    const long long e = enc_small<RAND>(R, R.b0 + p, 0, k, logn);
    for (u32 l = 0; l < level; l++) u[((p * level + l) << logn) + k] = gauss_residue(e, 1, LT[l].br);
}
// P [nb][2][level][N] <- NTT(u) x (masked row, mask row) of limb l = blockIdx.y: the key row is indexed, never broadcast
__global__ __launch_bounds__(256) void k_enc_keymul(u64* __restrict__ P, const u64* __restrict__ uh, const u64* __restrict__ pk,
                                                    const ntt_limb_t* __restrict__ LT, u32 level, u32 key_limbs, u32 logn) {
    const u32 k = blockIdx.x * 256 + threadIdx.x, l = blockIdx.y, n = 1u << logn;
    const u64 p = blockIdx.z;
    if (k >= n) return;
    const barrett_t br = LT[l].br;
    const u64 w = uh[((p * level + l) << logn) + k];
    P[(((p * 2 + 0) * level + l) << logn) + k] = mulmod(w, pk[(((size_t)key_limbs + l) << logn) + k], br);
    P[(((p * 2 + 1) * level + l) << logn) + k] = mulmod(w, pk[((size_t)l << logn) + k], br);
}
// out [nb][2][level][N] (the launch's ciphertexts) += mult_e e_{1 + comp} (+ msg for component 0), in place; blockIdx.y = 2 p + comp
template <bool RAND>
__global__ __launch_bounds__(256) void k_enc_finish(u64* __restrict__ out, const u64* __restrict__ msg, const ntt_limb_t* __restrict__ LT,
                                                    u32 level, u32 logn, enc_rand_t R) {
    const u32 k = blockIdx.x * 256 + threadIdx.x, n = 1u << logn, comp = blockIdx.y & 1u;
    const u64 p = blockIdx.y >> 1;
    if (k >= n) return;
    const long long e = enc_small<RAND>(R, R.b0 + p, 1 + (int)comp, k, logn);
    for (u32 l = 0; l < level; l++) {
        const barrett_t br = LT[l].br;
        const size_t at = (((p * 2 + comp) * level + l) << logn) + k;
        u64 r = addmod(out[at], gauss_residue(e, R.mult_e % br.q, br), br.q);
        if (msg && comp == 0) r = addmod(r, msg[((p * level + l) << logn) + k], br.q);
        out[at] = r;
    }
}
// B [nb][level][N] <- c1 + s c2 (+ s^2 c3) on NTT images F [nb][polys][level][N]; secret [key_limbs][N]
__global__ __launch_bounds__(256) void k_dec_keymul(u64* __restrict__ B, const u64* __restrict__ F, const u64* __restrict__ secret,
                                                    const ntt_limb_t* __restrict__ LT, u32 level, u32 polys, u32 logn) {
    const u32 k = blockIdx.x * 256 + threadIdx.x, l = blockIdx.y, n = 1u << logn;
    const u64 p = blockIdx.z;
    if (k >= n) return;
    const barrett_t br = LT[l].br;
    const u64 sw = secret[((size_t)l << logn) + k];
    u64 r = addmod(F[(((p * polys + 0) * level + l) << logn) + k], mulmod(F[(((p * polys + 1) * level + l) << logn) + k], sw, br), br.q);
    if (polys == 3) r = addmod(r, mulmod(F[(((p * polys + 2) * level + l) << logn) + k], mulmod(sw, sw, br), br), br.q);
    B[((p * level + l) << logn) + k] = r;
}
#endif  // __HIPCC__
