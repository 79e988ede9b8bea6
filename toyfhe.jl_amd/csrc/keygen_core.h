// keygen_core.h -- tfhe_evalkey_gen: public, relinearisation and Galois keys (rlwe_she.jl:155-166, 273-304; modulusraising.jl:28-32)
// written in the NTT domain, every word exactly once.  Component m = (key k, digit i), m = k n_digits + i, has at limb j
//   evk_k[i][0][j] = NTT_j(a_m)                                                            (mask)
//   evk_k[i][1][j] = gamma[i][j] old^_k[j] - ( NTT_j(a_m) s^[j] + NTT_j(mult_e e_m) )      (masked)
// with gamma a host table of gadget residues (all zero: a public key) and old^ one of: a caller's row, s^ s^ (relinearisation),
// s^ read through galois_ntt_pos (a Galois key: the automorphism is an index permutation without signs in the NTT domain).
//
// Fused form, N = 2^12 .. 2^14: k_evalkey_fused, one (component m, limb j) item per workgroup pass, built from the phases of
// enc_core.h (the transform through registers, its barrier sequences and the item walk: row_core.h).  The per-thread PHASES are plain TFHE_HD functions, so that the CPU
// emulation under tests/keygen_core_emul/ runs the very code of the kernel: one loop over the thread ids per phase.
//   1. the uniform row a_m is generated (or read from the caller's buffer) in place of the forward transform's loads;
//   2. forward transform; 3. row 0 stored, its canonical words kept in registers (N = 2^14: read back from row 0 by the thread
//   that wrote them, as enc_core parks NTT(u));  4. the Gaussian row mult_e e_m generated and transformed;  5. the combine, row 1.
// Traffic per item: one row of s^ read (cache-resident across the components; a Galois key reads it twice, once permuted; an explicit
// `old` adds one row, only where gamma[i][j] != 0) and two rows written.  With given randomness one more row (a_m) and N int32 read.
// Where gamma[i][j] == 0 -- every off-diagonal item of the RNS gadget, every item of a public key -- the old term is skipped, not
// multiplied by zero.
//
// Ranges.  u64 policy (ArithInt): as row_core.h -- the forward passes keep [0, 4q), the last one canonicalises; every product of two
// data words (a^ s^, gamma old^, s^ s^) goes through the limb's Barrett constants and is canonical; sums and differences are
// addmod / negmod of canonical words.
// fp64 policy (ArithFp, moduli below TFHE_FP_QMAX; the plan of fp64arith.h is entered at its stated point and nowhere else):
//   a_m      enters the forward transform as its canonical residue, uncentred, |v| < p: the FIRST entry of the forward sweep plan
//            (fp_fwd_sweep_before starts from the bound b = 1.0 p), the entry tfhe_nntt itself uses for a row of residues and the one
//            enc_core.h uses for u.  A row centred to |v| <= p / 2 would enter below that bound; the plan places its sweeps for 1.0 p,
//            so no centring pass is spent on it.  The last pass canonicalises (out_fwd).
//   mult_e e enters the same way: gauss_residue is canonical.
//   combine  works on the canonical words the two transforms left, in integers (Barrett, addmod, negmod): no double ever holds a
//            product of two data words, and nothing re-enters the fp64 plan.
// So the largest |operand| / p that enters an fp64 product or reduction is that of a plain forward transform (< TFHE_FP_LIMIT);
// tests/test_keygen_cpu.py runs the phases at the top of the fp64 class with growth-maximising rows and range tracking on.
//
// Resources (gfx950; tests/test_keygen_cpu.py reads them from the compiler): the LDS image is the transform's padded row,
// lds_words<LOGB, LOGT>() * 8 = 34.8 / 67.6 / 135.3 KB at 2^12 / 2^13 / 2^14 -- at 2^14 one workgroup of 512 threads per CU next to
// the 160 KiB of LDS, at 2^12 four; no static LDS, no scratch.  A thread's E words of a row lie 2^(LOGB - K3) words apart
// (nat_of), so a wave's store of register e covers 64 consecutive words (512 B): full lines, 8-byte accesses per lane -- the same
// map the fused encryption stores and parks through; 16-byte accesses would need a second LDS exchange.
//
// Composed form (every other size): k_key_fill writes a_m and the residues of mult_e e_m into rows 0 and 1 of the output buffer
// itself, one in-place batched forward transform runs over them, k_key_finish applies row 1 <- gamma old^ - (row 0 s^ + row 1).
// Per item: 2 rows written, 2 read + 2 written by the transform, 2 (+ s^, + old^) read and 1 written by the finish.
#pragma once
#include "enc_core.h"

struct key_rand_t {
    const u64* mask_rand;       // != nullptr: [n_keys][n_digits][key_limbs][N] canonical residues, coefficient domain
    const int32_t* noise_rand;  // != nullptr: [n_keys][n_digits][N] signed
    double sigma_e;
    u64 mult_e, seed, mask_poly, noise_poly, poly_stride;
    u32 stream_mask, stream_noise;
};
// tab (device): [n_keys] output pointers | [n_keys] Galois elements (0: s^ s^) | [n_digits][key_limbs] gadget residues
struct key_arg_t {
    const u64* secret;   // [key_limbs][N], NTT domain
    const u64* old;      // [n_keys][key_limbs][N], NTT domain, or nullptr
    const u64* tab;
    u32 n_keys, n_digits, key_limbs;
    u32 gadget;          // 0: public-key form (gamma = 0 everywhere)
    u64 m0;              // first component of this launch
};
enum { KEY_OLD_NONE = 0, KEY_OLD_ROW = 1, KEY_OLD_SQUARE = 2, KEY_OLD_GALOIS = 3 };

TFHE_HD u64* key_out(const key_arg_t& K, u32 k) { return (u64*)(uintptr_t)K.tab[k]; }
TFHE_HD u64 key_galois(const key_arg_t& K, u32 k) { return K.tab[(size_t)K.n_keys + k]; }
TFHE_HD u64 key_gamma(const key_arg_t& K, u32 i, u32 j) { return K.gadget ? K.tab[(size_t)2 * K.n_keys + (size_t)i * K.key_limbs + j] : 0; }
// where old^ of an item with gadget residue g comes from
TFHE_HD int key_old_mode(const key_arg_t& K, u32 k, u64 g) {
    if (!g) return KEY_OLD_NONE;
    if (K.old) return KEY_OLD_ROW;
    return key_galois(K, k) ? KEY_OLD_GALOIS : KEY_OLD_SQUARE;
}
// word `pos` of a_m at limb j / the signed integer e_m at coefficient pos (m: index in the whole call)
template <bool RAND>
TFHE_HD u64 key_mask_word(const key_rand_t& R, u64 m, u32 j, u32 key_limbs, u32 pos, u32 logn, u64 q) {
    if (RAND) return R.mask_rand[(((size_t)m * key_limbs + j) << logn) + pos];
    return sample_uniform_mod(((R.mask_poly + m * R.poly_stride) << 32) | pos, j, R.stream_mask, R.seed, q);
}
template <bool RAND>
TFHE_HD long long key_noise_int(const key_rand_t& R, u64 m, u32 pos, u32 logn) {
    if (RAND) return (long long)R.noise_rand[((size_t)m << logn) + pos];
    return sample_gauss_int(((R.noise_poly + m * R.poly_stride) << 32) | pos, R.stream_noise, R.seed, R.sigma_e);
}
// old^ at NTT position nat of limb row s (the secret's) / o (the caller's row)
template <int MODE>
TFHE_HD u64 key_old_word(const u64* s, const u64* o, u64 sw, u32 nat, u64 gel, u32 n, const barrett_t& br) {
    if (MODE == KEY_OLD_ROW) return o[nat];
    if (MODE == KEY_OLD_SQUARE) return mulmod(sw, sw, br);
    return s[galois_ntt_pos(nat, gel, n)];
}

template <class A, int LOGB, int LOGT>
struct key_core {
    typedef enc_core<A, LOGB, LOGT> M;
    static constexpr int E = M::E;
    static constexpr bool PARK = M::PARK;

    // a_m / mult_e e_m as canonical residues, written to the LDS words the thread's own first pass reads (no barrier between the two).
    // ROLLED loops, as enc_core::u_form: a draw is a Philox block (plus log, sqrt and cos in doubles for the Gaussian).
    static TFHE_HD void mask_form(u64* lds, const key_rand_t& R, u64 m, u32 j, u32 key_limbs, u64 q, u32 tid) {
#pragma unroll 2
        for (int e = 0; e < E; e++) {
            const u32 pos = M::src_of(tid, e);
            lds[lds_phi<LOGB, LOGT>(pos)] = key_mask_word<false>(R, m, j, key_limbs, pos, LOGB, q);
        }
    }
    template <bool RAND>
    static TFHE_HD void noise_form(u64* lds, const key_rand_t& R, u64 m, u64 mq, const barrett_t& br, u32 tid) {
#pragma unroll 2
        for (int e = 0; e < E; e++) {
            const u32 pos = M::src_of(tid, e);
            lds[lds_phi<LOGB, LOGT>(pos)] = gauss_residue(key_noise_int<RAND>(R, m, pos, LOGB), mq, br);
        }
    }
    // row 0: the canonical words of NTT(a_m), natural order
    static TFHE_HD void store_mask(u64* row0, const u64* ah, u32 tid) { M::park_row(row0, ah, tid); }
    // row 1 <- gamma old^ - (a^ s^ + e^); a^ from registers, or (PARK) from the row 0 words this thread stored.  Eight registers
    // per piece, as enc_core::dec_acc_ntt: one loop over all E with up to three Barrett products is left rolled (scratch).
    template <int MODE, int E0 = 0>
    static TFHE_HD void combine_m(u64* row1, const u64* row0, const u64* ah, const u64* eh, const u64* s, const u64* o, u64 g, u64 gel,
                                  const barrett_t& br, u32 tid) {
#pragma unroll
        for (int i = 0; i < 8; i++) {
            const u32 nat = M::nat_of(tid, E0 + i);
            const u64 sw = s[nat];
            const u64 aw = PARK ? row0[nat] : ah[E0 + i];
            u64 r = negmod(addmod(mulmod(aw, sw, br), eh[E0 + i], br.q), br.q);
            if (MODE != KEY_OLD_NONE) r = addmod(r, mulmod(g, key_old_word<MODE>(s, o, sw, nat, gel, 1u << LOGB, br), br), br.q);
            row1[nat] = r;
        }
        TFHE_SCHED_FENCE();
        if constexpr (E0 + 8 < E) combine_m<MODE, E0 + 8>(row1, row0, ah, eh, s, o, g, gel, br, tid);
    }
    static TFHE_HD void combine(int mode, u64* row1, const u64* row0, const u64* ah, const u64* eh, const u64* s, const u64* o, u64 g, u64 gel,
                                const barrett_t& br, u32 tid) {
        switch (mode) {   // (workgroup-uniform)
            case KEY_OLD_NONE: combine_m<KEY_OLD_NONE>(row1, row0, ah, eh, s, o, g, gel, br, tid); break;
            case KEY_OLD_ROW: combine_m<KEY_OLD_ROW>(row1, row0, ah, eh, s, o, g, gel, br, tid); break;
            case KEY_OLD_SQUARE: combine_m<KEY_OLD_SQUARE>(row1, row0, ah, eh, s, o, g, gel, br, tid); break;
            default: combine_m<KEY_OLD_GALOIS>(row1, row0, ah, eh, s, o, g, gel, br, tid); break;
        }
    }
};

#if defined(__HIPCC__)
// `sel` lists the limbs of this launch's policy; items are (component, selected limb), components K.m0 .. K.m0 + nitems / sel.n - 1 of
// the whole call (the pointers and counters are those of the whole call).
template <class A, int LOGB, int LOGT, bool RAND>
__global__ __launch_bounds__(1 << LOGT) void k_evalkey_fused(const ntt_limb_t* __restrict__ LT, limb_sel_t sel, u32 nitems, key_arg_t K,
                                                              key_rand_t R) {
    extern __shared__ __attribute__((aligned(16))) u64 lds[];
    typedef key_core<A, LOGB, LOGT> KC;
    typedef typename KC::M M;
    constexpr int E = M::E;
    const u32 nb = (u32)sel.n;
    bool first = true;
    for (u32 it = 0, item; row_item(it, nb, nitems, item); it++) {
        const u32 j = (u32)sel.idx[item % nb];
        const u64 m = K.m0 + item / nb;
        const u32 k = (u32)(m / K.n_digits), i = (u32)(m % K.n_digits);
        const ntt_limb_t& L = LT[j];
        const typename A::ctx C = A::make(L);
        const barrett_t br = L.br;
        u64* const row0 = key_out(K, k) + ((((size_t)i * 2 + 0) * K.key_limbs + j) << LOGB);
        u64* const row1 = key_out(K, k) + ((((size_t)i * 2 + 1) * K.key_limbs + j) << LOGB);
        const u64* const s = K.secret + ((size_t)j << LOGB);
        const u64 g = key_gamma(K, i, j), gel = key_galois(K, k);
        const int mode = key_old_mode(K, k, g);
        const u64* const o = K.old ? K.old + (((size_t)k * K.key_limbs + j) << LOGB) : nullptr;
        u64 ah[E], eh[E];
        {
            u64 raw[E];
            if constexpr (RAND) {
                M::fwd_load(raw, R.mask_rand + ((m * K.key_limbs + j) << LOGB), fresh_tid());
            } else {
                if (!first) __syncthreads();  // the previous transform's last pass has read LDS
                KC::mask_form(lds, R, m, j, K.key_limbs, br.q, fresh_tid());
                M::u_load(raw, lds, fresh_tid());
                first = true;                 // (that barrier is done)
            }
            row_forward<A, LOGB, LOGT>(lds, raw, C, first, ah);
        }
        KC::store_mask(row0, ah, fresh_tid());
        {
            u64 raw[E];
            __syncthreads();                  // the mask's last pass has read LDS
            KC::template noise_form<RAND>(lds, R, m, R.mult_e % br.q, br, fresh_tid());
            M::u_load(raw, lds, fresh_tid());
            first = true;
            row_forward<A, LOGB, LOGT>(lds, raw, C, first, eh);
        }
        KC::combine(mode, row1, row0, ah, eh, s, o, g, gel, br, fresh_tid());
    }
}

// ---- the composed form: two streaming kernels around one in-place batched forward transform -----------------------------------------
// rows 0 / 1 of component m = K.m0 + blockIdx.y <- a_m / the residues of mult_e e_m, every limb, coefficient domain
template <bool RAND>
__global__ __launch_bounds__(256) void k_key_fill(const ntt_limb_t* __restrict__ LT, u32 logn, key_arg_t K, key_rand_t R) {
    const u32 pos = blockIdx.x * 256 + threadIdx.x, n = 1u << logn;
    if (pos >= n) return;
    const u64 m = K.m0 + blockIdx.y;
    const u32 k = (u32)(m / K.n_digits), i = (u32)(m % K.n_digits);
    u64* const c0 = key_out(K, k) + (((size_t)i * 2 * K.key_limbs) << logn) + pos;
    u64* const c1 = c0 + ((size_t)K.key_limbs << logn);
    const long long e = key_noise_int<RAND>(R, m, pos, logn);
    for (u32 l = 0; l < K.key_limbs; l++) {
        const barrett_t br = LT[l].br;
        c0[(size_t)l << logn] = key_mask_word<RAND>(R, m, l, K.key_limbs, pos, logn, br.q);
        c1[(size_t)l << logn] = gauss_residue(e, R.mult_e % br.q, br);
    }
}
// row 1 <- gamma old^ - (row 0 s^ + row 1) on the NTT images; limb l = blockIdx.y, component m = K.m0 + blockIdx.z
__global__ __launch_bounds__(256) void k_key_finish(const ntt_limb_t* __restrict__ LT, u32 logn, key_arg_t K) {
    const u32 pos = blockIdx.x * 256 + threadIdx.x, l = blockIdx.y, n = 1u << logn;
    if (pos >= n) return;
    const u64 m = K.m0 + blockIdx.z;
    const u32 k = (u32)(m / K.n_digits), i = (u32)(m % K.n_digits);
    const barrett_t br = LT[l].br;
    const u64* const c0 = key_out(K, k) + ((((size_t)i * 2 + 0) * K.key_limbs + l) << logn);
    u64* const c1 = key_out(K, k) + ((((size_t)i * 2 + 1) * K.key_limbs + l) << logn);
    const u64* const s = K.secret + ((size_t)l << logn);
    const u64* const o = K.old ? K.old + (((size_t)k * K.key_limbs + l) << logn) : nullptr;
    const u64 g = key_gamma(K, i, l), gel = key_galois(K, k), sw = s[pos];
    u64 r = negmod(addmod(mulmod(c0[pos], sw, br), c1[pos], br.q), br.q);
    switch (key_old_mode(K, k, g)) {
        case KEY_OLD_NONE: break;
        case KEY_OLD_ROW: r = addmod(r, mulmod(g, key_old_word<KEY_OLD_ROW>(s, o, sw, pos, gel, n, br), br), br.q); break;
        case KEY_OLD_SQUARE: r = addmod(r, mulmod(g, key_old_word<KEY_OLD_SQUARE>(s, o, sw, pos, gel, n, br), br), br.q); break;
        default: r = addmod(r, mulmod(g, key_old_word<KEY_OLD_GALOIS>(s, o, sw, pos, gel, n, br), br), br.q); break;
    }
    c1[pos] = r;
}
#endif  // __HIPCC__
