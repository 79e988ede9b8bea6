// plain_core.h -- per-coefficient bodies of the BFV / BGV plaintext codecs and of the BFV noise remainder.
//
// Reference semantics (exact integers; Q = product of the ring's moduli, x in [0, Q) the CRT value of one coefficient,
// centred(x) = x - Q if x > Q÷2 else x, signedmod.jl:12-19):
//   BFV π⁻¹ (bfv.jl:21-24)   : Δ (m mod t) with Δ = Q ÷ t, per limb  (m mod t)(Δ mod q_l) mod q_l
//   BGV π⁻¹ (bgv.jl:21-25)   : (m mod t) mod q_l
//   BFV π   (bfv.jl:26-29)   : y = div(centred(x), Δ, RoundNearestTiesAway) (div_hacks.jl:120-135), result mod(SignedMod(y), t)
//   BGV π   (bgv.jl:21-25)   : centred(x) mod t
//   noise   (bfv.jl:137-166) : birem(x) = r if r <= Δ÷2 else Δ - r, r = x mod Δ of the UNSIGNED x
//
// The exact lift x comes from the base-conversion machinery of conv_core.h (conv_prepare + conv_words; BGV: the centred
// conv_prepare + conv_eval to the single target t).  The bodies below restate those three steps with every limb / word loop
// unrolled to a compile-time bound KM (KM >= the ring's limbs), so that the per-lane arrays live in registers: no private
// segment up to KM = 16.  Above 16 the loops stay rolled (KM = TFHE_MAX_LIMBS; scratch is accepted there).
//
// Division by Δ without a divide instruction.  With k = bitlen(Δ), sh = k - 1 and R = min(floor(2^(63+k) / Δ), 2^64 - 1):
// for m < 2^63 Δ (every m used here: m <= Q - 1 < (t + t/Δ) Δ <= 2 t Δ with t < 2^62),
//     qh = mulhi(floor(m / 2^sh), R) + 1   satisfies   floor(m / Δ) - 1 <= qh <= floor(m / Δ) + 1
// (writing m / 2^sh = mh + f, 2^(63+k) / Δ = R + g with f in [0, 1), g in [0, 1]: m/Δ - mh R / 2^64 = (f R + g mh + f g) / 2^64
// < 2, and the floor of mh R / 2^64 loses less than 1, so m/Δ - (qh - 1) lies in [0, 3)).  The remainder m - qh Δ is formed
// exactly (multi-word multiply-subtract) and lies in [-Δ, 2Δ): one ±1 correction of the quotient finishes it.
#pragma once
#include "conv_core.h"

enum { PLAIN_HIT_DOWN = 0, PLAIN_HIT_UP = 1, PLAIN_HIT_TIE = 2, PLAIN_HIT_EXACT_ALPHA = 3, PLAIN_HIT_N = 4 };
#if defined(TFHE_EMUL_TRACK_RANGE) && !defined(__HIP_DEVICE_COMPILE__)
// CPU emulation only (tests/plain_emul): how often each rare branch ran (quotient corrected down / up, an exact tie, the
// exact-α decision of the lift)
#define TFHE_PLAIN_HIT(i) (g_plain_hits[(i)]++)
#else
#define TFHE_PLAIN_HIT(i) ((void)0)
#endif

// Device-resident table of one (ring basis, t) pair.  Word arrays are little-endian and zero past their length.
struct plain_tab_t {
    conv_tab_t cv;               // basis(ring) -> {t}: the exact lift, and the centred conversion to t (BGV π)
    int nq;                      // words of Q (= cv.nwords)
    int nd;                      // words of Δ
    u32 sh;                      // bitlen(Δ) - 1
    u64 R;                       // min(floor(2^(63 + bitlen Δ) / Δ), 2^64 - 1)
    u64 t;
    barrett_t bt;                // t
    u64 D[TFHE_MAX_LIMBS];       // Δ = Q ÷ t
    u64 Dh[TFHE_MAX_LIMBS];      // Δ ÷ 2          (birem: r <= Δ÷2 keeps r)
    u64 Dc[TFHE_MAX_LIMBS];      // Δ - Δ ÷ 2      (= ⌈Δ/2⌉; rounding: 2r >= Δ <=> r >= ⌈Δ/2⌉)
    u64 Qh[TFHE_MAX_LIMBS];      // Q ÷ 2          (centring: x > Q÷2 => x - Q)
    tw_t enc[2][TFHE_MAX_LIMBS]; // encode factor per limb: [0] BFV Δ mod q_l, [1] BGV 1
};

#define TFHE_PLAIN_UNROLL(KM) ((KM) <= 16 ? (KM) : 1)

// a <=> b over the low n words (n <= KM): -1, 0, 1
template <int KM>
TFHE_HD int plain_cmp(const u64 (&a)[KM], const u64* b, int n) {
    int c = 0;
#pragma unroll TFHE_PLAIN_UNROLL(KM)
    for (int i = KM - 1; i >= 0; i--)
        if (i < n && c == 0) c = a[i] > b[i] ? 1 : (a[i] < b[i] ? -1 : 0);
    return c;
}

// one column of X = Σ_j ξ_j (A/a_j): the 192-bit window (lo, hi, ex) accumulates word w of every product
template <int KM>
TFHE_HD void plain_column(const conv_tab_t& T, const u64 (&xi)[KM], int w, u64& acc_lo, u64& acc_hi, u64& acc_ex) {
#pragma unroll TFHE_PLAIN_UNROLL(KM)
    for (int j = 0; j < KM; j++) {
        if (j < T.k) {
            u64 lo, hi;
            mul64_full(xi[j], T.M[(size_t)j * T.nwords + w], lo, hi);
            u64 s = acc_lo + lo;
            const u64 c = (s < lo);
            acc_lo = s;
            s = acc_hi + hi;
            u64 c2 = (s < hi);
            s += c;
            c2 += (s < c);
            acc_hi = s;
            acc_ex += c2;
        }
    }
}

// conv_prepare (conv_core.h) unrolled: xi holds the residues on entry and ξ_j on exit; returns α.
template <int KM>
TFHE_HD u32 plain_prepare(const conv_tab_t& T, u64 (&xi)[KM], bool centred) {
    u64 frac = 0;
    u32 carries = 0;
#pragma unroll TFHE_PLAIN_UNROLL(KM)
    for (int j = 0; j < KM; j++) {
        if (j < T.k) {
            u64 x = xi[j];
            const u64 aj = T.a[j];
            if (centred) x = addmod(x, T.half[j], aj);
            const u64 xij = shoup_full(x, T.inv[j], aj);
            xi[j] = xij;
            const u64 xb = xij << T.sh[j];
            const u64 f = xb + mulhi64(xb, T.rho[j]);
            const u64 s = frac + f;
            carries += (s < f);
            frac = s;
        }
    }
    const u64 slack = 2ull * (u64)T.k;
    if (frac + slack >= frac) return carries;
    // exact decision (conv_prepare's slow path): X >= (carries + 1) A ?
    TFHE_PLAIN_HIT(PLAIN_HIT_EXACT_ALPHA);
    const u64 mult = (u64)carries + 1;
    u64 acc_lo = 0, acc_hi = 0, acc_ex = 0, mcarry = 0, borrow = 0;
#pragma unroll TFHE_PLAIN_UNROLL(KM)
    for (int w = 0; w <= KM; w++) {
        if (w <= T.nwords) {
            if (w < T.nwords) plain_column<KM>(T, xi, w, acc_lo, acc_hi, acc_ex);
            const u64 xw = acc_lo;
            acc_lo = acc_hi; acc_hi = acc_ex; acc_ex = 0;
            const u64 aw = w < T.nwords ? T.Aw[w] : 0;
            const u64 plo = aw * mult, phi = mulhi64(aw, mult);
            const u64 yw = plo + mcarry;
            mcarry = phi + (yw < plo);
            const u64 d = xw - yw;
            borrow = (u64)(xw < yw) | (u64)(d < borrow);
        }
    }
    return carries + (borrow ? 0u : 1u);
}

// conv_words (conv_core.h) unrolled: the plain lift X - α A in [0, A) as words (zero from T.nwords up)
template <int KM>
TFHE_HD void plain_words(const conv_tab_t& T, const u64 (&xi)[KM], u32 alpha, u64 (&out)[KM]) {
    u64 acc_lo = 0, acc_hi = 0, acc_ex = 0, mcarry = 0, borrow = 0;
#pragma unroll TFHE_PLAIN_UNROLL(KM)
    for (int w = 0; w < KM; w++) {
        if (w < T.nwords) {
            plain_column<KM>(T, xi, w, acc_lo, acc_hi, acc_ex);
            const u64 xw = acc_lo;
            acc_lo = acc_hi; acc_hi = acc_ex; acc_ex = 0;
            const u64 aw = T.Aw[w];
            const u64 plo = aw * (u64)alpha, phi = mulhi64(aw, (u64)alpha);
            const u64 yw = plo + mcarry;
            mcarry = phi + (yw < plo);
            const u64 d = xw - yw;
            out[w] = d - borrow;
            borrow = (u64)(xw < yw) | (u64)(d < borrow);
        } else {
            out[w] = 0;
        }
    }
}

// conv_eval (conv_core.h) unrolled, for the single target t (index 0)
template <int KM>
TFHE_HD u64 plain_eval_t(const conv_tab_t& T, const u64 (&xi)[KM], u32 alpha, bool centred) {
    const barrett_t& bt = T.t[0];
    const int cf = T.copy_from[0];
    u64 r;
    if (cf >= 0) {  // t is one of the ring's moduli
        u64 x = 0;
#pragma unroll TFHE_PLAIN_UNROLL(KM)
        for (int j = 0; j < KM; j++)
            if (j == cf) x = xi[j];
        r = mulmod(x, T.C[(size_t)cf * T.m], bt);
    } else {
        acc128 acc{0, 0};
        u64 sum = 0;
        int pending = 0;
#pragma unroll TFHE_PLAIN_UNROLL(KM)
        for (int j = 0; j < KM; j++) {
            if (j < T.k) {
                acc_mac(acc, xi[j], T.C[(size_t)j * T.m]);
                if (++pending == T.lazy) {
                    sum = addmod(sum, barrett_reduce128(acc.lo, acc.hi, bt), bt.q);
                    acc = acc128{0, 0};
                    pending = 0;
                }
            }
        }
        if (pending) sum = addmod(sum, barrett_reduce128(acc.lo, acc.hi, bt), bt.q);
        r = submod(sum, mulmod((u64)alpha, T.Amod[0], bt), bt.q);
    }
    if (centred) r = submod(r, T.halfT[0], bt.q);
    return r;
}

// the exact plain lift of the coefficient whose limb l is c[l * ls]
template <int KM>
TFHE_HD void plain_lift(const plain_tab_t& P, const u64* c, size_t ls, u64 (&x)[KM]) {
    u64 xi[KM];
#pragma unroll TFHE_PLAIN_UNROLL(KM)
    for (int j = 0; j < KM; j++) xi[j] = j < P.cv.k ? c[(size_t)j * ls] : 0;
    const u32 alpha = plain_prepare<KM>(P.cv, xi, false);
    plain_words<KM>(P.cv, xi, alpha, x);
}

// q = floor(m / Δ), r = m mod Δ (words of r from nd up are zero), for m < 2^63 Δ given as nq words
template <int KM>
TFHE_HD u64 plain_divmod_delta(const plain_tab_t& P, const u64 (&m)[KM], u64 (&r)[KM]) {
    const int ws = (int)(P.sh >> 6), bs = (int)(P.sh & 63);
    u64 lo = 0, hi = 0;
#pragma unroll TFHE_PLAIN_UNROLL(KM)
    for (int i = 0; i < KM; i++) {
        if (i == ws) lo = m[i];
        if (i == ws + 1) hi = m[i];
    }
    const u64 mh = bs ? (lo >> bs) | (hi << (64 - bs)) : lo;  // floor(m / 2^sh) < 2^64
    u64 q = mulhi64(mh, P.R) + 1;                              // floor(m / Δ) + {-1, 0, 1}
    // r = m - q Δ over nq words; the word above (0 for m) says whether it went negative
    u64 mcarry = 0, borrow = 0;
#pragma unroll TFHE_PLAIN_UNROLL(KM)
    for (int i = 0; i < KM; i++) {
        if (i < P.nq) {
            u64 plo, phi;
            mul64_full(P.D[i], q, plo, phi);
            const u64 yw = plo + mcarry;
            mcarry = phi + (yw < plo);
            const u64 d = m[i] - yw;
            r[i] = d - borrow;
            borrow = (u64)(m[i] < yw) | (u64)(d < borrow);
        } else {
            r[i] = 0;
        }
    }
    if (mcarry | borrow) {  // r in [-Δ, 0): one Δ back (the carry out of the top word cancels the negative sign)
        TFHE_PLAIN_HIT(PLAIN_HIT_DOWN);
        q--;
        u64 carry = 0;
#pragma unroll TFHE_PLAIN_UNROLL(KM)
        for (int i = 0; i < KM; i++) {
            if (i < P.nq) {
                const u64 s = r[i] + P.D[i];
                const u64 c1 = s < r[i];
                r[i] = s + carry;
                carry = c1 | (u64)(r[i] < carry);
            }
        }
    } else if (plain_cmp<KM>(r, P.D, P.nq) >= 0) {  // r in [Δ, 2Δ)
        TFHE_PLAIN_HIT(PLAIN_HIT_UP);
        q++;
        u64 br = 0;
#pragma unroll TFHE_PLAIN_UNROLL(KM)
        for (int i = 0; i < KM; i++) {
            if (i < P.nq) {
                const u64 d = r[i] - P.D[i];
                const u64 b1 = r[i] < P.D[i];
                const u64 e = d - br;
                br = b1 | (u64)(d < br);
                r[i] = e;
            }
        }
    }
    return q;
}

// BFV π of one coefficient (limb l at c[l * ls])
template <int KM>
TFHE_HD u64 plain_bfv_decode_coeff(const plain_tab_t& P, const u64* c, size_t ls) {
    u64 x[KM], r[KM];
    plain_lift<KM>(P, c, ls, x);
    // |centred(x)| as the magnitude m (x or Q - x; Q is odd, so |centred(x)| <= (Q-1)/2)
    const bool neg = plain_cmp<KM>(x, P.Qh, P.nq) > 0;
    if (neg) {
        u64 br = 0;
#pragma unroll TFHE_PLAIN_UNROLL(KM)
        for (int i = 0; i < KM; i++) {
            if (i < P.nq) {
                const u64 a = P.cv.Aw[i];
                const u64 d = a - x[i];
                const u64 b1 = a < x[i];
                x[i] = d - br;
                br = b1 | (u64)(d < br);
            }
        }
    }
    u64 q = plain_divmod_delta<KM>(P, x, r);
    // RoundNearestTiesAway on the magnitude: up when 2r >= Δ, i.e. r >= ⌈Δ/2⌉; 2r == Δ (Δ even) is the tie, rounded away
    const int cr = plain_cmp<KM>(r, P.Dc, P.nd);
    if (cr >= 0) {
        if (cr == 0 && (P.D[0] & 1) == 0) TFHE_PLAIN_HIT(PLAIN_HIT_TIE);
        q++;
    }
    // y = ±q.  The reference then wraps y through SignedMod(·, Q) (bfv.jl:26-29); that wrap is the identity because |y| < Q/2:
    // for Δ = 1, |y| = |centred(x)| <= (Q-1)/2; for Δ >= 2, |y| <= (Q-1)/(2Δ) + 1/2 <= (Q+1)/4 < Q/2 (Q >= 3).
    // And q <= t: (Q-1)/2 / Δ < t (Δ+1) / (2Δ) <= t since Q < t (Δ+1), so one conditional subtraction reduces it.
    const u64 ym = q >= P.t ? q - P.t : q;
    return (neg && ym) ? P.t - ym : ym;
}

// BGV π of one coefficient: centred(x) mod t, one exact centred conversion to t
template <int KM>
TFHE_HD u64 plain_bgv_decode_coeff(const plain_tab_t& P, const u64* c, size_t ls) {
    u64 xi[KM];
#pragma unroll TFHE_PLAIN_UNROLL(KM)
    for (int j = 0; j < KM; j++) xi[j] = j < P.cv.k ? c[(size_t)j * ls] : 0;
    const u32 alpha = plain_prepare<KM>(P.cv, xi, true);
    return plain_eval_t<KM>(P.cv, xi, alpha, true);
}

// the BFV noise remainder birem(x) of one coefficient, as words (zero from nd up)
template <int KM>
TFHE_HD void plain_noise_coeff(const plain_tab_t& P, const u64* c, size_t ls, u64 (&out)[KM]) {
    u64 x[KM];
    plain_lift<KM>(P, c, ls, x);
    plain_divmod_delta<KM>(P, x, out);
    if (plain_cmp<KM>(out, P.Dh, P.nd) > 0) {  // r > Δ÷2: Δ - r
        u64 br = 0;
#pragma unroll TFHE_PLAIN_UNROLL(KM)
        for (int i = 0; i < KM; i++) {
            if (i < P.nd) {
                const u64 d = P.D[i] - out[i];
                const u64 b1 = P.D[i] < out[i];
                out[i] = d - br;
                br = b1 | (u64)(d < br);
            }
        }
    }
}

// π⁻¹ of one coefficient m (any u64; negative plaintexts arrive reduced mod t): limb l gets (m mod t) f_l mod q_l
TFHE_HD void plain_encode_coeff(const plain_tab_t& P, int bgv, u64 m, u64* dst, size_t ls) {
    const u64 mt = barrett_reduce128(m, 0, P.bt);  // m < 2^64 <= 2^(bitlen(t) + 62): inside the Barrett window
    const tw_t* f = P.enc[bgv ? 1 : 0];
    for (int l = 0; l < P.cv.k; l++) dst[(size_t)l * ls] = shoup_full(mt, f[l], P.cv.a[l]);
}
