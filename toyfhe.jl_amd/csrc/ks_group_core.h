// ks_group_core.h -- the kernels of the key switch with grouped RNS digits and several special primes (tfhe_keyswitch_grouped and the
// hoisted rotations, ks_api.inc; the tail that carries the rescale of tfhe_mul_relin_grouped, mul_api.inc; the permutation and the lift of
// the evaluation-domain rotation phase of tfhe_matmul_diag_grouped / tfhe_matmul_bsgs_grouped and the gather and the finish of a fold step
// of tfhe_rotate_sum_grouped / tfhe_matmul_bsgs_fold_grouped, md_api.inc), and their per-coefficient bodies.
//
// Digit g of c[end] is the centred representative of c[end] modulo Q_g = prod_{i in G_g} q_i (the exact CRT value with the tie
// rule of signedmod.jl:12-19, n > Q_g ÷ 2 => n - Q_g; switch(ℛ_W, .) of bfv.jl:202-226 on the sub-ring of the group; with one limb
// per group the digit of rlwe_she.jl:326-329), reduced into every working limb W = [0 .. level-1] ∪ [the k special primes].  The
// key sums over W are contracted by modswitch (crt.jl:215-228, unsigned c_last) once per special prime, the last one first.
// The bodies are TFHE_HD: tests/ks_group_emul, tests/ks_group_rot_emul, tests/mdg_lift_emul and tests/mdg_fold_emul run them on the host.
#pragma once
#include <cstdio>

#include "../../include/toyfhe_hip.h"
#include "conv_core.h"

#define TFHE_KSG_MAX_SPECIAL 4

// The host checks of tfhe_keyswitch_grouped / tfhe_rotate_grouped in the order include/toyfhe_hip.h states, on plain numbers (L, N:
// the context's ring; any_null: a null argument, the context among them), so that tests/ks_group_emul runs them without a device.
// Returns TFHE_OK, or the status with its message in `msg`.
inline int ks_group_check(bool any_null, int L, int64_t N, int Lk, int level, int k, int group, int n_digits, int polys, int64_t batch, bool rotate,
                          uint64_t galois, char* msg, size_t cap) {
    msg[0] = 0;
    if (any_null) return snprintf(msg, cap, "null argument"), TFHE_E_BADARG;
    if (polys != 2 && polys != 3) return snprintf(msg, cap, "keyswitch needs a 2- or 3-element ciphertext (rlwe_she.jl:318), got %d", polys), TFHE_E_BADARG;
    if (Lk < 1 || Lk > L) return snprintf(msg, cap, "key_limbs=%d outside [1,%d]", Lk, L), TFHE_E_BADARG;
    const int kmax = TFHE_KSG_MAX_SPECIAL < Lk - 1 ? TFHE_KSG_MAX_SPECIAL : Lk - 1;
    if (k < 0 || k > kmax) return snprintf(msg, cap, "n_special=%d outside [0,%d]", k, kmax), TFHE_E_BADARG;
    if (group < 1) return snprintf(msg, cap, "group=%d: a digit takes at least one limb", group), TFHE_E_BADARG;
    if (level < 1 || level > Lk - k) return snprintf(msg, cap, "level=%d outside [1,%d]", level, Lk - k), TFHE_E_LEVEL_MISMATCH;
    const int d = (int)(((int64_t)level + group - 1) / group);
    if (n_digits < d)
        return snprintf(msg, cap, "evaluation key has %d components, level %d in groups of %d needs %d", n_digits, level, group, d), TFHE_E_PARAMS_MISMATCH;
    if (level + k > TFHE_MAX_LIMBS) return snprintf(msg, cap, "%d working limbs, at most %d are supported", level + k, TFHE_MAX_LIMBS), TFHE_E_UNSUPPORTED;
    if (batch < 0) return snprintf(msg, cap, "negative batch"), TFHE_E_BADARG;
    if (rotate && ((galois & 1) == 0 || galois >= 2 * (uint64_t)N)) return snprintf(msg, cap, "galois element must be odd and below 2N"), TFHE_E_BADARG;
    return TFHE_OK;
}

// The host checks of tfhe_rotate_many_grouped (product = false) / tfhe_matmul_diag_grouped in the order include/toyfhe_hip.h states, on
// plain numbers: any_null -- a null context, evks, galois_elements, ct, out (or diags); evks / galois -- the caller's HOST arrays, of
// which only evks[r] == nullptr and galois[r] are looked at; ct / out / diags -- the operands' addresses, compared and never followed.
// *nothing_to_do comes back true where the call returns TFHE_OK without work (no rotations to hoist, an empty batch).
inline int ks_group_many_check(bool product, bool any_null, int L, int64_t N, int Lk, int level, int k, int group, int n_digits, int64_t batch,
                               const uint64_t* const* evks, const uint64_t* galois, int n_rot, uintptr_t ct, uintptr_t out, uintptr_t diags,
                               bool* nothing_to_do, char* msg, size_t cap, int max_rot = 64) {
    msg[0] = 0;
    *nothing_to_do = false;
    if (any_null || n_rot < 0) return snprintf(msg, cap, "null argument"), TFHE_E_BADARG;
    if (product && n_rot > max_rot)
        return snprintf(msg, cap, "tfhe_matmul_diag_grouped takes at most %d rotations per call", max_rot), TFHE_E_UNSUPPORTED;
    if (!product && n_rot == 0) return *nothing_to_do = true, TFHE_OK;
    for (int r = 0; r < n_rot; r++) {
        const int rc = ks_group_check(evks[r] == nullptr, L, N, Lk, level, k, group, n_digits, 2, batch, true, galois[r], msg, cap);
        if (rc) return rc;
    }
    if (n_rot == 0) {
        const int rc = ks_group_check(false, L, N, Lk, level, k, group, n_digits, 2, batch, false, 0, msg, cap);
        if (rc) return rc;
    }
    // the tail scatters into `out` while other workgroups still read `ct`; the accumulation reads `diags` while it writes
    const uint64_t ct_bytes = (uint64_t)batch * 2 * level * (uint64_t)N * 8;
    const uint64_t out_bytes = product ? ct_bytes : ct_bytes * (uint64_t)n_rot;
    const auto overlap = [](uintptr_t a, uint64_t na, uintptr_t b, uint64_t nb) { return a < b + nb && b < a + na; };
    if (overlap(out, out_bytes, ct, ct_bytes) || (product && overlap(out, out_bytes, diags, (uint64_t)(n_rot + 1) * level * (uint64_t)N * 8)))
        return snprintf(msg, cap, "out overlaps an operand"), TFHE_E_BADARG;
    *nothing_to_do = batch == 0;
    return TFHE_OK;
}

// The host checks of tfhe_matmul_bsgs_grouped in the order include/toyfhe_hip.h states, on plain numbers: any_null -- a null context, key
// or Galois array, diags, cts or out; the HOST arrays are read no further than a valid count reaches; bias / out -- addresses, compared
// and never followed (bias may be 0).  *nothing_to_do comes back true where the call returns TFHE_OK without work (an empty batch).
inline int ks_group_bsgs_check(bool any_null, int L, int64_t N, int Lk, int level, int k, int group, int n_digits, int64_t batch,
                               const uint64_t* const* baby_evks, const uint64_t* baby_galois, int n_baby, const uint64_t* const* giant_evks,
                               const uint64_t* giant_galois, int n_giant, const uint64_t* const* diags, const uint64_t* const* cts, int n_in,
                               uintptr_t bias, uintptr_t out, bool* nothing_to_do, char* msg, size_t cap, int max_n = 64) {
    msg[0] = 0;
    *nothing_to_do = false;
    if (any_null) return snprintf(msg, cap, "null argument"), TFHE_E_BADARG;
    const auto within = [max_n](int n) { return n < 0 ? 0 : (n > max_n ? max_n : n); };
    for (int r = 0; r < within(n_baby); r++)
        if (!baby_evks[r]) return snprintf(msg, cap, "null baby key %d", r), TFHE_E_BADARG;
    for (int r = 0; r < within(n_giant); r++)
        if (!giant_evks[r]) return snprintf(msg, cap, "null giant key %d", r), TFHE_E_BADARG;
    for (int m = 0; m < within(n_in); m++) {
        if (!diags[m]) return snprintf(msg, cap, "null diagonals of input %d", m), TFHE_E_BADARG;
        if (!cts[m]) return snprintf(msg, cap, "null ciphertext of input %d", m), TFHE_E_BADARG;
    }
    if (n_baby < 0 || n_baby > max_n) return snprintf(msg, cap, "n_baby=%d outside [0,%d]", n_baby, max_n), TFHE_E_BADARG;
    if (n_giant < 0 || n_giant > max_n) return snprintf(msg, cap, "n_giant=%d outside [0,%d]", n_giant, max_n), TFHE_E_BADARG;
    if (n_in < 1 || n_in > max_n) return snprintf(msg, cap, "n_in=%d outside [1,%d]", n_in, max_n), TFHE_E_BADARG;
    for (int r = 0; r < n_baby + n_giant; r++) {
        const uint64_t g = r < n_baby ? baby_galois[r] : giant_galois[r - n_baby];
        const int rc = ks_group_check(false, L, N, Lk, level, k, group, n_digits, 2, batch, true, g, msg, cap);
        if (rc) return rc;
    }
    if (n_baby + n_giant == 0) {
        const int rc = ks_group_check(false, L, N, Lk, level, k, group, n_digits, 2, batch, false, 0, msg, cap);
        if (rc) return rc;
    }
    // the closing sum writes `out` while other workgroups still read the operands of the next chunk
    const uint64_t ct_bytes = (uint64_t)batch * 2 * level * (uint64_t)N * 8;
    const uint64_t diag_bytes = (uint64_t)(n_giant + 1) * (n_baby + 1) * level * (uint64_t)N * 8;
    const auto overlap = [](uintptr_t a, uint64_t na, uintptr_t b, uint64_t nb) { return a == b || (a < b + nb && b < a + na); };
    bool hit = bias && overlap(out, ct_bytes, bias, (uint64_t)level * (uint64_t)N * 8);
    for (int m = 0; m < n_in && !hit; m++)
        hit = overlap(out, ct_bytes, (uintptr_t)cts[m], ct_bytes) || overlap(out, ct_bytes, (uintptr_t)diags[m], diag_bytes);
    if (hit) return snprintf(msg, cap, "out overlaps an operand"), TFHE_E_BADARG;
    *nothing_to_do = batch == 0;
    return TFHE_OK;
}

// The host checks of tfhe_rotate_sum_grouped (product = false: no baby or giant key, diags unused, cts = the one input, n_in = 1) and
// tfhe_matmul_bsgs_fold_grouped in the order include/toyfhe_hip.h states, on plain numbers: any_null -- a null context or array; the
// HOST arrays are read no further than a valid count reaches; fold_evks / fold_galois: all fold steps back to back, fold_sizes
// [n_fold_steps]; bias / out -- addresses, compared and never followed (bias may be 0).  The fold's rules and messages are fold_check_host's
// (md_api.inc).  *nothing_to_do comes back true where the call returns TFHE_OK without work (an empty batch).
inline int ks_group_fold_check(bool product, bool any_null, int L, int64_t N, int Lk, int level, int k, int group, int n_digits, int64_t batch,
                               const uint64_t* const* baby_evks, const uint64_t* baby_galois, int n_baby, const uint64_t* const* giant_evks,
                               const uint64_t* giant_galois, int n_giant, const uint64_t* const* diags, const uint64_t* const* cts, int n_in,
                               const uint64_t* const* fold_evks, const uint64_t* fold_galois, const int* fold_sizes, int n_fold_steps, uintptr_t bias,
                               uintptr_t out, bool* nothing_to_do, char* msg, size_t cap, int max_n = 64) {
    msg[0] = 0;
    *nothing_to_do = false;
    if (any_null) return snprintf(msg, cap, "null argument"), TFHE_E_BADARG;
    if (n_fold_steps < 0 || n_fold_steps > max_n) return snprintf(msg, cap, "n_fold_groups=%d outside [0,%d]", n_fold_steps, max_n), TFHE_E_BADARG;
    int n_fold = 0;
    for (int t = 0; t < n_fold_steps; t++) {
        if (fold_sizes[t] < 1) return snprintf(msg, cap, "fold group %d has size %d, below 1", t, fold_sizes[t]), TFHE_E_BADARG;
        if (fold_sizes[t] > max_n || (n_fold += fold_sizes[t]) > max_n) return snprintf(msg, cap, "more than %d fold keys", max_n), TFHE_E_BADARG;
    }
    for (int r = 0; r < n_fold; r++)
        if (!fold_evks[r]) return snprintf(msg, cap, "null fold key %d", r), TFHE_E_BADARG;
    if (product) {
        const auto within = [max_n](int n) { return n < 0 ? 0 : (n > max_n ? max_n : n); };
        for (int r = 0; r < within(n_baby); r++)
            if (!baby_evks[r]) return snprintf(msg, cap, "null baby key %d", r), TFHE_E_BADARG;
        for (int r = 0; r < within(n_giant); r++)
            if (!giant_evks[r]) return snprintf(msg, cap, "null giant key %d", r), TFHE_E_BADARG;
        for (int m = 0; m < within(n_in); m++) {
            if (!diags[m]) return snprintf(msg, cap, "null diagonals of input %d", m), TFHE_E_BADARG;
            if (!cts[m]) return snprintf(msg, cap, "null ciphertext of input %d", m), TFHE_E_BADARG;
        }
        if (n_baby < 0 || n_baby > max_n) return snprintf(msg, cap, "n_baby=%d outside [0,%d]", n_baby, max_n), TFHE_E_BADARG;
        if (n_giant < 0 || n_giant > max_n) return snprintf(msg, cap, "n_giant=%d outside [0,%d]", n_giant, max_n), TFHE_E_BADARG;
        if (n_in < 1 || n_in > max_n) return snprintf(msg, cap, "n_in=%d outside [1,%d]", n_in, max_n), TFHE_E_BADARG;
    } else {
        n_baby = n_giant = 0;
        n_in = 1;
    }
    for (int r = 0; r < n_baby + n_giant + n_fold; r++) {
        const uint64_t g = r < n_baby ? baby_galois[r] : (r < n_baby + n_giant ? giant_galois[r - n_baby] : fold_galois[r - n_baby - n_giant]);
        const int rc = ks_group_check(false, L, N, Lk, level, k, group, n_digits, 2, batch, true, g, msg, cap);
        if (rc) return rc;
    }
    if (n_baby + n_giant + n_fold == 0) {
        const int rc = ks_group_check(false, L, N, Lk, level, k, group, n_digits, 2, batch, false, 0, msg, cap);
        if (rc) return rc;
    }
    // the last step writes `out` while other workgroups still read the operands (of the next chunk)
    const uint64_t ct_bytes = (uint64_t)batch * 2 * level * (uint64_t)N * 8;
    const uint64_t diag_bytes = (uint64_t)(n_giant + 1) * (n_baby + 1) * level * (uint64_t)N * 8;
    const auto overlap = [](uintptr_t a, uint64_t na, uintptr_t b, uint64_t nb) { return a == b || (a < b + nb && b < a + na); };
    bool hit = bias && overlap(out, ct_bytes, bias, (uint64_t)level * (uint64_t)N * 8);
    for (int m = 0; m < n_in && !hit; m++)
        hit = overlap(out, ct_bytes, (uintptr_t)cts[m], ct_bytes) || (product && overlap(out, ct_bytes, (uintptr_t)diags[m], diag_bytes));
    if (hit) return snprintf(msg, cap, "out overlaps an operand"), TFHE_E_BADARG;
    *nothing_to_do = batch == 0;
    return TFHE_OK;
}

// The host checks of tfhe_mul_relin_grouped in the order include/toyfhe_hip.h states, on plain numbers: any_null -- a null context,
// evk, c1, c2 or out; logN -- log2 of the ring degree; c1 / c2 / out -- the operands' addresses, compared and never followed.
// *nothing_to_do comes back true where the call returns TFHE_OK without work (an empty batch).
inline int ks_group_mul_check(bool any_null, int L, int64_t N, int logN, int Lk, int level, int k, int group, int n_digits, int64_t batch, int ntt_in,
                              int rescale, uintptr_t c1, uintptr_t c2, uintptr_t out, bool* nothing_to_do, char* msg, size_t cap) {
    msg[0] = 0;
    *nothing_to_do = false;
    if (any_null) return snprintf(msg, cap, "null argument"), TFHE_E_BADARG;
    if (batch < 0) return snprintf(msg, cap, "negative batch"), TFHE_E_BADARG;
    if ((ntt_in != 0 && ntt_in != 1) || (rescale != 0 && rescale != 1)) return snprintf(msg, cap, "ntt_in and rescale are 0 or 1"), TFHE_E_BADARG;
    if (rescale && level < 2) return snprintf(msg, cap, "modswitch after the product needs level >= 2, got %d", level), TFHE_E_LEVEL_MISMATCH;
    if (out == c1 || out == c2) return snprintf(msg, cap, "out overlaps an operand"), TFHE_E_BADARG;
    const int rc = ks_group_check(false, L, N, Lk, level, k, group, n_digits, 3, batch, false, 0, msg, cap);
    if (rc) return rc;
    const uint64_t in_bytes = (uint64_t)batch * 2 * level * (uint64_t)N * 8, out_bytes = (uint64_t)batch * 2 * (level - rescale) * (uint64_t)N * 8;
    const auto overlap = [](uintptr_t a, uint64_t na, uintptr_t b, uint64_t nb) { return a < b + nb && b < a + na; };
    if (overlap(out, out_bytes, c1, in_bytes) || overlap(out, out_bytes, c2, in_bytes)) return snprintf(msg, cap, "out overlaps an operand"), TFHE_E_BADARG;
    if (batch == 0) return *nothing_to_do = true, TFHE_OK;
    // the transforms count rows in 31 bits (tfhe_mul_relin's bound)
    if ((batch * 4 * level) << (logN > 14 ? logN - 14 : 0) > 0x7fffffffll) return snprintf(msg, cap, "bad batch"), TFHE_E_BADARG;
    return TFHE_OK;
}

// ---- digits: conv_prepare (centred) over the group's residues, conv_eval into each working limb ------------------------------
// G: the residues a thread holds, at least the group's size T.k (a group cut short by the level has fewer); G = 0: any size
template <int G>
struct ks_group_digit_t {
    u64 xi[G ? G : TFHE_MAX_LIMBS];   // the group's residues of one coefficient on entry, conv_prepare's xi afterwards
    u32 alpha;
};
template <int G>
TFHE_HD void ks_group_prepare(const conv_tab_t& T, ks_group_digit_t<G>& D) { D.alpha = conv_prepare_n<G>(T, D.xi, 1, true); }
// the digit modulo working limb i (a limb of the group itself: the residue back, conv_eval's copy path)
template <int G>
TFHE_HD u64 ks_group_eval(const conv_tab_t& T, const ks_group_digit_t<G>& D, int i) { return conv_eval_n<G>(T, D.xi, 1, i, D.alpha, true); }

// ---- tail: K modswitch steps, the last special prime first -------------------------------------------------------------------
// inv[t][j] = p_t^-1 mod (working limb j), p_t the t-th special prime (working limb level + t); only j < level + t is read.
// The steps on the special limbs themselves are triangular: step t takes y[t] as it stands -- the unsigned "last" of that step --
// out of every y[u], u < t.  On return y[t] is the "last" of step t.
template <int K>
TFHE_HD void ks_group_tail_special(u64 (&y)[K], const barrett_t* pb, const tw_t (*inv)[TFHE_MAX_LIMBS], int level) {
#pragma unroll
    for (int t = K - 1; t >= 1; t--)
#pragma unroll
        for (int u = 0; u < t; u++)
            y[u] = shoup_full(submod(y[u], barrett_reduce128(y[t], 0, pb[u]), pb[u].q), inv[t][level + u], pb[u].q);
}
// one ciphertext limb j through the K updates (x - last) p_t^-1;  K = 1: the words of k_ks_rescale_add
template <int K>
TFHE_HD u64 ks_group_tail_limb(u64 x, const u64 (&last)[K], const barrett_t& bj, const tw_t (*inv)[TFHE_MAX_LIMBS], int j) {
#pragma unroll
    for (int t = K - 1; t >= 0; t--) x = shoup_full(submod(x, barrett_reduce128(last[t], 0, bj), bj.q), inv[t][j], bj.q);
    return x;
}

// ---- tail with a rescale riding on it (tfhe_mul_relin_grouped): the modswitch that follows the key switch is one more step of the
// same form, (x - [last]_{q_j}) q_last^-1 mod q_j with the unsigned last (k_rescale), last = word level - 1 of the key switch's result
struct ks_group_rescale_t {
    tw_t qlinv[TFHE_MAX_LIMBS];   // q_{level-1}^-1 mod q_j, j < level - 1
};
// the rescale's `last`: ciphertext limb level - 1 through the K steps, plus its addend
template <int K>
TFHE_HD u64 ks_group_tail_last(u64 x, u64 addend, const u64 (&y)[K], const barrett_t& bl, const tw_t (*inv)[TFHE_MAX_LIMBS], int level) {
    return addmod(ks_group_tail_limb<K>(x, y, bl, inv, level - 1), addend, bl.q);
}
// ciphertext limb j < level - 1: the K steps, the addend, then the (K+1)-th step against `last`
template <int K>
TFHE_HD u64 ks_group_tail_rescale_limb(u64 x, u64 addend, const u64 (&y)[K], u64 last, const barrett_t& bj, const tw_t (*inv)[TFHE_MAX_LIMBS],
                                       const tw_t& qlinv, int j) {
    x = addmod(ks_group_tail_limb<K>(x, y, bj, inv, j), addend, bj.q);
    return shoup_full(submod(x, barrett_reduce128(last, 0, bj), bj.q), qlinv, bj.q);
}

// ---- tail of a hoisted rotation: the signed permutation sigma_g BEFORE the K steps (the floor does not commute with sign changes) ----
// One coefficient i of one row group (rotation, ciphertext, component): t -> coefficient i of limb 0 of T = INTT(S') (nw rows of n
// words), c -> coefficient i of limb 0 of the addend c_0 (component 0) or nullptr, o -> limb 0 of the output rows; the coefficient
// goes to position m = g i mod n, negated (neg) where floor(g i / n) is odd.  lb: the nw working limbs' Barrett words, the special
// primes last.  The K special words first, the ciphertext limbs stream through: K + 2 words live per coefficient.
template <int K>
TFHE_HD void ks_group_rot_tail_coeff(const u64* t, const u64* c, u64* o, size_t n, u32 m, bool neg, int level, const barrett_t* lb,
                                     const tw_t (*inv)[TFHE_MAX_LIMBS]) {
    u64 y[K ? K : 1];
    if constexpr (K > 0) {
#pragma unroll
        for (int u = 0; u < K; u++) {
            const u64 v = t[(size_t)(level + u) * n];
            y[u] = neg ? negmod(v, lb[level + u].q) : v;
        }
        ks_group_tail_special<K>(y, lb + level, inv, level);
    }
    for (int j = 0; j < level; j++) {
        const barrett_t bj = lb[j];
        u64 x = t[(size_t)j * n];
        if (neg) x = negmod(x, bj.q);
        if constexpr (K > 0) x = ks_group_tail_limb<K>(x, y, bj, inv, j);
        if (c) {
            const u64 a = c[(size_t)j * n];
            x = addmod(x, neg ? negmod(a, bj.q) : a, bj.q);
        }
        o[(size_t)j * n + m] = x;
    }
}

// ---- the lift of the evaluation-domain rotation phase (mdg_rotations, md_api.inc) ----------------------------------------------------
// ks_group_tail_limb is affine in x: tail_j(x) = x Pinv_j + tail_j(0), Pinv_j = prod_t inv[t][j].  In the evaluation domain the key
// sums of a hoisted rotation keep the first term (V = S' Pinv_j, the key-sum kernels' epilogue) and only the second needs the
// coefficient domain -- it depends on the K special words alone:  U_j = -tail_j(0) = negmod(ks_group_tail_limb<K>(0, y)), with y the
// "lasts" ks_group_tail_special<K> leaves from the special words of sigma_g(INTT(S')).  The rotated ciphertext is V o pi_g - NTT_j(U_j).
template <int K>
TFHE_HD u64 mdg_lift_limb(const u64 (&y)[K], const barrett_t& bj, const tw_t (*inv)[TFHE_MAX_LIMBS], int j) {
    return negmod(ks_group_tail_limb<K>(0, y, bj, inv, j), bj.q);
}
// One coefficient of one row group: p -> the coefficient in special row 0 (K rows of n words), u -> the same coefficient in row 0 of
// the group's `level` output rows.  lb: the nw working limbs' Barrett words, the special primes last.
template <int K>
TFHE_HD void mdg_lift_coeff(const u64* p, u64* u, size_t n, int level, const barrett_t* lb, const tw_t (*inv)[TFHE_MAX_LIMBS]) {
    u64 y[K];
#pragma unroll
    for (int t = 0; t < K; t++) y[t] = p[(size_t)t * n];
    ks_group_tail_special<K>(y, lb + level, inv, level);
    for (int j = 0; j < level; j++) u[(size_t)j * n] = mdg_lift_limb<K>(y, lb[j], inv, j);
}

// ---- one fold step in the evaluation domain (mdg_fold_run, md_api.inc) ---------------------------------------------------------------
// In a fold step every rotation has the coefficient 1 and the step ends in an inverse transform, so the lifts never enter the
// evaluation domain:   F + sum_r rotate_grouped(gk_r, F) = INTT( X + sum_r V_r o pi_r ) - sum_r mdg_lift_limb(y_r),   X = NTT(F).
// The gather adds one permuted key-sum word to the running sum of a position (k_mdg_fold_gather); the finish takes, per coefficient
// and rotation, the K special words through the triangular steps and the lift of every limb of a block off the block's words.
// One rotation's share of one coefficient: y -- its K special words (the "lasts" on return), acc -- the words of limbs j0 .. j0 + nj - 1
// (nj <= JB), which lose the limb's lift.  lb: the nw working limbs' Barrett words, the special primes last.
template <int K, int JB>
TFHE_HD void mdg_fold_finish_coeff(u64 (&acc)[JB], u64 (&y)[K], int j0, int nj, int level, const barrett_t* lb, const tw_t (*inv)[TFHE_MAX_LIMBS]) {
    ks_group_tail_special<K>(y, lb + level, inv, level);
#pragma unroll
    for (int r = 0; r < JB; r++)
        if (r < nj) acc[r] = submod(acc[r], mdg_lift_limb<K>(y, lb[j0 + r], inv, j0 + r), lb[j0 + r].q);
}
#ifndef TFHE_MDG_FOLD_JB
#define TFHE_MDG_FOLD_JB 6   // limbs of a block: level 6 is one block; 2 JB accumulator and 2 K special words live at V = 2 (8: scratch at K = 4)
#endif

#if defined(__HIPCC__)
struct ks_group_arg_t {
    int level, nw, k, polys;   // ciphertext limbs, working limbs (level + k), special primes, elements of the input ciphertext
    int group, d;              // limbs per digit, digits = ceil(level / group)
    limb_sel_t w;              // the working limbs
    tw_t inv[TFHE_KSG_MAX_SPECIAL][TFHE_MAX_LIMBS];
};

// dig [batch][d][nw][N] from c[end] of ct [batch][polys][level][N]; tabs: one conv_tab_t per group (source: the group cut at this
// level, targets: W).  A thread takes V coefficients (V = 2: 16-byte loads and stores, as k_rescale_cm) of one (ciphertext, group):
// it reads the group's rows once and writes nw rows -- the kernel is bound by its stores, `level` rows in and d nw rows out per
// ciphertext.  grid: batch * d * gx workgroups, gx = ceil(N / (256 V)).
template <int G, int V>
__global__ __launch_bounds__(256) void k_ks_group_digits(const u64* __restrict__ ct, u64* __restrict__ dig,
                                                          const conv_tab_t* __restrict__ tabs, ks_group_arg_t A, u32 n, u32 gx) {
    const u32 i = ((blockIdx.x % gx) * 256 + threadIdx.x) * (u32)V;
    const u32 g = (blockIdx.x / gx) % (u32)A.d;
    const size_t b = blockIdx.x / (gx * (u32)A.d);
    if (i >= n) return;
    const conv_tab_t& T = tabs[g];
    const u64* src = ct + ((b * A.polys + A.polys - 1) * A.level + (size_t)g * A.group) * n + i;
    u64* dst = dig + ((b * A.d + g) * A.nw) * n + i;
    ks_group_digit_t<G> D[V];
    constexpr int GG = G ? G : TFHE_MAX_LIMBS;
    if constexpr (G != 0) {
#pragma unroll
        for (int j = 0; j < GG; j++) {
            const int jj = j < T.k ? j : T.k - 1;   // a group cut short: the spare registers repeat its last limb, unused
            if constexpr (V == 2) {
                const u64x2_t x = *(const u64x2_t*)(src + (size_t)jj * n);
                D[0].xi[j] = x.x; D[1].xi[j] = x.y;
            } else {
                D[0].xi[j] = src[(size_t)jj * n];
            }
        }
    } else {
        for (int j = 0; j < T.k; j++) {
            if constexpr (V == 2) {
                const u64x2_t x = *(const u64x2_t*)(src + (size_t)j * n);
                D[0].xi[j] = x.x; D[1].xi[j] = x.y;
            } else {
                D[0].xi[j] = src[(size_t)j * n];
            }
        }
    }
#pragma unroll
    for (int v = 0; v < V; v++) ks_group_prepare<G>(T, D[v]);
    for (int j = 0; j < A.nw; j++) {
        if constexpr (V == 2) {
            u64x2_t o;
            o.x = ks_group_eval<G>(T, D[0], j);
            o.y = ks_group_eval<G>(T, D[1], j);
            *(u64x2_t*)(dst + (size_t)j * n) = o;
        } else {
            dst[(size_t)j * n] = ks_group_eval<G>(T, D[0], j);
        }
    }
}

// out [batch][2][level][N] from T = INTT(S) [batch][2][nw][N]:  out_s = c_s + the K-step contraction of T_s (c_s for s < add_s).
// A thread takes V coefficients of one (ciphertext, component): the K special words first -- the triangular steps stay in
// registers and leave the unsigned "last" of every step -- then the ciphertext limbs stream through one at a time, so no thread
// holds nw words.  2 nw (+ the addends) rows in, 2 level rows out per ciphertext.  grid: batch * 2 * gx workgroups.
template <int K, int V>
__global__ __launch_bounds__(256) void k_ks_group_tail(const u64* __restrict__ T, const u64* __restrict__ ct, u64* __restrict__ out,
                                                        const ntt_limb_t* __restrict__ LT, ks_group_arg_t A, u32 n, u32 gx, u32 add_s) {
    const u32 i = ((blockIdx.x % gx) * 256 + threadIdx.x) * (u32)V;
    const u32 s = (blockIdx.x / gx) & 1u;
    const size_t b = blockIdx.x / (gx * 2u);
    if (i >= n) return;
    const u64* t = T + ((b * 2 + s) * A.nw) * n + i;
    const u64* c = s < add_s ? ct + ((b * A.polys + s) * A.level) * n + i : nullptr;
    u64* o = out + ((b * 2 + s) * A.level) * n + i;
    barrett_t pb[K];
    u64 y[V][K];
#pragma unroll
    for (int u = 0; u < K; u++) {
        pb[u] = LT[A.w.idx[A.level + u]].br;
        if constexpr (V == 2) {
            const u64x2_t x = *(const u64x2_t*)(t + (size_t)(A.level + u) * n);
            y[0][u] = x.x; y[1][u] = x.y;
        } else {
            y[0][u] = t[(size_t)(A.level + u) * n];
        }
    }
#pragma unroll
    for (int v = 0; v < V; v++) ks_group_tail_special<K>(y[v], pb, A.inv, A.level);
    for (int j = 0; j < A.level; j++) {
        const barrett_t bj = LT[A.w.idx[j]].br;
        if constexpr (V == 2) {
            const u64x2_t x = *(const u64x2_t*)(t + (size_t)j * n);
            u64x2_t r;
            r.x = ks_group_tail_limb<K>(x.x, y[0], bj, A.inv, j);
            r.y = ks_group_tail_limb<K>(x.y, y[1], bj, A.inv, j);
            if (c) {
                const u64x2_t cc = *(const u64x2_t*)(c + (size_t)j * n);
                r.x = addmod(r.x, cc.x, bj.q);
                r.y = addmod(r.y, cc.y, bj.q);
            }
            *(u64x2_t*)(o + (size_t)j * n) = r;
        } else {
            u64 r = ks_group_tail_limb<K>(t[(size_t)j * n], y[0], bj, A.inv, j);
            if (c) r = addmod(r, c[(size_t)j * n], bj.q);
            o[(size_t)j * n] = r;
        }
    }
}

// k_ks_group_tail with the modswitch of BOTH components riding on it (tfhe_mul_relin_grouped, rescale = 1; a 3-element input: both
// components carry addends): out [batch][2][level - 1][N] = tfhe_rescale of what k_ks_group_tail would have written, straight into
// the caller's array.  A thread takes V coefficients of one (ciphertext, component): the K special words, the triangular steps in
// registers; then limb level - 1 through the K steps plus its addend -- the rescale's unsigned `last`; then the limbs j < level - 1
// stream through: K steps, the addend, the (K+1)-th step with R.qlinv[j], the store.  No thread holds nw words.  The limbs go in
// blocks of JB: the 2 JB rows of a block (T and the addend) are requested before the first is used, as in k_rescale_cm -- one limb
// at a time the loop runs at the latency of its loads.  2 nw + 2 level rows in and 2 (level - 1) rows out per ciphertext: against
// k_ks_group_tail -> k_rescale_cm, 2 level rows written and 2 level rows read are gone.  grid: batch * 2 * gx workgroups.
template <int K, int V>
__global__ __launch_bounds__(256) void k_ks_group_tail_rescale(const u64* __restrict__ T, const u64* __restrict__ ct, u64* __restrict__ out,
                                                                const ntt_limb_t* __restrict__ LT, ks_group_arg_t A, ks_group_rescale_t R, u32 n,
                                                                u32 gx) {
    const u32 i = ((blockIdx.x % gx) * 256 + threadIdx.x) * (u32)V;
    const u32 s = (blockIdx.x / gx) & 1u;
    const size_t b = blockIdx.x / (gx * 2u);
    if (i >= n) return;
    const int jl = A.level - 1;   // the limb the rescale drops
    const u64* t = T + ((b * 2 + s) * A.nw) * n + i;
    const u64* c = ct + ((b * A.polys + s) * A.level) * n + i;
    u64* o = out + ((b * 2 + s) * jl) * n + i;
    struct word_t { u64 v[V]; };
    const auto ld = [](const u64* p) {
        word_t w;
        if constexpr (V == 2) {
            const u64x2_t x = *(const u64x2_t*)p;
            w.v[0] = x.x; w.v[1] = x.y;
        } else {
            w.v[0] = *p;
        }
        return w;
    };
    barrett_t pb[K];
    u64 y[V][K];
#pragma unroll
    for (int u = 0; u < K; u++) {
        pb[u] = LT[A.w.idx[A.level + u]].br;
        const word_t x = ld(t + (size_t)(A.level + u) * n);
#pragma unroll
        for (int v = 0; v < V; v++) y[v][u] = x.v[v];
    }
    const word_t tl = ld(t + (size_t)jl * n), cl = ld(c + (size_t)jl * n);
#pragma unroll
    for (int v = 0; v < V; v++) ks_group_tail_special<K>(y[v], pb, A.inv, A.level);
    u64 last[V];
    {
        const barrett_t bl = LT[A.w.idx[jl]].br;
#pragma unroll
        for (int v = 0; v < V; v++) last[v] = ks_group_tail_last<K>(tl.v[v], cl.v[v], y[v], bl, A.inv, A.level);
    }
    constexpr int JB = 4;
    for (int j0 = 0; j0 < jl; j0 += JB) {
        word_t xt[JB], xc[JB];
#pragma unroll
        for (int r = 0; r < JB; r++) {
            const int j = j0 + r < jl ? j0 + r : jl - 1;   // past the end: the block's spare registers repeat the last row, unused
            xt[r] = ld(t + (size_t)j * n);
            xc[r] = ld(c + (size_t)j * n);
        }
#pragma unroll
        for (int r = 0; r < JB; r++) {
            const int j = j0 + r;
            if (j < jl) {
                const barrett_t bj = LT[A.w.idx[j]].br;
                u64 res[V];
#pragma unroll
                for (int v = 0; v < V; v++) res[v] = ks_group_tail_rescale_limb<K>(xt[r].v[v], xc[r].v[v], y[v], last[v], bj, A.inv, R.qlinv[j], j);
                if constexpr (V == 2) {
                    u64x2_t w;
                    w.x = res[0]; w.y = res[1];
                    *(u64x2_t*)(o + (size_t)j * n) = w;
                } else {
                    o[(size_t)j * n] = res[0];
                }
            }
        }
    }
}

// Hoisted rotations on grouped-digit keys, the tail of ALL rotations of a tile in one launch (tfhe_rotate_many_grouped,
// tfhe_matmul_diag_grouped): T = INTT(S') [n_tile][batch][2][nw][N], the inverse-transformed key sums of the UNROTATED digits against
// the prepared keys;  out[r][b][s] = sigma_g(c_s) [s = 0] + the K-step contraction of sigma_g(T[r][b][s])  (ks_group_rot_tail_coeff).
// The grouped counterpart of k_ks_rot_tail, with its two measured decisions: scatter form -- the nw source rows and the addend are
// read in order and coefficient i is stored at g i mod N -- and the XCD-cooperative walk -- the workgroups of one XCD (blockIdx.x & 7)
// share ONE row group (r, b, s) at a time, so that its level windows of N words stay in that XCD's L2 until their lines are complete.
// Per row group nw rows (+ level addend rows for s = 0) in and level rows out.  The per-limb constants sit in LDS.
// out_stride: words of `out` between two rotations (the caller's whole batch, not the chunk).  grid: 8 * TFHE_ROT_TAIL_SLOTS.
struct ks_group_rot_t {
    u64 g[TFHE_DOT_MAX];
    size_t out_stride;
};
template <int K>
__global__ __launch_bounds__(256) void k_ks_group_rot_tail(const u64* __restrict__ T, const u64* __restrict__ ct, u64* __restrict__ out,
                                                            const ntt_limb_t* __restrict__ LT, ks_group_arg_t A, ks_group_rot_t G, u32 n, u32 batch,
                                                            u32 ngroups) {
    __shared__ barrett_t lb[TFHE_MAX_LIMBS];
    __shared__ tw_t linv[K ? K : 1][TFHE_MAX_LIMBS];
    const u32 level = (u32)A.level, nw = (u32)A.nw;
    for (u32 j = threadIdx.x; j < nw; j += blockDim.x) {
        lb[j] = LT[A.w.idx[j]].br;
#pragma unroll
        for (int t = 0; t < K; t++) linv[t][j] = A.inv[t][j];
    }
    __syncthreads();
    const u32 xcd = blockIdx.x & 7u, slot = blockIdx.x >> 3, nslot = gridDim.x >> 3;
    const u64 mask2n = 2ull * n - 1;
    for (u32 grp = xcd; grp < ngroups; grp += 8u) {   // grp = (r * batch + b) * 2 + s
        const u32 s = grp & 1u, b = (grp >> 1) % batch, r = (grp >> 1) / batch;
        const u64 g = G.g[r];
        const u64* tg = T + (size_t)grp * nw * n;
        const u64* cg = s == 0 ? ct + ((size_t)b * 2 * level) * n : nullptr;   // 2-element input: only c_1 has an addend (rlwe_she.jl:324)
        u64* og = out + (size_t)r * G.out_stride + ((size_t)b * 2 + s) * level * n;
        for (u32 i = slot * blockDim.x + threadIdx.x; i < n; i += nslot * blockDim.x) {
            const u64 t = ((u64)i * g) & mask2n;
            ks_group_rot_tail_coeff<K>(tg + i, cg ? cg + i : nullptr, og, n, (u32)t & (n - 1), t >= n, (int)level, lb, linv);
        }
    }
}
// ---- the evaluation-domain rotation phase on grouped-digit keys (mdg_rotations, md_api.inc) -------------------------------------------
// k_md_special_perm for K special limbs: PB[grp][t] = S'[grp][level + t] o pi_g, grp = (r * batch + b) * 2 + s, out of the key sums in
// the EPI layout (epi_pair): both components of a position come from one 16-byte gather.  The XCD-cooperative walk of
// k_md_special_perm over the rows (ciphertext, special limb): one window of 2 N words per XCD at a time, teams for small rows.
__global__ __launch_bounds__(256) void k_mdg_special_perm(const u64* __restrict__ S, u64* __restrict__ PB, rot_tail_arg_t G, u32 n, u32 nw,
                                                           u32 level, u32 nsp, u32 batch, u32 ngroups) {
    const u32 xcd = blockIdx.x & 7u, slot = blockIdx.x >> 3, nslot = gridDim.x >> 3;
    const u32 spt = n / blockDim.x >= nslot ? nslot : (n / blockDim.x ? n / blockDim.x : 1u), teams = nslot / spt, team = slot / spt, ts = slot % spt;
    if (team >= teams) return;
    for (u32 row = team * 8u + xcd; row < (ngroups / 2u) * nsp; row += 8u * teams) {   // row = ci * nsp + t, ciphertext ci = r * batch + b
        const u32 ci = row / nsp, t = row % nsp;
        const u64 g = G.g[ci / batch];
        const u64x2_t* s = (const u64x2_t*)(S + epi_pair(ci, level + t, 0u, nw, n));
        u64 *d0 = PB + ((size_t)(2u * ci) * nsp + t) * n, *d1 = d0 + (size_t)nsp * n;
        for (u32 m = ts * blockDim.x + threadIdx.x; m < n; m += spt * blockDim.x) {
            const u64x2_t w = s[galois_ntt_pos(m, g, n)];
            d0[m] = w.x;
            d1[m] = w.y;
        }
    }
}
// U [groups][level][N] from PB [groups][K][N], the inverse-transformed special limbs (coefficient domain, canonical): per coefficient
// the triangular steps on the K special words, then -tail_j(0) for every ciphertext limb (mdg_lift_coeff).  A stream: K rows in,
// `level` rows out per group, V coefficients per thread (V = 2: 16-byte loads and stores, as k_ks_group_tail); the constants sit in
// LDS, as in k_ks_group_rot_tail.  K + 1 words live per coefficient.  grid: groups * gx workgroups, gx = ceil(N / (256 V)).
template <int K, int V>
__global__ __launch_bounds__(256) void k_mdg_lift(const u64* __restrict__ PB, u64* __restrict__ U, const ntt_limb_t* __restrict__ LT,
                                                   ks_group_arg_t A, u32 n, u32 gx) {
    __shared__ barrett_t lb[TFHE_MAX_LIMBS];
    __shared__ tw_t linv[K][TFHE_MAX_LIMBS];
    const u32 level = (u32)A.level, nw = (u32)A.nw;
    for (u32 j = threadIdx.x; j < nw; j += blockDim.x) {
        lb[j] = LT[A.w.idx[j]].br;
#pragma unroll
        for (int t = 0; t < K; t++) linv[t][j] = A.inv[t][j];
    }
    __syncthreads();
    const u32 i = ((blockIdx.x % gx) * 256 + threadIdx.x) * (u32)V;
    const size_t grp = blockIdx.x / gx;
    if (i >= n) return;
    const u64* p = PB + grp * K * n + i;
    u64* u = U + grp * level * n + i;
    if constexpr (V == 2) {
        u64 y[2][K];
#pragma unroll
        for (int t = 0; t < K; t++) {
            const u64x2_t x = *(const u64x2_t*)(p + (size_t)t * n);
            y[0][t] = x.x; y[1][t] = x.y;
        }
#pragma unroll
        for (int v = 0; v < 2; v++) ks_group_tail_special<K>(y[v], lb + level, linv, (int)level);
        for (u32 j = 0; j < level; j++) {
            const barrett_t bj = lb[j];
            u64x2_t r;
            r.x = mdg_lift_limb<K>(y[0], bj, linv, (int)j);
            r.y = mdg_lift_limb<K>(y[1], bj, linv, (int)j);
            *(u64x2_t*)(u + (size_t)j * n) = r;
        }
    } else {
        mdg_lift_coeff<K>(p, u, n, (int)level, lb, linv);
    }
}
// ---- one fold step of tfhe_rotate_sum_grouped / tfhe_matmul_bsgs_fold_grouped in the evaluation domain (mdg_fold_run, md_api.inc) -------
// E[b][s][j][k] = X[b][s][j][k] + sum_{r < nrot} V[(r batch + b)][j][pi_r k].{s}: k_md_fold without the U stream and its factor -- the
// lifts are taken off after the inverse transform of E (k_mdg_fold_finish).  k_md_fold's walk, for its reasons: one XCD takes the row
// pair (b, 0, j), (b, 1, j) at a time, so that the two V windows of one rotation stay in one L2; teams for small rows; TFHE_MD_KB
// coefficients per thread; both components of a position from one 16-byte gather (epi_pair); rotation t + 1 requested before rotation
// t is added.  X, E: [batch][2][level][N], NTT domain; E may not be X.  grid: 8 * TFHE_MD_SLOTS.
__global__ __launch_bounds__(256) void k_mdg_fold_gather(const u64* __restrict__ X, const u64* __restrict__ V, u64* __restrict__ E,
                                                          const ntt_limb_t* __restrict__ LT, limb_sel_t sel, rot_tail_arg_t G, u32 n, u32 nw,
                                                          u32 nrot, u32 batch) {
    constexpr int KB = TFHE_MD_KB;
    const u32 level = (u32)sel.n;
    const u32 xcd = blockIdx.x & 7u, slot = blockIdx.x >> 3, nslot = gridDim.x >> 3;
    const u32 per = blockDim.x * KB, spt = n / per >= nslot ? nslot : (n / per ? n / per : 1u), teams = nslot / spt, team = slot / spt, ts = slot % spt;
    if (team >= teams) return;
    const u32 stride = spt * blockDim.x;
    struct term_t { u64 v0[KB], v1[KB]; };
    for (u32 pr = team * 8u + xcd; pr < batch * level; pr += 8u * teams) {
        const u32 j = pr % level, b = pr / level;
        const u64 q = LT[sel.idx[j]].q;
        const size_t row0 = ((size_t)b * 2 * level + j) * n, row1 = row0 + (size_t)level * n;
        for (u32 kb = ts * blockDim.x + threadIdx.x; kb < n; kb += stride * KB) {
            u32 k[KB];
#pragma unroll
            for (int i = 0; i < KB; i++) k[i] = kb + (u32)i * stride < n ? kb + (u32)i * stride : kb;   // (a clamped lane repeats kb; not stored)
            auto fetch = [&](u32 t, term_t& T) {
                const u64 g = G.g[t];
                const u64x2_t* pv = (const u64x2_t*)(V + epi_pair(t * batch + b, j, 0u, nw, n));   // both components of a position: one gather
#pragma unroll
                for (int i = 0; i < KB; i++) {
                    const u64x2_t vv = pv[galois_ntt_pos(k[i], g, n)];
                    T.v0[i] = vv.x; T.v1[i] = vv.y;
                }
            };
            u64 a0[KB], a1[KB];
#pragma unroll
            for (int i = 0; i < KB; i++) { a0[i] = X[row0 + k[i]]; a1[i] = X[row1 + k[i]]; }
            term_t cur;
            fetch(0, cur);
            for (u32 t = 0; t < nrot; t++) {
                term_t nxt;
                fetch(t + 1 < nrot ? t + 1 : t, nxt);
#pragma unroll
                for (int i = 0; i < KB; i++) {
                    a0[i] = addmod(a0[i], cur.v0[i], q);
                    a1[i] = addmod(a1[i], cur.v1[i], q);
                }
                cur = nxt;
            }
#pragma unroll
            for (int i = 0; i < KB; i++) {
                if (kb + (u32)i * stride < n) {
                    E[row0 + k[i]] = a0[i];
                    E[row1 + k[i]] = a1[i];
                }
            }
        }
    }
}
// dst[b][s][j] = E[b][s][j] - sum_{r < nrot} mdg_lift_limb(y_r)[j] (+ bias[j] for s = 0): E the inverse-transformed sum of
// k_mdg_fold_gather, y_r the "lasts" of the K inverse-transformed special rows PB[(r batch + b) 2 + s][t] (coefficient domain, canonical).
// A stream per (ciphertext, component): K nrot + level rows in (the special rows once per block of TFHE_MDG_FOLD_JB limbs), level rows
// out; V coefficients per thread (V = 2: 16-byte loads and stores, k_mdg_lift's alignment rule); the block's words stay in registers
// while the rotations go by, the block's E rows requested before the first special word is used; the constants sit in LDS, as in
// k_mdg_lift.  bias: null, or [level][N].  grid: batch * 2 * gx workgroups, gx = ceil(N / (256 V)).
template <int K, int V>
__global__ __launch_bounds__(256) void k_mdg_fold_finish(const u64* __restrict__ PB, const u64* __restrict__ E, const u64* __restrict__ bias,
                                                          u64* __restrict__ dst, const ntt_limb_t* __restrict__ LT, ks_group_arg_t A, u32 n, u32 gx,
                                                          u32 nrot, u32 batch) {
    constexpr int JB = TFHE_MDG_FOLD_JB;
    __shared__ barrett_t lb[TFHE_MAX_LIMBS];
    __shared__ tw_t linv[K][TFHE_MAX_LIMBS];
    const u32 level = (u32)A.level, nw = (u32)A.nw;
    for (u32 j = threadIdx.x; j < nw; j += blockDim.x) {
        lb[j] = LT[A.w.idx[j]].br;
#pragma unroll
        for (int t = 0; t < K; t++) linv[t][j] = A.inv[t][j];
    }
    __syncthreads();
    const u32 i = ((blockIdx.x % gx) * 256 + threadIdx.x) * (u32)V;
    const size_t grp = blockIdx.x / gx;   // b * 2 + s
    if (i >= n) return;
    const u64* p = PB + grp * K * n + i;
    const size_t rstride = (size_t)batch * 2 * K * n;   // one rotation's special rows
    const u64* e = E + grp * level * n + i;
    u64* o = dst + grp * level * n + i;
    const u64* bs = bias != nullptr && (grp & 1u) == 0 ? bias + i : nullptr;
    const auto ld = [](const u64* q, u64 (&w)[V]) {
        if constexpr (V == 2) {
            const u64x2_t x = *(const u64x2_t*)q;
            w[0] = x.x; w[1] = x.y;
        } else {
            w[0] = *q;
        }
    };
    for (u32 j0 = 0; j0 < level; j0 += JB) {
        const int nj = (int)(level - j0 < (u32)JB ? level - j0 : (u32)JB);
        u64 acc[V][JB];
#pragma unroll
        for (int r = 0; r < JB; r++) {
            u64 w[V];
            ld(e + (size_t)(j0 + (u32)(r < nj ? r : nj - 1)) * n, w);   // past the end: the spare registers repeat the last row, unused
#pragma unroll
            for (int v = 0; v < V; v++) acc[v][r] = w[v];
        }
        for (u32 r = 0; r < nrot; r++) {
            u64 y[V][K];
#pragma unroll
            for (int t = 0; t < K; t++) {
                u64 w[V];
                ld(p + (size_t)r * rstride + (size_t)t * n, w);
#pragma unroll
                for (int v = 0; v < V; v++) y[v][t] = w[v];
            }
#pragma unroll
            for (int v = 0; v < V; v++) mdg_fold_finish_coeff<K, JB>(acc[v], y[v], (int)j0, nj, (int)level, lb, linv);
        }
#pragma unroll
        for (int r = 0; r < JB; r++) {
            if (r < nj) {
                const u32 j = j0 + (u32)r;
                u64 res[V];
#pragma unroll
                for (int v = 0; v < V; v++) res[v] = acc[v][r];
                if (bs) {
                    u64 w[V];
                    ld(bs + (size_t)j * n, w);
#pragma unroll
                    for (int v = 0; v < V; v++) res[v] = addmod(res[v], w[v], lb[j].q);
                }
                if constexpr (V == 2) {
                    u64x2_t w;
                    w.x = res[0]; w.y = res[1];
                    *(u64x2_t*)(o + (size_t)j * n) = w;
                } else {
                    o[(size_t)j * n] = res[0];
                }
            }
        }
    }
}
#endif  // __HIPCC__
