// plain_tables.h -- host construction of the plaintext-codec table (plain_core.h).  Pure host C++ (no HIP):
// plain_api.inc uploads it, tests/plain_emul/ runs the same table against the same per-coefficient bodies on the CPU.
#pragma once
#include <cstring>
#include <string>
#include <vector>

#include "bfv_tables.h"
#include "host_math.h"
#include "plain_core.h"

struct plain_host_t {
    plain_tab_t tab;  // tab.cv's C/M/Aw point into cv's vectors
    conv_host_t cv;
};

namespace plainhost {
using hostmath::bigint;

inline int words_of(const bigint& a) {
    int n = (int)a.size();
    while (n > 1 && a[n - 1] == 0) n--;
    return n;
}
inline int bits_of(const bigint& a) {
    const int n = words_of(a);
    return (n - 1) * 64 + hostmath::bitlen(a[n - 1]);
}
// floor(a / d) and a mod d for a u64 divisor
inline bigint divmod_u64(const bigint& a, u64 d, u64* rem) {
    bigint q(a.size(), 0);
    u128 r = 0;
    for (size_t i = a.size(); i-- > 0;) {
        r = (r << 64) | a[i];
        q[i] = (u64)(r / d);
        r %= d;
    }
    if (rem) *rem = (u64)r;
    hostmath::big_trim(q);
    return q;
}
// floor(2^e / d), clamped to 2^64 - 1 (restoring division, one bit at a time; host set-up only)
inline u64 pow2_div(int e, const bigint& d) {
    const int n = words_of(d);
    std::vector<u64> r(n + 1, 0);
    u64 q = 0;
    bool over = false;
    for (int b = e; b >= 0; b--) {
        u64 c = b == e ? 1 : 0;  // shift in the bits of 2^e
        for (int i = 0; i <= n; i++) {
            const u64 nc = r[i] >> 63;
            r[i] = (r[i] << 1) | c;
            c = nc;
        }
        bool ge = r[n] != 0;
        if (!ge) {
            ge = true;
            for (int i = n - 1; i >= 0; i--)
                if (r[i] != d[i]) { ge = r[i] > d[i]; break; }
        }
        if (ge) {
            u64 br = 0;
            for (int i = 0; i <= n; i++) {
                const u64 di = i < n ? d[i] : 0;
                const u64 t = r[i] - di - br;
                br = (r[i] < di) || (r[i] - di < br);
                r[i] = t;
            }
            if (b >= 64) over = true;
            else q |= 1ull << b;
        }
    }
    return over ? ~0ull : q;
}
inline void put_words(const bigint& a, u64* dst) {
    for (int i = 0; i < TFHE_MAX_LIMBS; i++) dst[i] = i < (int)a.size() ? a[i] : 0;
}
}  // namespace plainhost

// qs = the ring's moduli in buffer limb order (distinct odd primes < 2^62).  Returns 0, or -1 with *err set (t outside
// [2, 2^62) or not below Q, or too many limbs).
inline int build_plain_host(const std::vector<u64>& qs, u64 t, plain_host_t* H, std::string* err) {
    using namespace hostmath;
    const int k = (int)qs.size();
    if (k < 1 || k > TFHE_MAX_LIMBS) { *err = "limbs out of range"; return -1; }
    if (t < 2 || t >= (1ull << 62)) { *err = "plaintext modulus t must lie in [2, 2^62)"; return -1; }
    bigint Q = big_from(1);
    for (u64 q : qs) Q = big_mul_u64(Q, q);
    if (plainhost::bits_of(Q) <= 64 && Q[0] <= t) { *err = "plaintext modulus t must be below the ring modulus Q"; return -1; }
    plain_tab_t& P = H->tab;
    memset(&P, 0, sizeof P);
    build_conv_host(qs, std::vector<u64>{t}, &H->cv);
    P.cv = H->cv.tab;
    P.nq = P.cv.nwords;
    const bigint D = plainhost::divmod_u64(Q, t, nullptr);  // Δ = Q ÷ t >= 1
    P.nd = plainhost::words_of(D);
    const int kb = plainhost::bits_of(D);
    P.sh = (u32)(kb - 1);
    P.R = plainhost::pow2_div(63 + kb, D);
    P.t = t;
    P.bt = make_barrett(t);
    plainhost::put_words(D, P.D);
    const bigint Dh = big_shr1(D);
    plainhost::put_words(Dh, P.Dh);
    u64 br = 0;  // ⌈Δ/2⌉ = Δ - Δ÷2
    for (int i = 0; i < TFHE_MAX_LIMBS; i++) {
        const u64 d = P.D[i] - P.Dh[i] - br;
        br = (P.D[i] < P.Dh[i]) || (P.D[i] - P.Dh[i] < br);
        P.Dc[i] = d;
    }
    plainhost::put_words(big_shr1(Q), P.Qh);
    for (int l = 0; l < k; l++) {
        P.enc[0][l] = make_tw(big_mod_u64(D, qs[l]), qs[l]);
        P.enc[1][l] = make_tw(1, qs[l]);
    }
    return 0;
}
