// tests/enc_core_emul/enc_core_emul.cpp -- CPU emulation of the fused encryption / decryption kernels (toyfhe.jl_amd/csrc/enc_core.h).
//
// TEST INFRASTRUCTURE ONLY: never loaded by the product package.  The per-thread phases of k_encrypt_fused / k_decrypt_fused are
// plain host / device functions (enc_core<A, LOGB, LOGT>); the kernels string them together with barriers and live behind the
// header's hipcc guard.  Here the same phases run on the host in the kernels' order -- one loop over the thread ids per phase,
// one loop boundary per __syncthreads() -- with the "registers" of every thread kept in arrays, the LDS image in a vector, and
// the host tables the library itself builds (ntt_tables.h).  The fp64 policy runs with range tracking on (fp64arith.h
// TFHE_TRACK): the largest |operand| / p that entered a product or a reduction is returned with the result.
#include <cstdint>
#include <vector>

#define TFHE_EMUL_TRACK_RANGE 1
static double g_fp_max_ratio = 0;  // fp64arith.h TFHE_TRACK
#include "../../toyfhe.jl_amd/csrc/bfv_tables.h"
#include "../../toyfhe.jl_amd/csrc/ntt_tables.h"
#include "../../toyfhe.jl_amd/csrc/enc_core.h"

namespace {

template <class A, int LOGB>
struct emul {
    static constexpr int LOGT = logt_for(LOGB);
    typedef enc_core<A, LOGB, LOGT> M;
    static constexpr int E = M::E;
    static constexpr u32 T = 1u << LOGT;
    typedef std::vector<u64> regs_t;                    // [T][E]: one register row of every thread
    typedef std::vector<typename A::elem> eregs_t;

    std::vector<u64> lds = std::vector<u64>(lds_words<LOGB, LOGT>());
    typename A::ctx C;
    barrett_t br;

    void forward(const regs_t& raw, regs_t& out) {
        for (u32 t = 0; t < T; t++) M::fwd_first(&raw[(size_t)t * E], lds.data(), C, t);
        for (u32 t = 0; t < T; t++) M::fwd_mid(lds.data(), C, t);
        for (u32 t = 0; t < T; t++) M::fwd_last(lds.data(), C, t, &out[(size_t)t * E]);
    }
    void inverse_head(eregs_t& v) {
        for (u32 t = 0; t < T; t++) M::inv_first(lds.data(), C, t, &v[(size_t)t * E]);
        for (u32 t = 0; t < T; t++) M::inv_mid(lds.data(), C, t);
    }
    // pk [2][N] (mask, masked), rand [3][N], msg [N] or null -> out [2][N]: the body of k_encrypt_fused<A, LOGB, LOGT, true>
    void encrypt(const ntt_limb_t& L, const u64* pk, const int32_t* rand, u64 mult_e, const u64* msg, u64* out) {
        const size_t n = (size_t)1 << LOGB;
        C = A::make(L);
        br = L.br;
        enc_rand_t R{};
        R.rand = rand; R.mult_e = mult_e; R.batch = 1;
        const u64 mq = mult_e % br.q;
        regs_t raw((size_t)T * E), uh((size_t)T * E);
        eregs_t v((size_t)T * E);
        u64 *o0 = out, *o1 = out + n;
        const u64 *mask = pk, *masked = pk + n;
        for (u32 t = 0; t < T; t++) {   // (one phase: a thread reads back the LDS words it wrote)
            M::template u_form<true>(lds.data(), R, 0, br, t);
            M::u_load(&raw[(size_t)t * E], lds.data(), t);
        }
        forward(raw, uh);
        for (u32 t = 0; t < T; t++) {
            M::prod_key(&v[(size_t)t * E], &uh[(size_t)t * E], masked, br, C, t);
            if (M::PARK) M::park_row(o1, &uh[(size_t)t * E], t);
        }
        inverse_head(v);
        for (u32 t = 0; t < T; t++) M::template inv_last_noise<true>(lds.data(), o0, msg, C, R, 0, 1, mq, br, t);
        for (u32 t = 0; t < T; t++) {
            if (M::PARK) M::prod_key_parked(&v[(size_t)t * E], o1, mask, br, C, t);
            else M::prod_key(&v[(size_t)t * E], &uh[(size_t)t * E], mask, br, C, t);
        }
        inverse_head(v);
        for (u32 t = 0; t < T; t++) M::template inv_last_noise<true>(lds.data(), o1, nullptr, C, R, 0, 2, mq, br, t);
    }
    // ct [polys][N], s [N] (NTT image) -> out [N]: the body of k_decrypt_fused<A, LOGB, LOGT, polys, ntt_in>
    void decrypt(const ntt_limb_t& L, const u64* s, const u64* ct, int polys, bool ntt_in, u64* out) {
        const size_t n = (size_t)1 << LOGB;
        C = A::make(L);
        br = L.br;
        regs_t acc((size_t)T * E), raw((size_t)T * E), ch((size_t)T * E);
        const u64 *c1 = ct, *c2 = ct + n, *c3 = ct + (size_t)(polys - 1) * n;
        if (ntt_in) {
            for (u32 t = 0; t < T; t++) {
                if (polys == 3) M::template dec_acc_ntt<3>(&acc[(size_t)t * E], c1, c2, c3, s, br, t);
                else M::template dec_acc_ntt<2>(&acc[(size_t)t * E], c1, c2, c3, s, br, t);
            }
        } else {
            for (u32 t = 0; t < T; t++) M::fwd_load(&raw[(size_t)t * E], c2, t);
            forward(raw, ch);
            for (u32 t = 0; t < T; t++) M::template dec_acc<true>(&acc[(size_t)t * E], &ch[(size_t)t * E], s, br, t);
            if (polys == 3) {
                for (u32 t = 0; t < T; t++) M::fwd_load(&raw[(size_t)t * E], c3, t);
                forward(raw, ch);
                for (u32 t = 0; t < T; t++) M::template dec_acc<false>(&acc[(size_t)t * E], &ch[(size_t)t * E], s, br, t);
            }
        }
        eregs_t v((size_t)T * E);
        for (u32 t = 0; t < T; t++) M::to_elem(&v[(size_t)t * E], &acc[(size_t)t * E], C);
        inverse_head(v);
        for (u32 t = 0; t < T; t++) M::inv_last(lds.data(), out, C, t, ntt_in ? nullptr : c1);
    }
};

template <class F>
int by_size(int logn, bool fp, F&& f) {
    switch (logn * 2 + (fp ? 1 : 0)) {
        case 24: { emul<ArithInt, 12> e; f(e); return 0; }
        case 25: { emul<ArithFp, 12> e; f(e); return 0; }
        case 26: { emul<ArithInt, 13> e; f(e); return 0; }
        case 27: { emul<ArithFp, 13> e; f(e); return 0; }
        case 28: { emul<ArithInt, 14> e; f(e); return 0; }
        case 29: { emul<ArithFp, 14> e; f(e); return 0; }
    }
    return -2;
}
int tables(int logn, uint64_t q, uint64_t psi, int fp, ntt_host_tabs_t& HT, ntt_limb_t* L) {
    const int64_t N = 1ll << logn;
    if (!psi) psi = hostmath::minimal_primitive_root(q, 2 * (u64)N);
    if (build_ntt_tables_all(N, q, psi, HT, L)) return -1;
    if (fp && !L->Wd) return -3;   // the modulus is not of fp64 size
    return 0;
}

}  // namespace

extern "C" {

// one (ciphertext, limb) item of k_encrypt_fused with given randomness.  Returns 0, -1 bad psi, -2 unsupported size, -3 fp64 policy
// asked for a modulus above TFHE_FP_QMAX.  *max_ratio: the range tracker's reading (0 for the u64 policy).
int enc_core_emul_encrypt(int logn, uint64_t q, int fp, const uint64_t* pk, const int32_t* rand, uint64_t mult_e, const uint64_t* msg,
                          uint64_t* out, double* max_ratio) {
    ntt_host_tabs_t HT;
    ntt_limb_t L;
    const int rc = tables(logn, q, 0, fp, HT, &L);
    if (rc) return rc;
    g_fp_max_ratio = 0;
    const int r2 = by_size(logn, fp != 0, [&](auto& e) { e.encrypt(L, pk, rand, mult_e, msg, out); });
    if (max_ratio) *max_ratio = g_fp_max_ratio;
    return r2;
}
int enc_core_emul_decrypt(int logn, uint64_t q, int fp, const uint64_t* s, const uint64_t* ct, int polys, int ntt_in, uint64_t* out,
                          double* max_ratio) {
    ntt_host_tabs_t HT;
    ntt_limb_t L;
    const int rc = tables(logn, q, 0, fp, HT, &L);
    if (rc) return rc;
    g_fp_max_ratio = 0;
    const int r2 = by_size(logn, fp != 0, [&](auto& e) { e.decrypt(L, s, ct, polys, ntt_in != 0, out); });
    if (max_ratio) *max_ratio = g_fp_max_ratio;
    return r2;
}

}  // extern "C"
