// tests/keygen_core_emul/keygen_core_emul.cpp -- CPU emulation of the fused key-generation kernel (toyfhe.jl_amd/csrc/keygen_core.h).
//
// TEST INFRASTRUCTURE ONLY: never loaded by the product package.  The per-thread phases of k_evalkey_fused are plain host / device
// functions (key_core<A, LOGB, LOGT> over enc_core<A, LOGB, LOGT>); the kernel strings them together with barriers and lives behind
// the header's hipcc guard.  Here the same phases run on the host in the kernel's order -- one loop over the thread ids per phase,
// one loop boundary per __syncthreads() -- with the "registers" of every thread kept in arrays, the LDS image in a vector, and the
// host tables the library itself builds (ntt_tables.h).  The fp64 policy runs with range tracking on (fp64arith.h TFHE_TRACK):
// the largest |operand| / p that entered a product or a reduction is returned with the result.
#include <cstdint>
#include <vector>

#define TFHE_EMUL_TRACK_RANGE 1
static double g_fp_max_ratio = 0;  // fp64arith.h TFHE_TRACK
#include "../../toyfhe.jl_amd/csrc/bfv_tables.h"
#include "../../toyfhe.jl_amd/csrc/ntt_tables.h"
#include "../../toyfhe.jl_amd/csrc/keygen_core.h"

namespace {

template <class A, int LOGB>
struct emul {
    static constexpr int LOGT = logt_for(LOGB);
    typedef key_core<A, LOGB, LOGT> KC;
    typedef typename KC::M M;
    static constexpr int E = M::E;
    static constexpr u32 T = 1u << LOGT;
    typedef std::vector<u64> regs_t;                    // [T][E]: one register row of every thread

    std::vector<u64> lds = std::vector<u64>(lds_words<LOGB, LOGT>());
    typename A::ctx C;

    void forward(const regs_t& raw, regs_t& out) {
        for (u32 t = 0; t < T; t++) M::fwd_first(&raw[(size_t)t * E], lds.data(), C, t);
        for (u32 t = 0; t < T; t++) M::fwd_mid(lds.data(), C, t);
        for (u32 t = 0; t < T; t++) M::fwd_last(lds.data(), C, t, &out[(size_t)t * E]);
    }
    // one (component, limb) item of k_evalkey_fused<A, LOGB, LOGT, true>: mask [N] residues, noise [N] signed, s / old [N] NTT
    // images (old may be null), gamma the gadget residue, gel the Galois element (0: s s) -> out [2][N]
    void item(const ntt_limb_t& L, const u64* s, const u64* old, u64 gamma, u64 gel, const u64* mask, const int32_t* noise, u64 mult_e,
              u64* out) {
        const size_t n = (size_t)1 << LOGB;
        C = A::make(L);
        const barrett_t br = L.br;
        // the kernel's own argument structs: one key, one digit, one limb
        u64 tab[3] = {(u64)(uintptr_t)out, gel, gamma};
        key_arg_t K{};
        K.secret = s; K.old = old; K.tab = tab; K.n_keys = 1; K.n_digits = 1; K.key_limbs = 1; K.gadget = 1;
        key_rand_t R{};
        R.mask_rand = mask; R.noise_rand = noise; R.mult_e = mult_e;
        run(K, R, 0, 0, 1, br, s, old, n, out);
    }
    // the same item with device randomness (k_evalkey_fused<A, LOGB, LOGT, false>): component m of the call, limb j of key_limbs (the
    // limb byte of the uniform counter); the table L, s and out are those of that one limb
    void item_stream(const ntt_limb_t& L, const u64* s, u64 gamma, u64 gel, const key_rand_t& R, u64 m, u32 j, u32 key_limbs, u64* out) {
        const size_t n = (size_t)1 << LOGB;
        C = A::make(L);
        u64 tab[3] = {(u64)(uintptr_t)out, gel, gamma};
        key_arg_t K{};
        K.secret = s; K.old = nullptr; K.tab = tab; K.n_keys = 1; K.n_digits = 1; K.key_limbs = 1; K.gadget = 1;
        run(K, R, m, j, key_limbs, L.br, s, nullptr, n, out);
    }
    void run(const key_arg_t& K, const key_rand_t& R, u64 m, u32 j, u32 key_limbs, const barrett_t& br, const u64* s, const u64* old, size_t n,
             u64* out) {
        const u64 g = key_gamma(K, 0, 0);
        const int mode = key_old_mode(K, 0, g);
        u64 *row0 = out, *row1 = row0 + n;
        regs_t raw((size_t)T * E), ah((size_t)T * E), eh((size_t)T * E);
        if (R.mask_rand) {
            for (u32 t = 0; t < T; t++) M::fwd_load(&raw[(size_t)t * E], R.mask_rand, t);
        } else {
            for (u32 t = 0; t < T; t++) {   // (one phase: a thread reads back the LDS words it wrote)
                KC::mask_form(lds.data(), R, m, j, key_limbs, br.q, t);
                M::u_load(&raw[(size_t)t * E], lds.data(), t);
            }
        }
        forward(raw, ah);
        for (u32 t = 0; t < T; t++) KC::store_mask(row0, &ah[(size_t)t * E], t);
        for (u32 t = 0; t < T; t++) {   // (one phase: a thread reads back the LDS words it wrote)
            if (R.mask_rand) KC::template noise_form<true>(lds.data(), R, m, R.mult_e % br.q, br, t);
            else KC::template noise_form<false>(lds.data(), R, m, R.mult_e % br.q, br, t);
            M::u_load(&raw[(size_t)t * E], lds.data(), t);
        }
        forward(raw, eh);
        for (u32 t = 0; t < T; t++) KC::combine(mode, row1, row0, &ah[(size_t)t * E], &eh[(size_t)t * E], s, old, g, key_galois(K, 0), br, t);
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

}  // namespace

extern "C" {

// one item of k_evalkey_fused with given randomness.  Returns 0, -1 bad psi, -2 unsupported size, -3 fp64 policy asked for a modulus
// above TFHE_FP_QMAX.  *max_ratio: the range tracker's reading (0 for the u64 policy).
int keygen_core_emul_item(int logn, uint64_t q, int fp, const uint64_t* s, const uint64_t* old, uint64_t gamma, uint64_t gel,
                          const uint64_t* mask, const int32_t* noise, uint64_t mult_e, uint64_t* out, double* max_ratio) {
    ntt_host_tabs_t HT;
    ntt_limb_t L;
    const int64_t N = 1ll << logn;
    if (build_ntt_tables_all(N, q, hostmath::minimal_primitive_root(q, 2 * (u64)N), HT, &L)) return -1;
    if (fp && !L.Wd) return -3;
    g_fp_max_ratio = 0;
    const int rc = by_size(logn, fp != 0, [&](auto& e) { e.item(L, s, old, gamma, gel, mask, noise, mult_e, out); });
    if (max_ratio) *max_ratio = g_fp_max_ratio;
    return rc;
}

// one item of k_evalkey_fused with device randomness: component m, limb j of key_limbs, old^ = s^ s^ (gel 0) or the secret under
// x -> x^gel.  noise_out [N]: the signed integers key_noise_int drew for the item (what the kernel transforms, times mult_e).
int keygen_core_emul_item_stream(int logn, uint64_t q, int fp, const uint64_t* s, uint64_t gamma, uint64_t gel, double sigma_e, uint64_t mult_e,
                                 uint64_t seed, uint32_t stream_mask, uint32_t stream_noise, uint64_t mask_poly, uint64_t noise_poly,
                                 uint64_t poly_stride, uint64_t m, uint32_t j, uint32_t key_limbs, uint64_t* out, int64_t* noise_out,
                                 double* max_ratio) {
    ntt_host_tabs_t HT;
    ntt_limb_t L;
    const int64_t N = 1ll << logn;
    if (build_ntt_tables_all(N, q, hostmath::minimal_primitive_root(q, 2 * (u64)N), HT, &L)) return -1;
    if (fp && !L.Wd) return -3;
    key_rand_t R{};
    R.sigma_e = sigma_e; R.mult_e = mult_e; R.seed = seed; R.mask_poly = mask_poly; R.noise_poly = noise_poly; R.poly_stride = poly_stride;
    R.stream_mask = stream_mask; R.stream_noise = stream_noise;
    g_fp_max_ratio = 0;
    const int rc = by_size(logn, fp != 0, [&](auto& e) { e.item_stream(L, s, gamma, gel, R, m, j, key_limbs, out); });
    for (int64_t k = 0; k < N; k++) noise_out[k] = (int64_t)key_noise_int<false>(R, m, (u32)k, (u32)logn);
    if (max_ratio) *max_ratio = g_fp_max_ratio;
    return rc;
}

// the dynamic LDS bytes the launch of k_evalkey_fused asks for at this size (keygen_api.inc: lds_words<LOGB, LOGT>() * 8); -2 unsupported
long keygen_core_emul_lds_bytes(int logn) {
    switch (logn) {
        case 12: return (long)lds_words<12, logt_for(12)>() * 8;
        case 13: return (long)lds_words<13, logt_for(13)>() * 8;
        case 14: return (long)lds_words<14, logt_for(14)>() * 8;
    }
    return -2;
}

}  // extern "C"
