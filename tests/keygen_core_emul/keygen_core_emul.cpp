// tests/keygen_core_emul/keygen_core_emul.cpp -- CPU emulation of the fused key-generation kernel (toyfhe.jl_amd/csrc/keygen_core.h):
// the body of k_evalkey_fused on the harness of tests/row_emul.h, range tracking on.  TEST INFRASTRUCTURE ONLY.
#define TFHE_EMUL_TRACK_RANGE 1
#include "../row_emul.h"
#include "../../toyfhe.jl_amd/csrc/keygen_core.h"

namespace {

template <class A, int LOGB>
struct emul : row_emul<A, LOGB> {
    typedef row_emul<A, LOGB> H;
    typedef key_core<A, LOGB, H::LOGT> KC;
    typedef typename KC::M M;
    using H::T; using H::br; using H::lds; using H::at; using H::forward; using H::forward_row;

    // one (component, limb) item of k_evalkey_fused<A, LOGB, LOGT, true>: mask [N] residues, noise [N] signed, s / old [N] NTT
    // images (old may be null), gamma the gadget residue, gel the Galois element (0: s s) -> out [2][N]
    void item(const u64* s, const u64* old, u64 gamma, u64 gel, const u64* mask, const int32_t* noise, u64 mult_e, u64* out) {
        key_rand_t R{};
        R.mask_rand = mask; R.noise_rand = noise; R.mult_e = mult_e;
        item_stream(s, old, gamma, gel, R, 0, 0, 1, out);
    }
    // the same item with the randomness R describes (R.mask_rand == nullptr: device randomness, k_evalkey_fused<A, LOGB, LOGT, false>):
    // component m of the call, limb j of key_limbs (the limb byte of the uniform counter); the tables, s and out are those of that limb
    void item_stream(const u64* s, const u64* old, u64 gamma, u64 gel, const key_rand_t& R, u64 m, u32 j, u32 key_limbs, u64* out) {
        // the kernel's own argument structs: one key, one digit, one limb
        u64 tab[3] = {(u64)(uintptr_t)out, gel, gamma};
        key_arg_t K{};
        K.secret = s; K.old = old; K.tab = tab; K.n_keys = 1; K.n_digits = 1; K.key_limbs = 1; K.gadget = 1;
        const u64 g = key_gamma(K, 0, 0);
        const int mode = key_old_mode(K, 0, g);
        u64 *row0 = out, *row1 = row0 + H::N;
        typename H::regs_t raw = H::regs(), ah = H::regs(), eh = H::regs();
        if (R.mask_rand) {
            forward_row(R.mask_rand, ah);
        } else {
            for (u32 t = 0; t < T; t++) {   // (one phase: a thread reads back the LDS words it wrote)
                KC::mask_form(lds.data(), R, m, j, key_limbs, br.q, t);
                M::u_load(at(raw, t), lds.data(), t);
            }
            forward(raw, ah);
        }
        for (u32 t = 0; t < T; t++) KC::store_mask(row0, at(ah, t), t);
        for (u32 t = 0; t < T; t++) {   // (one phase: a thread reads back the LDS words it wrote)
            if (R.mask_rand) KC::template noise_form<true>(lds.data(), R, m, R.mult_e % br.q, br, t);
            else KC::template noise_form<false>(lds.data(), R, m, R.mult_e % br.q, br, t);
            M::u_load(at(raw, t), lds.data(), t);
        }
        forward(raw, eh);
        for (u32 t = 0; t < T; t++) KC::combine(mode, row1, row0, at(ah, t), at(eh, t), s, old, g, key_galois(K, 0), br, t);
    }
};

}  // namespace

extern "C" {

// one item of k_evalkey_fused with given randomness.  Returns 0, -1 bad psi, -2 unsupported size, -3 fp64 policy asked for a modulus
// above TFHE_FP_QMAX.  *max_ratio: the range tracker's reading (0 for the u64 policy).
int keygen_core_emul_item(int logn, uint64_t q, int fp, const uint64_t* s, const uint64_t* old, uint64_t gamma, uint64_t gel,
                          const uint64_t* mask, const int32_t* noise, uint64_t mult_e, uint64_t* out, double* max_ratio) {
    return row_emul_run<emul>(logn, q, 0, fp, max_ratio, [&](auto& e) { e.item(s, old, gamma, gel, mask, noise, mult_e, out); });
}

// one item of k_evalkey_fused with device randomness: component m, limb j of key_limbs, old^ = s^ s^ (gel 0) or the secret under
// x -> x^gel.  noise_out [N]: the signed integers key_noise_int drew for the item (what the kernel transforms, times mult_e).
int keygen_core_emul_item_stream(int logn, uint64_t q, int fp, const uint64_t* s, uint64_t gamma, uint64_t gel, double sigma_e, uint64_t mult_e,
                                 uint64_t seed, uint32_t stream_mask, uint32_t stream_noise, uint64_t mask_poly, uint64_t noise_poly,
                                 uint64_t poly_stride, uint64_t m, uint32_t j, uint32_t key_limbs, uint64_t* out, int64_t* noise_out,
                                 double* max_ratio) {
    key_rand_t R{};
    R.sigma_e = sigma_e; R.mult_e = mult_e; R.seed = seed; R.mask_poly = mask_poly; R.noise_poly = noise_poly; R.poly_stride = poly_stride;
    R.stream_mask = stream_mask; R.stream_noise = stream_noise;
    return row_emul_run<emul>(logn, q, 0, fp, max_ratio, [&](auto& e) {
        e.item_stream(s, nullptr, gamma, gel, R, m, j, key_limbs, out);
        for (size_t k = 0; k < e.N; k++) noise_out[k] = (int64_t)key_noise_int<false>(R, m, (u32)k, (u32)logn);
    });
}

}  // extern "C"
