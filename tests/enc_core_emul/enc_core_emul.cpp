// tests/enc_core_emul/enc_core_emul.cpp -- CPU emulation of the fused encryption / decryption kernels (toyfhe.jl_amd/csrc/enc_core.h):
// the bodies of k_encrypt_fused / k_decrypt_fused on the harness of tests/row_emul.h, range tracking on.  TEST INFRASTRUCTURE ONLY.
#define TFHE_EMUL_TRACK_RANGE 1
#include "../row_emul.h"
#include "../../toyfhe.jl_amd/csrc/enc_core.h"

namespace {

template <class A, int LOGB>
struct emul : row_emul<A, LOGB> {
    typedef row_emul<A, LOGB> H;
    typedef enc_core<A, LOGB, H::LOGT> M;
    using H::T; using H::C; using H::br; using H::lds; using H::at; using H::forward; using H::forward_row; using H::inverse_head;

    // pk [2][N] (mask, masked), rand [3][N], msg [N] or null -> out [2][N]: the body of k_encrypt_fused<A, LOGB, LOGT, true>
    void encrypt(const u64* pk, const int32_t* rand, u64 mult_e, const u64* msg, u64* out) {
        const size_t n = H::N;
        enc_rand_t R{};
        R.rand = rand; R.mult_e = mult_e; R.batch = 1;
        const u64 mq = mult_e % br.q;
        typename H::regs_t raw = H::regs(), uh = H::regs();
        typename H::eregs_t v((size_t)T * H::E);
        u64 *o0 = out, *o1 = out + n;
        const u64 *mask = pk, *masked = pk + n;
        for (u32 t = 0; t < T; t++) {   // (one phase: a thread reads back the LDS words it wrote)
            M::template u_form<true>(lds.data(), R, 0, br, t);
            M::u_load(at(raw, t), lds.data(), t);
        }
        forward(raw, uh);
        for (u32 t = 0; t < T; t++) {
            M::prod_key(at(v, t), at(uh, t), masked, br, C, t);
            if (M::PARK) M::park_row(o1, at(uh, t), t);
        }
        inverse_head(v);
        for (u32 t = 0; t < T; t++) M::template inv_last_noise<true>(lds.data(), o0, msg, C, R, 0, 1, mq, br, t);
        for (u32 t = 0; t < T; t++) {
            if (M::PARK) M::prod_key_parked(at(v, t), o1, mask, br, C, t);
            else M::prod_key(at(v, t), at(uh, t), mask, br, C, t);
        }
        inverse_head(v);
        for (u32 t = 0; t < T; t++) M::template inv_last_noise<true>(lds.data(), o1, nullptr, C, R, 0, 2, mq, br, t);
    }
    // ct [polys][N], s [N] (NTT image) -> out [N]: the body of k_decrypt_fused<A, LOGB, LOGT, polys, ntt_in>
    void decrypt(const u64* s, const u64* ct, int polys, bool ntt_in, u64* out) {
        const size_t n = H::N;
        typename H::regs_t acc = H::regs(), ch = H::regs();
        const u64 *c1 = ct, *c2 = ct + n, *c3 = ct + (size_t)(polys - 1) * n;
        if (ntt_in) {
            for (u32 t = 0; t < T; t++) {
                if (polys == 3) M::template dec_acc_ntt<3>(at(acc, t), c1, c2, c3, s, br, t);
                else M::template dec_acc_ntt<2>(at(acc, t), c1, c2, c3, s, br, t);
            }
        } else {
            forward_row(c2, ch);
            for (u32 t = 0; t < T; t++) M::template dec_acc<true>(at(acc, t), at(ch, t), s, br, t);
            if (polys == 3) {
                forward_row(c3, ch);
                for (u32 t = 0; t < T; t++) M::template dec_acc<false>(at(acc, t), at(ch, t), s, br, t);
            }
        }
        typename H::eregs_t v((size_t)T * H::E);
        for (u32 t = 0; t < T; t++) M::to_elem(at(v, t), at(acc, t), C);
        H::inverse(v, out, ntt_in ? nullptr : c1);
    }
};

}  // namespace

extern "C" {

// one (ciphertext, limb) item of k_encrypt_fused with given randomness.  Returns 0, -1 bad psi, -2 unsupported size, -3 fp64 policy
// asked for a modulus above TFHE_FP_QMAX.  *max_ratio: the range tracker's reading (0 for the u64 policy).
int enc_core_emul_encrypt(int logn, uint64_t q, int fp, const uint64_t* pk, const int32_t* rand, uint64_t mult_e, const uint64_t* msg,
                          uint64_t* out, double* max_ratio) {
    return row_emul_run<emul>(logn, q, 0, fp, max_ratio, [&](auto& e) { e.encrypt(pk, rand, mult_e, msg, out); });
}
int enc_core_emul_decrypt(int logn, uint64_t q, int fp, const uint64_t* s, const uint64_t* ct, int polys, int ntt_in, uint64_t* out,
                          double* max_ratio) {
    return row_emul_run<emul>(logn, q, 0, fp, max_ratio, [&](auto& e) { e.decrypt(s, ct, polys, ntt_in != 0, out); });
}

}  // extern "C"
