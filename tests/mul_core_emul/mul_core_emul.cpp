// tests/mul_core_emul/mul_core_emul.cpp -- CPU emulation of the u64 fused product core (toyfhe.jl_amd/csrc/mul_core.h): the body of
// k_mul_core_int on the harness of tests/row_emul.h, the parking rows in vectors.  TEST INFRASTRUCTURE ONLY.
// tests/test_mul_relin_cpu.py compares the three result rows with the oracle (enc_mul, then inverse transforms).
#include <type_traits>

#include "../row_emul.h"
#include "../../toyfhe.jl_amd/csrc/mul_core.h"

namespace {

template <class A, int LOGB>
struct emul : row_emul<A, LOGB> {
    typedef row_emul<A, LOGB> H;
    typedef mul_core_int<LOGB, H::LOGT> M;
    using H::T; using H::br; using H::at; using H::forward_row; using H::inverse;

    // a, b: [2][N] (b == a when squaring); out: [3][N]; the branches are those of k_mul_core_int
    void run(const u64* a, const u64* b, u64* out, bool square, bool ntt_in) {
        const size_t n = H::N;
        typename H::regs_t A0 = H::regs(), A1 = H::regs(), v = H::regs();
        std::vector<u64> p1(n), p2(n);
        if (ntt_in) {
            for (int k = 0; k < 3; k++) {
                for (u32 t = 0; t < T; t++) M::prod_ntt(at(v, t), a, a + n, b, b + n, k, square, br, t);
                inverse(v, out + k * n, nullptr);
            }
        } else if (square) {
            forward_row(a, A0);
            forward_row(a + n, A1);
            for (int k = 0; k < 3; k++) {
                for (u32 t = 0; t < T; t++) M::prod_sq(at(v, t), at(A0, t), at(A1, t), k, br);
                inverse(v, out + k * n, nullptr);
            }
        } else if (LOGB >= 14) {   // PARK2
            forward_row(a, A0);
            forward_row(a + n, v);
            for (u32 t = 0; t < T; t++) M::park_row(p1.data(), at(v, t), t);
            forward_row(b, v);
            for (u32 t = 0; t < T; t++) M::prod_b0_parked(at(v, t), at(A0, t), p1.data(), p2.data(), br, t);
            inverse(v, out, nullptr);
            forward_row(b + n, v);
            for (u32 t = 0; t < T; t++) M::prod_b1_parked(at(v, t), at(A0, t), at(A1, t), p1.data(), p2.data(), br, t);
            inverse(A0, out + n, nullptr);
            inverse(A1, out + 2 * n, nullptr);
        } else {
            forward_row(a, A0);
            forward_row(a + n, A1);
            forward_row(b, v);
            for (u32 t = 0; t < T; t++) M::prod_b0(at(v, t), at(A0, t), at(A1, t), p1.data(), br, t);
            inverse(v, out, nullptr);
            forward_row(b + n, v);
            for (u32 t = 0; t < T; t++) M::prod_b1(at(v, t), at(A0, t), at(A1, t), p1.data(), br, t);
            inverse(A0, out + n, nullptr);
            inverse(A1, out + 2 * n, nullptr);
        }
    }
};

}  // namespace

extern "C" {

// one (ciphertext, limb) item of k_mul_core_int: a, b [2][N] -> out [3][N].  Returns 0, -1 on bad psi, -2 on unsupported size.
int mul_core_emul(int logn, uint64_t q, uint64_t psi, int square, int ntt_in, const uint64_t* a, const uint64_t* b, uint64_t* out) {
    return row_emul_run<emul>(logn, q, psi, 0, nullptr, [&](auto& e) {
        if constexpr (std::is_same<typename std::decay_t<decltype(e)>::policy, ArithInt>::value)
            e.run(a, b, out, square != 0, ntt_in != 0);   // (the u64 policy only: by_size names both)
    });
}

}  // extern "C"
