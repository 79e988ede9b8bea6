// tests/mul_core_emul/mul_core_emul.cpp -- CPU emulation of the u64 fused product core (toyfhe.jl_amd/csrc/mul_core.h).
//
// TEST INFRASTRUCTURE ONLY: never loaded by the product package.  The per-thread phases of k_mul_core_int are plain host /
// device functions (mul_core_int<LOGB, LOGT>); the kernel strings them together with barriers and lives behind the header's
// hipcc guard.  Here the same phases run on the host in the kernel's order -- one loop over the thread ids per phase, one loop
// boundary per __syncthreads() -- with the "registers" of every thread kept in arrays, the LDS image and the parking rows in
// vectors, and the host tables the library itself builds (ntt_tables.h).  tests/test_mul_relin_cpu.py compares the three
// result rows with the oracle (enc_mul, then inverse transforms).
#include <cstdint>
#include <vector>

static double g_fp_max_ratio = 0;  // fp64arith.h TFHE_TRACK (ntt_tables.h pulls it in)
#include "../../toyfhe.jl_amd/csrc/bfv_tables.h"
#include "../../toyfhe.jl_amd/csrc/ntt_tables.h"
#include "../../toyfhe.jl_amd/csrc/mul_core.h"

namespace {

template <int LOGB>
struct emul {
    static constexpr int LOGT = logt_for(LOGB);
    typedef mul_core_int<LOGB, LOGT> M;
    static constexpr int E = M::E;
    static constexpr u32 T = 1u << LOGT;
    typedef std::vector<u64> regs_t;   // [T][E]: one register row of every thread

    std::vector<u64> lds = std::vector<u64>(lds_words<LOGB, LOGT>());
    ArithInt::ctx C;
    barrett_t br;

    void forward(const u64* row, regs_t& v) {
        regs_t raw((size_t)T * E);
        for (u32 t = 0; t < T; t++) M::fwd_load(&raw[(size_t)t * E], row, t);
        // (barrier: the previous transform's last pass has read LDS)
        for (u32 t = 0; t < T; t++) M::fwd_first(&raw[(size_t)t * E], lds.data(), C, t, &v[(size_t)t * E]);
        for (u32 t = 0; t < T; t++) M::fwd_mid(lds.data(), C, t);
        for (u32 t = 0; t < T; t++) M::fwd_last(lds.data(), C, t, &v[(size_t)t * E]);
    }
    void inverse(regs_t& v, u64* dst) {
        for (u32 t = 0; t < T; t++) M::inv_first(lds.data(), C, t, &v[(size_t)t * E]);
        for (u32 t = 0; t < T; t++) M::inv_mid(lds.data(), C, t);
        for (u32 t = 0; t < T; t++) M::inv_last(lds.data(), dst, C, t);
    }
    // a, b: [2][N] (b == a when squaring); out: [3][N]; the branches are those of k_mul_core_int
    void run(const ntt_limb_t& L, const u64* a, const u64* b, u64* out, bool square, bool ntt_in) {
        const size_t n = (size_t)1 << LOGB;
        C = ArithInt::make(L);
        br = L.br;
        regs_t A0((size_t)T * E), A1((size_t)T * E), v((size_t)T * E);
        std::vector<u64> p1(n), p2(n);
        auto R = [](regs_t& r, u32 t) { return &r[(size_t)t * E]; };
        if (ntt_in) {
            for (int k = 0; k < 3; k++) {
                for (u32 t = 0; t < T; t++) M::prod_ntt(R(v, t), a, a + n, b, b + n, k, square, br, t);
                inverse(v, out + k * n);
            }
        } else if (square) {
            forward(a, A0);
            forward(a + n, A1);
            for (int k = 0; k < 3; k++) {
                for (u32 t = 0; t < T; t++) M::prod_sq(R(v, t), R(A0, t), R(A1, t), k, br);
                inverse(v, out + k * n);
            }
        } else if (LOGB >= 14) {   // PARK2
            forward(a, A0);
            forward(a + n, v);
            for (u32 t = 0; t < T; t++) M::park_row(p1.data(), R(v, t), t);
            forward(b, v);
            for (u32 t = 0; t < T; t++) M::prod_b0_parked(R(v, t), R(A0, t), p1.data(), p2.data(), br, t);
            inverse(v, out);
            forward(b + n, v);
            for (u32 t = 0; t < T; t++) M::prod_b1_parked(R(v, t), R(A0, t), R(A1, t), p1.data(), p2.data(), br, t);
            inverse(A0, out + n);
            inverse(A1, out + 2 * n);
        } else {
            forward(a, A0);
            forward(a + n, A1);
            forward(b, v);
            for (u32 t = 0; t < T; t++) M::prod_b0(R(v, t), R(A0, t), R(A1, t), p1.data(), br, t);
            inverse(v, out);
            forward(b + n, v);
            for (u32 t = 0; t < T; t++) M::prod_b1(R(v, t), R(A0, t), R(A1, t), p1.data(), br, t);
            inverse(A0, out + n);
            inverse(A1, out + 2 * n);
        }
    }
};

}  // namespace

extern "C" {

// one (ciphertext, limb) item of k_mul_core_int: a, b [2][N] -> out [3][N].  Returns 0, -1 on bad psi, -2 on unsupported size.
int mul_core_emul(int logn, uint64_t q, uint64_t psi, int square, int ntt_in, const uint64_t* a, const uint64_t* b, uint64_t* out) {
    const int64_t N = 1ll << logn;
    if (!psi) psi = hostmath::minimal_primitive_root(q, 2 * (u64)N);
    ntt_host_tabs_t HT;
    ntt_limb_t L;
    if (build_ntt_tables_all(N, q, psi, HT, &L)) return -1;
    switch (logn) {
        case 12: { emul<12> e; e.run(L, a, b, out, square != 0, ntt_in != 0); return 0; }
        case 13: { emul<13> e; e.run(L, a, b, out, square != 0, ntt_in != 0); return 0; }
        case 14: { emul<14> e; e.run(L, a, b, out, square != 0, ntt_in != 0); return 0; }
    }
    return -2;
}

}  // extern "C"
