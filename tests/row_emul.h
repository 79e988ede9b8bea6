// tests/row_emul.h -- the CPU emulation harness of the fused row kernels (toyfhe.jl_amd/csrc/row_core.h and the kernels built on it).
//
// TEST INFRASTRUCTURE ONLY: never loaded by the product package.  The per-thread phases of a fused row kernel are plain host /
// device functions; the kernel strings them together with barriers and lives behind its header's hipcc guard.  An emulation runs
// the same phases on the host in the kernel's order -- one loop over the thread ids per phase, one loop boundary per
// __syncthreads() -- with the "registers" of every thread kept in arrays, the LDS image in a vector, and the host tables the
// library itself builds (ntt_tables.h).  This header holds what every such emulation needs: the per-(policy, size) state, the
// transform sequences, the switch over (policy, size) and the preamble of an extern "C" function.  A .cpp includes it, includes
// its kernel's header, derives `template <class A, int LOGB> struct emul : row_emul<A, LOGB>` with the kernel's body, and calls
// row_emul_run<emul>.  With TFHE_EMUL_TRACK_RANGE defined to 1 before the include, the fp64 policy runs with range tracking on
// (fp64arith.h TFHE_TRACK): the largest |operand| / p that entered a product or a reduction is returned with the result.
#pragma once
#include <cstdint>
#include <vector>

static double g_fp_max_ratio = 0;  // fp64arith.h TFHE_TRACK (ntt_tables.h pulls it in)
#include "../toyfhe.jl_amd/csrc/bfv_tables.h"
#include "../toyfhe.jl_amd/csrc/ntt_tables.h"
#include "../toyfhe.jl_amd/csrc/row_core.h"

template <class A, int LOGB>
struct row_emul {
    typedef A policy;
    static constexpr int LOGT = logt_for(LOGB);
    typedef row_core<A, LOGB, LOGT> RC;
    static constexpr int E = RC::E;
    static constexpr u32 T = 1u << LOGT;
    static constexpr size_t N = (size_t)1 << LOGB;
    typedef std::vector<u64> regs_t;                    // [T][E]: one register row of every thread
    typedef std::vector<typename A::elem> eregs_t;
    static regs_t regs() { return regs_t((size_t)T * E); }
    template <class V>
    static auto at(V& r, u32 t) { return &r[(size_t)t * E]; }   // thread t's registers

    std::vector<u64> lds = std::vector<u64>(lds_words<LOGB, LOGT>());
    typename A::ctx C;
    barrett_t br;
    void limb(const ntt_limb_t& L) { C = A::make(L); br = L.br; }

    // row_forward: (barrier: the previous transform's last pass has read LDS) | first | barrier | mid | barrier | last
    void forward(const regs_t& raw, regs_t& out) {
        for (u32 t = 0; t < T; t++) RC::fwd_first(at(raw, t), lds.data(), C, t);
        for (u32 t = 0; t < T; t++) RC::fwd_mid(lds.data(), C, t);
        for (u32 t = 0; t < T; t++) RC::fwd_last(lds.data(), C, t, at(out, t));
    }
    void forward_row(const u64* row, regs_t& out) {     // fwd_load, then the above
        regs_t raw = regs();
        for (u32 t = 0; t < T; t++) RC::fwd_load(at(raw, t), row, t);
        forward(raw, out);
    }
    // row_inverse_head: (barrier, as above) | first | barrier | mid | barrier; the caller's last pass follows
    void inverse_head(eregs_t& v) {
        for (u32 t = 0; t < T; t++) RC::inv_first(lds.data(), C, t, at(v, t));
        for (u32 t = 0; t < T; t++) RC::inv_mid(lds.data(), C, t);
    }
    void inverse(eregs_t& v, u64* dst, const u64* addend) {
        inverse_head(v);
        for (u32 t = 0; t < T; t++) RC::inv_last(lds.data(), dst, C, t, addend);
    }
};

// f(e) on a fresh EM<policy, logn>; -2: no fused row kernel at this size
template <template <class, int> class EM, class F>
int by_size(int logn, bool fp, F&& f) {
    switch (logn * 2 + (fp ? 1 : 0)) {
        case 24: { EM<ArithInt, 12> e; f(e); return 0; }
        case 25: { EM<ArithFp, 12> e; f(e); return 0; }
        case 26: { EM<ArithInt, 13> e; f(e); return 0; }
        case 27: { EM<ArithFp, 13> e; f(e); return 0; }
        case 28: { EM<ArithInt, 14> e; f(e); return 0; }
        case 29: { EM<ArithFp, 14> e; f(e); return 0; }
    }
    return -2;
}
// the dynamic LDS bytes the launch of a fused row kernel asks for at this size (launch_fused_rows: lds_words<LOGB, LOGT>() * 8); -2
// unsupported.  Every library built on this header exports it (tests/kernel_harness.py lds_bytes).
extern "C" long row_emul_lds_bytes(int logn) {
    long bytes = 0;
    const int rc = by_size<row_emul>(logn, false, [&](auto& e) { bytes = (long)e.lds.size() * 8; });
    return rc ? rc : bytes;
}
// The preamble of an extern "C" emulation function: the tables of the one limb (psi = 0: the minimal root), the tracker reset,
// f(e) with e.limb() set, the tracker's reading to *max_ratio (0 for the u64 policy).  Returns 0, -1 bad psi, -2 unsupported size,
// -3 fp64 policy asked for a modulus above TFHE_FP_QMAX.
template <template <class, int> class EM, class F>
int row_emul_run(int logn, uint64_t q, uint64_t psi, int fp, double* max_ratio, F&& f) {
    const int64_t N = 1ll << logn;
    if (!psi) psi = hostmath::minimal_primitive_root(q, 2 * (u64)N);
    ntt_host_tabs_t HT;
    ntt_limb_t L;
    if (build_ntt_tables_all(N, q, psi, HT, &L)) return -1;
    if (fp && !L.Wd) return -3;   // the modulus is not of fp64 size
    g_fp_max_ratio = 0;
    const int rc = by_size<EM>(logn, fp != 0, [&](auto& e) { e.limb(L); f(e); });
    if (max_ratio) *max_ratio = g_fp_max_ratio;
    return rc;
}
