// tests/md_acc_emul/md_acc_emul.cpp -- CPU emulation of the accumulations of tfhe_matmul_diag (one output), tfhe_matmul_bsgs (a tile of
// outputs; both nin = 1) and tfhe_matmul_bsgs_blocks (several inputs chained through the seed).  The bodies of
// toyfhe.jl_amd/csrc/lazy_sum.h strung together in the order of k_md_acc (gather form) and k_md_acc_dense (kernels.h), one "thread"
// per coefficient, one limb; input 0 runs the unseeded form over whatever `inner` holds, every later input the seeded form
// (csrc/md_api.inc: matmul_bsgs_run).  TEST INFRASTRUCTURE ONLY.
#include <cstddef>
#include <cstdint>
#include "../../toyfhe.jl_amd/csrc/host_math.h"
#include "../../toyfhe.jl_amd/csrc/lazy_sum.h"

namespace {

// k_md_acc_dense<NG, SEED>: x [n], rot [nrot][n], diag [ngiant1][nrot + 1][n] -> inner [ngiant1][n]
template <int NG, bool SEED>
void dense(const barrett_t& br, u32 n, u32 nrot, u32 ngiant1, const u64* x, const u64* rot, const u64* diag, u64* inner) {
    const size_t dstride = n, jstride = (size_t)(nrot + 1u) * dstride;
    const u32 chunk = lazy_chunk(br.q);
    for (u32 i = 0; i < n; i++) {
        for (u32 j0 = 0; j0 < ngiant1; j0 += NG) {
            const u64* dg[NG];
            for (int o = 0; o < NG; o++) dg[o] = diag + (size_t)bsgs_tile_step(j0, (u32)o, ngiant1) * jstride + i;
            lazy_sums<NG> s;
            if (SEED) {
                u64 w[NG];
                for (int o = 0; o < NG; o++) w[o] = j0 + (u32)o < ngiant1 ? inner[(size_t)(j0 + (u32)o) * n + i] : 0;
                s.seed(w);
            } else {
                s.clear();
            }
            u32 pend = 0;
            for (u32 k = 0; k <= nrot; k++) {
                const u64 v = k == 0 ? x[i] : rot[(size_t)(k - 1) * n + i];
                u64 d[NG];
                for (int o = 0; o < NG; o++) d[o] = dg[o][(size_t)k * dstride];
                if (lazy_fold_due(pend, chunk)) s.fold(br);
                s.mac(v, d);
                pend++;
            }
            for (int o = 0; o < NG; o++)
                if (j0 + (u32)o < ngiant1) inner[(size_t)(j0 + (u32)o) * n + i] = s.word(o, br);
        }
    }
}
// k_md_acc<USCALE, NG, SEED>, one row pair: x0, x1 [n]; v [nrot][n][2] (both components of a position side by side, epi_pair);
// u0, u1 [nrot][n]; g [nrot]; diag as above -> inner0, inner1 [ngiant1][n]
template <bool USCALE, int NG, bool SEED>
void gather(const barrett_t& br, tw_t pinv, u32 n, u32 nrot, u32 ngiant1, const u64* x0, const u64* x1, const u64* v, const u64* u0, const u64* u1,
            const u64* g, const u64* diag, u64* inner0, u64* inner1) {
    const size_t dstride = n, jstride = (size_t)(nrot + 1u) * dstride;
    const u32 chunk = lazy_chunk(br.q);
    for (u32 k = 0; k < n; k++) {
        for (u32 j0 = 0; j0 < ngiant1; j0 += NG) {
            const u64* dg[NG];
            for (int o = 0; o < NG; o++) dg[o] = diag + (size_t)bsgs_tile_step(j0, (u32)o, ngiant1) * jstride;
            lazy_sums<NG> a0, a1;
            u64 d[NG];
            for (int o = 0; o < NG; o++) d[o] = dg[o][k];
            if (SEED) {
                u64 s0[NG], s1[NG];
                for (int o = 0; o < NG; o++) {
                    const bool live = j0 + (u32)o < ngiant1;
                    s0[o] = live ? inner0[(size_t)(j0 + (u32)o) * n + k] : 0;
                    s1[o] = live ? inner1[(size_t)(j0 + (u32)o) * n + k] : 0;
                }
                a0.seed(s0); a1.seed(s1);
            } else {
                a0.clear(); a1.clear();
            }
            a0.mac(x0[k], d);
            a1.mac(x1[k], d);
            u32 pend = 1;
            for (u32 t = 0; t < nrot; t++) {
                const u32 kk = galois_ntt_pos(k, g[t], n);
                const u64* vv = v + ((size_t)t * n + kk) * 2;
                for (int o = 0; o < NG; o++) d[o] = dg[o][(size_t)(t + 1) * dstride + k];
                if (lazy_fold_due(pend, chunk)) { a0.fold(br); a1.fold(br); }
                a0.mac(gather_term<USCALE>(vv[0], u0[(size_t)t * n + k], pinv, br.q), d);
                a1.mac(gather_term<USCALE>(vv[1], u1[(size_t)t * n + k], pinv, br.q), d);
                pend++;
            }
            for (int o = 0; o < NG; o++) {
                if (j0 + (u32)o < ngiant1) {
                    inner0[(size_t)(j0 + (u32)o) * n + k] = a0.word(o, br);
                    inner1[(size_t)(j0 + (u32)o) * n + k] = a1.word(o, br);
                }
            }
        }
    }
}

template <int NG>
void dense_inputs(const barrett_t& br, u32 n, u32 nrot, u32 ngiant1, u32 nin, const u64* x, const u64* rot, const u64* diag, u64* inner) {
    const size_t rs = (size_t)(nrot ? nrot : 1u) * n, ds = (size_t)ngiant1 * (nrot + 1u) * n;
    for (u32 m = 0; m < nin; m++) {
        if (m == 0) dense<NG, false>(br, n, nrot, ngiant1, x, rot, diag, inner);
        else dense<NG, true>(br, n, nrot, ngiant1, x + (size_t)m * n, rot + m * rs, diag + m * ds, inner);
    }
}
template <bool USCALE, int NG>
void gather_inputs(const barrett_t& br, tw_t pinv, u32 n, u32 nrot, u32 ngiant1, u32 nin, const u64* x, const u64* v, const u64* u, const u64* g,
                   const u64* diag, u64* inner0, u64* inner1) {
    const size_t rs = (size_t)nrot * n, ds = (size_t)ngiant1 * (nrot + 1u) * n;
    for (u32 m = 0; m < nin; m++) {
        const u64 *xm = x + (size_t)m * 2 * n, *um = u + m * 2 * rs;
        if (m == 0) gather<USCALE, NG, false>(br, pinv, n, nrot, ngiant1, xm, xm + n, v, um, um + rs, g, diag, inner0, inner1);
        else gather<USCALE, NG, true>(br, pinv, n, nrot, ngiant1, xm, xm + n, v + m * 2 * rs, um, um + rs, g, diag + m * ds, inner0, inner1);
    }
}

}  // namespace

extern "C" {

// the lazy-reduction chunk of a modulus
unsigned md_acc_emul_chunk(uint64_t q) { return lazy_chunk(q); }

// x [nin][n], rot [nin][max(nrot, 1)][n], diag [nin][ngiant1][nrot + 1][n] -> inner [ngiant1][n] (whatever it holds on entry is
// overwritten by input 0).  0, or -1 for a tile the kernels are not built for
int md_acc_emul_dense(uint64_t q, int tile, uint32_t n, uint32_t nrot, uint32_t ngiant1, uint32_t nin, const uint64_t* x, const uint64_t* rot,
                           const uint64_t* diag, uint64_t* inner) {
    const barrett_t br = hostmath::make_barrett(q);
    switch (tile) {
        case 1: dense_inputs<1>(br, n, nrot, ngiant1, nin, x, rot, diag, inner); return 0;
        case 2: dense_inputs<2>(br, n, nrot, ngiant1, nin, x, rot, diag, inner); return 0;
        case 4: dense_inputs<4>(br, n, nrot, ngiant1, nin, x, rot, diag, inner); return 0;
    }
    return -1;
}
// x [nin][2][n], v [nin][nrot][n][2], u [nin][2][nrot][n], g [nrot] (one key set for every input), diag as above -> inner0, inner1
// [ngiant1][n].  uscale != 0: the lifts arrive without the factor pinv (a residue below q), which the term applies itself
int md_acc_emul_gather(uint64_t q, int tile, int uscale, uint64_t pinv, uint32_t n, uint32_t nrot, uint32_t ngiant1, uint32_t nin,
                            const uint64_t* x, const uint64_t* v, const uint64_t* u, const uint64_t* g, const uint64_t* diag, uint64_t* inner0,
                            uint64_t* inner1) {
    const barrett_t br = hostmath::make_barrett(q);
    const tw_t pw = hostmath::make_tw(pinv, q);
#define GO(US, NG) gather_inputs<US, NG>(br, pw, n, nrot, ngiant1, nin, x, v, u, g, diag, inner0, inner1); return 0
    switch (tile * 2 + (uscale ? 1 : 0)) {
        case 2: GO(false, 1);
        case 3: GO(true, 1);
        case 4: GO(false, 2);
        case 5: GO(true, 2);
        case 8: GO(false, 4);
        case 9: GO(true, 4);
    }
#undef GO
    return -1;
}

}  // extern "C"
