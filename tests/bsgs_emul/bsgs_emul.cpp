// tests/bsgs_emul/bsgs_emul.cpp -- CPU emulation of the accumulations of tfhe_matmul_diag (one output) and tfhe_matmul_bsgs (a tile
// of outputs): the bodies of toyfhe.jl_amd/csrc/lazy_sum.h strung together in the order of k_md_acc (gather form) and
// k_md_acc_dense (kernels.h), one "thread" per coefficient, one limb.  TEST INFRASTRUCTURE ONLY.
#include <cstddef>
#include <cstdint>
#include "../../toyfhe.jl_amd/csrc/host_math.h"
#include "../../toyfhe.jl_amd/csrc/lazy_sum.h"

namespace {

// k_md_acc_dense: x [n], rot [nrot][n], diag [ngiant1][nrot + 1][n] -> inner [ngiant1][n]
template <int NG>
void dense(const barrett_t& br, u32 n, u32 nrot, u32 ngiant1, const u64* x, const u64* rot, const u64* diag, u64* inner) {
    const size_t dstride = n, jstride = (size_t)(nrot + 1u) * dstride;
    const u32 chunk = lazy_chunk(br.q);
    for (u32 i = 0; i < n; i++) {
        for (u32 j0 = 0; j0 < ngiant1; j0 += NG) {
            const u64* dg[NG];
            for (int o = 0; o < NG; o++) dg[o] = diag + (size_t)bsgs_tile_step(j0, (u32)o, ngiant1) * jstride + i;
            lazy_sums<NG> s;
            s.clear();
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
// k_md_acc, one row pair: x0, x1 [n]; v [nrot][n][2] (both components of a position side by side, epi_pair); u0, u1 [nrot][n];
// g [nrot]; diag as above -> inner0, inner1 [ngiant1][n]
template <bool USCALE, int NG>
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
            a0.clear(); a1.clear();
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

}  // namespace

extern "C" {

// the lazy-reduction chunk of a modulus
unsigned bsgs_emul_chunk(uint64_t q) { return lazy_chunk(q); }

// 0, or -1 for a tile the kernels are not built for
int bsgs_emul_dense(uint64_t q, int tile, uint32_t n, uint32_t nrot, uint32_t ngiant1, const uint64_t* x, const uint64_t* rot, const uint64_t* diag,
                    uint64_t* inner) {
    const barrett_t br = hostmath::make_barrett(q);
    switch (tile) {
        case 1: dense<1>(br, n, nrot, ngiant1, x, rot, diag, inner); return 0;
        case 2: dense<2>(br, n, nrot, ngiant1, x, rot, diag, inner); return 0;
        case 4: dense<4>(br, n, nrot, ngiant1, x, rot, diag, inner); return 0;
    }
    return -1;
}
// uscale != 0: the lifts arrive without the factor pinv (a residue below q), which the term applies itself
int bsgs_emul_gather(uint64_t q, int tile, int uscale, uint64_t pinv, uint32_t n, uint32_t nrot, uint32_t ngiant1, const uint64_t* x0, const uint64_t* x1,
                     const uint64_t* v, const uint64_t* u0, const uint64_t* u1, const uint64_t* g, const uint64_t* diag, uint64_t* inner0,
                     uint64_t* inner1) {
    const barrett_t br = hostmath::make_barrett(q);
    const tw_t pw = hostmath::make_tw(pinv, q);
#define GO(US, NG) gather<US, NG>(br, pw, n, nrot, ngiant1, x0, x1, v, u0, u1, g, diag, inner0, inner1); return 0
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
