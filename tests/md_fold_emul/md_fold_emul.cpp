// tests/md_fold_emul/md_fold_emul.cpp -- CPU emulation of the rotate-and-sum fold kernel k_md_fold (kernels.h): the body of
// toyfhe.jl_amd/csrc/lazy_sum.h (fold_term over gather_term) strung together in the kernel's order and with its WALK -- `nslot`
// workgroups of 256 threads split into teams for small rows, TFHE_MD_KB coefficients per thread, a clamped lane repeating its first
// coefficient unstored, rotation t + 1 fetched before rotation t is added -- for one row pair of one limb.  TEST INFRASTRUCTURE ONLY.
#include <cstddef>
#include <cstdint>
#include "../../toyfhe.jl_amd/csrc/host_math.h"
#include "../../toyfhe.jl_amd/csrc/lazy_sum.h"

namespace {

constexpr int KB = 8;   // TFHE_MD_KB

// x0, x1 [n]; v [nrot][n][2] (both components of a position side by side, epi_pair); u0, u1 [nrot][n]; g [nrot] -> s0, s1 [n].
// Returns the number of stores (every coefficient must be written exactly once: n per row)
template <bool USCALE>
size_t fold(u64 q, tw_t pinv, u32 n, u32 nrot, u32 nslot, const u64* x0, const u64* x1, const u64* v, const u64* u0, const u64* u1, const u64* g,
            u64* s0, u64* s1) {
    const u32 bdim = 256;
    size_t stores = 0;
    for (u32 slot = 0; slot < nslot; slot++) {
        const u32 per = bdim * KB, spt = n / per >= nslot ? nslot : (n / per ? n / per : 1u), teams = nslot / spt, team = slot / spt, ts = slot % spt;
        if (team >= teams || team != 0) continue;   // (the one row pair of this emulation belongs to team 0)
        const u32 stride = spt * bdim;
        for (u32 tid = 0; tid < bdim; tid++) {
            for (u32 kb = ts * bdim + tid; kb < n; kb += stride * KB) {
                u32 k[KB];
                for (int i = 0; i < KB; i++) k[i] = kb + (u32)i * stride < n ? kb + (u32)i * stride : kb;
                struct term_t { u64 v0[KB], v1[KB], u0[KB], u1[KB]; };
                auto fetch = [&](u32 t, term_t& T) {
                    for (int i = 0; i < KB; i++) {
                        const u64* vv = v + ((size_t)t * n + galois_ntt_pos(k[i], g[t], n)) * 2;
                        T.v0[i] = vv[0]; T.v1[i] = vv[1]; T.u0[i] = u0[(size_t)t * n + k[i]]; T.u1[i] = u1[(size_t)t * n + k[i]];
                    }
                };
                u64 a0[KB], a1[KB];
                for (int i = 0; i < KB; i++) { a0[i] = x0[k[i]]; a1[i] = x1[k[i]]; }
                term_t cur;
                fetch(0, cur);
                for (u32 t = 0; t < nrot; t++) {
                    term_t nxt;
                    fetch(t + 1 < nrot ? t + 1 : t, nxt);
                    for (int i = 0; i < KB; i++) {
                        a0[i] = fold_term<USCALE>(a0[i], cur.v0[i], cur.u0[i], pinv, q);
                        a1[i] = fold_term<USCALE>(a1[i], cur.v1[i], cur.u1[i], pinv, q);
                    }
                    cur = nxt;
                }
                for (int i = 0; i < KB; i++) {
                    if (kb + (u32)i * stride < n) {
                        s0[k[i]] = a0[i];
                        s1[k[i]] = a1[i];
                        stores++;
                    }
                }
            }
        }
    }
    return stores;
}

}  // namespace

extern "C" {

// uscale != 0: the lifts arrive without the factor pinv (a residue below q), which the term applies itself.  nslot: workgroups per XCD
// (TFHE_MD_SLOTS = 32 in the engine).  Returns the number of coefficients stored per row, or -1 for nrot < 1
long md_fold_emul(uint64_t q, int uscale, uint64_t pinv, uint32_t n, uint32_t nrot, uint32_t nslot, const uint64_t* x0, const uint64_t* x1,
                  const uint64_t* v, const uint64_t* u0, const uint64_t* u1, const uint64_t* g, uint64_t* s0, uint64_t* s1) {
    if (nrot < 1) return -1;
    const tw_t pw = hostmath::make_tw(pinv, q);
    return (long)(uscale ? fold<true>(q, pw, n, nrot, nslot, x0, x1, v, u0, u1, g, s0, s1)
                         : fold<false>(q, pw, n, nrot, nslot, x0, x1, v, u0, u1, g, s0, s1));
}

}  // extern "C"
