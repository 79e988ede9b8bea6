// mul_api.inc -- tfhe_mul_relin and, on grouped-digit keys, tfhe_mul_relin_grouped (at the end): ciphertext product + relinearisation
// (+ modswitch) of the schemes whose mul_expand / mul_contract are the identity (CKKS, BGV: rlwe_she.jl:39-40, :247-262); included by
// toyfhe_hip.hip.
//
// The call is the chain  nntt x2 -> tensor -> inntt -> keyswitch(polys = 3) -> rescale  run directly on the packed
// ciphertexts ([batch][2][level][N] is 2 batch polynomials), with the intermediates in the context workspace:
//     ws = [ region 0: the key switch's block / transform scratch | F: 4 rows per limb (NTT images) | T: 3 rows | R: 2 rows | parking rows x 2 ]
// The block is sized once, before the first launch, for both users (ws_layout.h): keyswitch_impl is handed region 0 as its span and
// lays out its own block there, by the plan that sized it.
//
// Routing of the product (forward transforms + tensor + inverse transforms) per limb:
//   N = 2^12 .. 2^14, variant 0, fp64-size limb : k_bfv_core_fused (MODE: packed operands / squaring / NTT-domain input)
//   N = 2^12 .. 2^14, variant 0, larger limb    : k_mul_core_int (mul_core.h), beside the fp64 core on the second lane
//   (the size test, the limb subsets and the two lanes: toyfhe_hip.hip, "the fused row kernels")
//   everything else                             : batched transform kernels + k_tensor on the packed layout (not fused)
// Every path leaves canonical residues, so the words are those of the chain through the public entry points.

namespace {

// parking rows (N words each) the two fused cores may ask for: one per workgroup (k_bfv_core_fused; k_mul_core_int below 2^14), two per
// workgroup at 2^14 (k_mul_core_int) -- the grids are at most two workgroups per CU below 2^14 and one at 2^14
size_t mr_park_rows(const tfhe_ctx* c) { return (size_t)2 * std::max(256, c->num_cus); }

// the subset `mask` (positions in the ciphertext) of the first `level` limbs as a selection + its place in the packed buffers
void mr_subset(int level, u32 mask, const u64* a, const u64* b, limb_sel_t* sel, core_alt_t* alt) {
    *sel = limb_subset(level, mask);
    *alt = core_alt_t{};
    alt->a = a; alt->b = b; alt->ns = level;
    for (int j = 0; j < sel->n; j++) alt->idx[j] = (signed char)sel->idx[j];
}
int64_t mr_transforms(unsigned items, bool square, bool ntt_in) { return (int64_t)items * ((ntt_in ? 0 : (square ? 2 : 4)) + 3); }

// the fused product of the fp64-size limbs of one chunk (mask: positions in the ciphertext); T rows of the other limbs untouched
int mr_core_fp(tfhe_ctx* c, const u64* a, const u64* b, u64* T, u64* scratch, int64_t nct, int level, u32 mask, bool whole, bool square, bool ntt_in) {
    limb_sel_t sel;
    core_alt_t alt;
    mr_subset(level, mask, a, b, &sel, &alt);
    if (sel.n == 0) return TFHE_OK;
    if (whole && !square && !ntt_in) {
        // every limb of the ring, general form: the BFV plan's own instantiation, fed from the packed ciphertexts (core_alt_t)
        bool done = false;
        const int rc = launch_bfv_core_fused(c, a, b, T, scratch, nct, sel, &done, &alt);
        if (rc) return rc;
        return done ? TFHE_OK : fail(TFHE_E_UNSUPPORTED, "internal: fused product core not available");
    }
    const unsigned items = (unsigned)(nct * sel.n);
    return dispatch_int<12, 14>(c->logN, [&](auto lb) {
        constexpr int LOGB = decltype(lb)::value, LOGT = logt_for(LOGB);
        void (*kern)(const u64*, const u64*, u64*, u64*, const ntt_limb_t*, limb_sel_t, u32, core_alt_t) = nullptr;
        if (square && ntt_in) kern = k_bfv_core_fused<ArithFp, LOGB, LOGT, false, CORE_PACKED | CORE_SQUARE | CORE_NTTIN>;
        else if (square) kern = k_bfv_core_fused<ArithFp, LOGB, LOGT, false, CORE_PACKED | CORE_SQUARE>;
        else if (ntt_in) kern = k_bfv_core_fused<ArithFp, LOGB, LOGT, false, CORE_PACKED | CORE_NTTIN>;
        else if constexpr (LOGB < 14) kern = k_bfv_core_fused<ArithFp, LOGB, LOGT, false, CORE_PACKED>;
        if (!kern) return fail(TFHE_E_UNSUPPORTED, "internal: this form of the fused product core is not built at N = 2^%d", LOGB);
        const unsigned grid = cu_grid(c, items, LOGB == 14 ? 1u : 2u);
        return launch_prof(c, mr_transforms(items, square, ntt_in), kern, dim3(grid), dim3(1 << LOGT), fused_lds_bytes<LOGB, LOGT>(), a, b, T,
                           scratch, c->limbs_dev, sel, items, alt);
    });
}
// the same for the limbs of the u64 policy (k_mul_core_int, mul_core.h)
int mr_core_int(tfhe_ctx* c, const u64* a, const u64* b, u64* T, u64* scratch, int64_t nct, int level, u32 mask, bool square, bool ntt_in) {
    limb_sel_t sel;
    core_alt_t alt;
    mr_subset(level, mask, a, b, &sel, &alt);
    if (sel.n == 0) return TFHE_OK;
    const unsigned items = (unsigned)(nct * sel.n);
    return dispatch_int<12, 14>(c->logN, [&](auto lb) {
        constexpr int LOGB = decltype(lb)::value, LOGT = logt_for(LOGB);
        auto kern = (square && ntt_in) ? k_mul_core_int<LOGB, LOGT, CORE_PACKED | CORE_SQUARE | CORE_NTTIN>
                    : square           ? k_mul_core_int<LOGB, LOGT, CORE_PACKED | CORE_SQUARE>
                    : ntt_in           ? k_mul_core_int<LOGB, LOGT, CORE_PACKED | CORE_NTTIN>
                                       : k_mul_core_int<LOGB, LOGT, CORE_PACKED>;
        const unsigned grid = cu_grid(c, items, LOGB == 14 ? 1u : 2u);
        return launch_prof(c, mr_transforms(items, square, ntt_in), kern, dim3(grid), dim3(1 << LOGT), (size_t)lds_words<LOGB, LOGT>() * 8, T, scratch,
                           c->limbs_dev, sel, items, alt);
    });
}

// batched kernels on the packed layout, restricted to the limbs of `mask` (0 = all): T [nct][3][level][N] coefficient domain
int mr_product_composed(tfhe_ctx* c, const u64* a, const u64* b, u64* F, u64* T, int64_t nct, int level, bool square, bool ntt_in) {
    const size_t N = (size_t)c->N;
    const limb_sel_t sel = first_limbs(level);
    const u64 *fa = a, *fb = b;
    int rc;
    if (!ntt_in) {
        u64* F2 = F + (size_t)nct * 2 * level * N;
        rc = run_ntt(c, false, a, F, nct * 2 * level, sel);
        if (rc) return rc;
        if (!square) {
            rc = run_ntt(c, false, b, F2, nct * 2 * level, sel);
            if (rc) return rc;
        }
        fa = F;
        fb = square ? F : F2;
    }
    rc = launch(c, k_tensor, row_grid((unsigned)(nct * level), N), dim3(256), 0, fa, fb, T, c->limbs_dev, sel, (u32)N);   // rlwe_she.jl:255-258
    if (rc) return rc;
    return run_ntt(c, true, T, T, nct * 3 * level, sel);
}

// The product stage of one call, decided once: what tfhe_mul_relin and tfhe_mul_relin_grouped share -- it does not depend on the key.
struct mr_product_t {
    bool square, ntt_in, fused;
    u32 fp_mask, int_mask;   // fused: the limbs of each core
    size_t f_rows;           // rows per limb of F (the NTT images of the operands: the batched path only)
    size_t park;             // words of parking rows per fused core
    size_t park_bytes() const { return fused ? 2 * park * 8 : 0; }
    // F, T and R (r_rows per limb: the key switch's result where a pass of its own follows it), then the parking rows
    ws_region_t F, T, R, SCR;
    void declare(ws_layout_t& L, int level, size_t r_rows) {
        F = L.rows(f_rows * level);
        T = L.rows((size_t)3 * level);
        R = L.rows(r_rows * level);
        SCR = L.tail(park_bytes());
    }
};
mr_product_t mr_product_plan(const tfhe_ctx* c, int level, bool square, bool ntt_in) {
    mr_product_t M{};
    M.square = square; M.ntt_in = ntt_in;
    const policy_split_t ps = policy_split(c, first_limbs(level));
    // fused product cores: N = 2^12 .. 2^14, variant 0.  The general form of the fp64 core with a limb subset is not built at 2^14
    // (it does not fit the registers there, DESIGN.md): a ring that mixes the policies takes the batched kernels for that form.
    M.fused = fused_rows_ok(c, level) && !(c->logN == 14 && ps.mixed_fp() && !square && !ntt_in);
    M.fp_mask = M.fused ? ps.fpmask : 0u;
    M.int_mask = M.fused ? (ps.all & ~ps.fpmask) : 0u;
    M.f_rows = (M.fused || ntt_in) ? 0 : (square ? 2 : 4);
    M.park = mr_park_rows(c) * (size_t)c->N;
    return M;
}
// T [nct][3][level][N], coefficient domain, from the packed operands a, b of one chunk; SCR: the parking rows of the two cores
int mr_product(tfhe_ctx* c, const mr_product_t& M, const u64* a, const u64* b, u64* F, u64* T, u64* SCR, int64_t nct, int level) {
    if (!M.fused) return mr_product_composed(c, a, b, F, T, nct, level, M.square, M.ntt_in);
    // both cores side by side (both_policies), over disjoint rows of T; the lanes join before the key switch reads T
    return both_policies(c, M.int_mask, M.fp_mask, [&](auto pol, u32 mask) {
        if constexpr (std::is_same<decltype(pol), ArithInt>::value) return mr_core_int(c, a, b, T, SCR, nct, level, mask, M.square, M.ntt_in);
        else return mr_core_fp(c, a, b, T, SCR + M.park, nct, level, mask, M.int_mask == 0, M.square, M.ntt_in);
    });
}

}  // namespace

extern "C" int tfhe_mul_relin(tfhe_ctx* c, int Lk, int level, int special, const uint64_t* evk, int n_digits, const uint64_t* c1,
                              const uint64_t* c2, int ntt_in, int rescale, uint64_t* out, int64_t batch) {
    // every check runs on the host before any device use
    if (!evk || !c1 || !c2 || !out) return fail(TFHE_E_BADARG, "null argument");
    if (batch < 0) return fail(TFHE_E_BADARG, "negative batch");
    if ((ntt_in != 0 && ntt_in != 1) || (rescale != 0 && rescale != 1)) return fail(TFHE_E_BADARG, "ntt_in and rescale are 0 or 1");
    if (rescale && level < 2) return fail(TFHE_E_LEVEL_MISMATCH, "modswitch after the product needs level >= 2, got %d", level);
    if (out == c1 || out == c2) return fail(TFHE_E_BADARG, "out overlaps an operand");
    int rc = ks_check(c, Lk, level, special, evk, n_digits, c1, 3, out, batch);
    if (rc) return rc;
    const size_t N = (size_t)c->N;
    const size_t in_bytes = (size_t)batch * 2 * level * N * 8, out_bytes = (size_t)batch * 2 * (level - (rescale ? 1 : 0)) * N * 8;
    if (ranges_overlap(out, out_bytes, c1, in_bytes) || ranges_overlap(out, out_bytes, c2, in_bytes))
        return fail(TFHE_E_BADARG, "out overlaps an operand");
    if (batch == 0) return TFHE_OK;
    if ((batch * 4 * level) << std::max(0, c->logN - 14) > 0x7fffffffll) return fail(TFHE_E_BADARG, "bad batch");

    const limb_sel_t sel = first_limbs(level);
    mr_product_t M = mr_product_plan(c, level, c1 == c2, ntt_in != 0);

    // region 0: the key switch's block, by its own plan (no rotation: sizes only, no table is computed), and the scratch of the product's
    // transforms (3 level rows: T's inverse).  chunk: F (NTT images of the operands: the batched path only), T (3 rows per limb), R (2:
    // the key switch's result when a modswitch follows)
    ws_layout_t L(N);
    L.scratch((size_t)3 * level, [=](int64_t chunk) {
        const ks_plan_t P = ks_plan(c, Lk, level, special, 3, chunk);
        return P.L.bytes(P.chunk);
    });
    M.declare(L, level, rescale ? 2 : 0);
    const int64_t chunk = chunk_of(c, batch, 256, (size_t)4096 << 20, L.per_ct_bytes());
    void* ws = nullptr;
    ws_scope_t scope;
    rc = ws_begin(c, L, chunk, nullptr, &ws, &scope);   // once, for both users, before any fork
    if (rc) return rc;
    const ws_span_t span{ws, L.region0(chunk)};
    u64 *F = L.at(ws, chunk, M.F), *T = L.at(ws, chunk, M.T), *R = L.at(ws, chunk, M.R), *SCR = L.at(ws, chunk, M.SCR);
    const int lo = level - (rescale ? 1 : 0);
    for (int64_t b0 = 0; b0 < batch; b0 += chunk) {
        const int64_t nct = std::min(chunk, batch - b0);
        rc = mr_product(c, M, c1 + (size_t)b0 * 2 * level * N, c2 + (size_t)b0 * 2 * level * N, F, T, SCR, nct, level);
        if (rc) return rc;
        u64* ks_out = rescale ? R : out + (size_t)b0 * 2 * level * N;
        rc = keyswitch_impl(c, Lk, level, special, evk, T, 3, ks_out, nct, 0, false, false, false, &span);   // rlwe_she.jl:315-347
        if (rc) return rc;
        if (rescale) {
            rc = do_rescale(c, R, out + (size_t)b0 * 2 * lo * N, nct * 2, sel);       // crt.jl:215-228 on both components
            if (rc) return rc;
        }
    }
    return TFHE_OK;
}

// ---- the same on grouped-digit keys (tfhe_keyswitch_grouped's gadget): tfhe_mul_relin_grouped ---------------------------------------
// The product stage is tfhe_mul_relin's; the key switch is ksg_chunk on a plan and regions carved HERE, from one block sized before the
// first launch:
//     ws = [ region 0: the plan's block (its transform scratch | S | digits) | F | T | R (n_special == 0 only) | parking rows x 2 ]
// With a special prime the modswitch rides on the key switch's tail (k_ks_group_tail_rescale: no R region, the result goes straight
// into `out`); without one there is no tail to ride on and ks_plain_tail -> do_rescale are composed through R.  The chunk follows
// chunk_of over the larger of the two per-ciphertext footprints (the product's rows, the key switch's rows).
extern "C" int tfhe_mul_relin_grouped(tfhe_ctx* c, int Lk, int level, int k, int group, const uint64_t* evk, int n_digits, const uint64_t* c1,
                                      const uint64_t* c2, int ntt_in, int rescale, uint64_t* out, int64_t batch) {
    // every check runs on the host before any device use (ks_group_mul_check, ks_group_core.h)
    char msg[160];
    bool nothing = false;
    int rc = ks_group_mul_check(!c || !evk || !c1 || !c2 || !out, c ? c->L : 0, c ? c->N : 0, c ? c->logN : 0, Lk, level, k, group, n_digits, batch, ntt_in,
                                rescale, (uintptr_t)c1, (uintptr_t)c2, (uintptr_t)out, &nothing, msg, sizeof msg);
    if (rc) return fail(rc, "%s", msg);
    if (nothing) return TFHE_OK;
    group = std::min(group, level);   // (one digit: every larger group is the whole ciphertext ring)

    const size_t N = (size_t)c->N;
    const limb_sel_t sel = first_limbs(level);
    mr_product_t M = mr_product_plan(c, level, c1 == c2, ntt_in != 0);
    const bool ride = rescale && k > 0;                       // the rescale rides on the tail
    const size_t r_rows = rescale && !ride ? 2 : 0;
    ksg_plan_t P;                                             // (the regions are carved here, for the chunk decided here: not P.chunk)
    rc = ksg_plan(c, Lk, level, k, group, 3, batch, false, &P);
    if (rc) return rc;
    // region 0: the plan's block, and the scratch of the product's transforms (3 level rows: T's inverse)
    ws_layout_t L(N);
    L.scratch((size_t)3 * level, [&P](int64_t chunk) { return P.L.bytes(chunk); });
    M.declare(L, level, r_rows);
    const int64_t chunk = chunk_of(c, batch, 256, (size_t)4096 << 20, std::max(L.per_ct_bytes(), P.L.per_ct_bytes()));
    ks_group_rescale_t rs{};
    if (ride)
        for (int j = 0; j < level - 1; j++) rs.qlinv[j] = hostmath::make_tw(hostmath::invmod_prime(c->q[level - 1] % c->q[j], c->q[j]), c->q[j]);
    void* ws = nullptr;
    ws_scope_t scope;
    rc = ws_begin(c, L, chunk, nullptr, &ws, &scope);   // once, for both users, before any fork
    if (rc) return rc;
    u64 *S = P.L.at(ws, chunk, P.S), *dig = P.L.at(ws, chunk, P.dig);
    u64 *F = L.at(ws, chunk, M.F), *T = L.at(ws, chunk, M.T), *R = L.at(ws, chunk, M.R), *SCR = L.at(ws, chunk, M.SCR);
    const int lo = level - (rescale ? 1 : 0);
    for (int64_t b0 = 0; b0 < batch; b0 += chunk) {
        const int64_t nct = std::min(chunk, batch - b0);
        rc = mr_product(c, M, c1 + (size_t)b0 * 2 * level * N, c2 + (size_t)b0 * 2 * level * N, F, T, SCR, nct, level);
        if (rc) return rc;
        u64* dst = out + (size_t)b0 * 2 * lo * N;
        {
            const ws_scope_t ks(c->ws_scratch, P.L.region0(chunk));   // the key switch's transforms stay in ITS region 0, before S
            rc = ksg_chunk(c, P, evk, T, r_rows ? R : dst, nct, S, dig, ride ? &rs : nullptr);
        }
        if (rc) return rc;
        if (r_rows) {
            rc = do_rescale(c, R, dst, nct * 2, sel);         // crt.jl:215-228 on both components
            if (rc) return rc;
        }
    }
    return TFHE_OK;
}
