// enc_api.inc -- tfhe_encrypt / tfhe_decrypt_phase: public-key encryption (rlwe_she.jl:176-195) and the decryption phase
// b = c1 + s c2 (+ s^2 c3) (rlwe_she.jl:199-212) of a batch in one call each; included by toyfhe_hip.hip.
//
// Routing:
//   N = 2^12 .. 2^14, variant 0, level <= 32 : (except decryption of three NTT-domain components at 2^14)
//                                              k_encrypt_fused / k_decrypt_fused (enc_core.h), one (ciphertext, limb) item per workgroup
//                                              pass; a ring that mixes the policies runs one launch per policy on the two lanes
//                                              (the size test, the lanes and the launch: toyfhe_hip.hip, "the fused row kernels")
//   everything else                          : the batched transforms on the packed layout + the streaming kernels of enc_core.h
//       encrypt:  k_enc_fill -> nntt -> k_enc_keymul -> inntt (2 batch polynomials) -> k_enc_finish (in place)
//       decrypt:  nntt of the whole ciphertext (unless ntt_in) -> k_dec_keymul (c1 + s c2 + s^2 c3 on the images) -> inntt
//                 (the image of c1 is transformed and back instead of being added afterwards: one launch fewer, the same words)
// Workspace (context workspace, sized once before any lane fork; run_ntt takes the first rows of it as its scratch for N > 2^14):
//       encrypt:  [ transform scratch: 2 rows | U 1 | NTT(U) 1 | P 2 ]  x chunk x level x N words
//       decrypt:  [ transform scratch: polys rows | F polys (unless ntt_in) | B 1 ]
// Every path leaves canonical residues: the words are those of the chain through the public entry points.

namespace {

enum { ENC_CHUNK = 16384 };   // ciphertexts per launch: items = chunk x limbs stay far below 2^31, grid dimensions below 65536

template <class A>
int enc_launch_fused(tfhe_ctx* c, u32 mask, int key_limbs, int level, const u64* pk, const u64* msg, u64* out, int64_t nct, const enc_rand_t& R) {
    const limb_sel_t sel = limb_subset(level, mask);
    if (sel.n == 0) return TFHE_OK;
    const unsigned items = (unsigned)(nct * sel.n);
    auto kern = [&](auto lb) {
        constexpr int LOGB = decltype(lb)::value, LOGT = logt_for(LOGB);
        return R.rand ? k_encrypt_fused<A, LOGB, LOGT, true> : k_encrypt_fused<A, LOGB, LOGT, false>;
    };
    return launch_fused_rows(c, items, (int64_t)items * 3, kern, out, pk, msg, c->limbs_dev, sel, items, (u32)key_limbs, (u32)level, R);
}

template <class A>
int dec_launch_fused(tfhe_ctx* c, u32 mask, int level, const u64* secret, const u64* ct, int polys, bool ntt_in, u64* out, int64_t nct, u64 b0) {
    const limb_sel_t sel = limb_subset(level, mask);
    if (sel.n == 0) return TFHE_OK;
    if (c->logN == 14 && polys == 3 && ntt_in) return fail(TFHE_E_UNSUPPORTED, "internal: this form of the fused decryption is not built at N = 2^%d", 14);
    const unsigned items = (unsigned)(nct * sel.n);
    auto kern = [&](auto lb) {
        constexpr int LOGB = decltype(lb)::value, LOGT = logt_for(LOGB);
        if (polys == 2) return ntt_in ? k_decrypt_fused<A, LOGB, LOGT, 2, true> : k_decrypt_fused<A, LOGB, LOGT, 2, false>;
        if constexpr (LOGB < 14)   // (three NTT-domain components are not built at 2^14: refused above)
            if (ntt_in) return k_decrypt_fused<A, LOGB, LOGT, 3, true>;
        return k_decrypt_fused<A, LOGB, LOGT, 3, false>;
    };
    return launch_fused_rows(c, items, (int64_t)items * (ntt_in ? 1 : polys), kern, out, ct, secret, c->limbs_dev, sel, items, (u32)level, b0);
}

}  // namespace

extern "C" int tfhe_encrypt(tfhe_ctx* c, int key_limbs, int level, const uint64_t* pk, double sigma_u, double sigma_e, uint64_t mult_e,
                            uint64_t seed, uint32_t stream, uint64_t first_poly, const int32_t* rand, const uint64_t* msg, uint64_t* out,
                            int64_t batch) {
    // every check runs on the host before any device use
    if (!pk || !out) return fail(TFHE_E_BADARG, "null argument");
    if (batch < 0) return fail(TFHE_E_BADARG, "negative batch");
    if (key_limbs < 1 || level < 1 || level > key_limbs) return fail(TFHE_E_LEVEL_MISMATCH, "level=%d outside [1, key_limbs=%d]", level, key_limbs);
    if (!rand) {
        if (!(sigma_u >= 0) || sigma_u > 1e15 || !(sigma_e >= 0) || sigma_e > 1e15) return fail(TFHE_E_BADARG, "sigma out of range");
        if ((u64)batch > (1ull << 32) / 3 || first_poly > (1ull << 32) - 3 * (u64)batch) return fail(TFHE_E_BADARG, "polynomial counter exceeds 2^32");
    }
    if ((const void*)out == (const void*)pk || (const void*)out == (const void*)msg || (const void*)out == (const void*)rand)
        return fail(TFHE_E_BADARG, "out overlaps an operand");
    if (!c) return fail(TFHE_E_BADARG, "null context");
    if (key_limbs > c->L) return fail(TFHE_E_LEVEL_MISMATCH, "key_limbs=%d above the ring's %d moduli", key_limbs, c->L);
    const size_t N = (size_t)c->N;
    if ((u64)batch > (1ull << 40) / ((u64)2 * level * N)) return fail(TFHE_E_BADARG, "bad batch");
    const size_t out_bytes = (size_t)batch * 2 * level * N * 8;
    if (ranges_overlap(out, out_bytes, pk, (size_t)2 * key_limbs * N * 8) || (msg && ranges_overlap(out, out_bytes, msg, (size_t)batch * level * N * 8)) ||
        (rand && ranges_overlap(out, out_bytes, rand, (size_t)batch * 3 * N * 4)))
        return fail(TFHE_E_BADARG, "out overlaps an operand");
    if (batch == 0) return TFHE_OK;

    enc_rand_t R{};
    R.rand = rand; R.sigma_u = sigma_u; R.sigma_e = sigma_e; R.mult_e = mult_e; R.seed = seed; R.first_poly = first_poly; R.stream = stream;
    R.batch = (u64)batch;
    const limb_sel_t sel = first_limbs(level);
    if (fused_rows_ok(c, level)) {
        const policy_split_t ps = policy_split(c, sel);
        const int64_t chunk = chunk_of(c, batch, ENC_CHUNK);
        for (int64_t b0 = 0; b0 < batch; b0 += chunk) {
            const int64_t nct = std::min(chunk, batch - b0);
            R.b0 = (u64)b0;
            const int rc = both_policies(c, ps.all & ~ps.fpmask, ps.fpmask, [&](auto pol, u32 mask) {
                return enc_launch_fused<decltype(pol)>(c, mask, key_limbs, level, pk, msg, out, nct, R);
            });
            if (rc) return rc;
        }
        return TFHE_OK;
    }
    if (c->logN > 17) return fail(TFHE_E_UNSUPPORTED, "N = 2^%d not supported (max 2^17)", c->logN);
    const u32 logn = (u32)c->logN, n = (u32)N;
    const size_t row = (size_t)level * N;   // words of one polynomial
    const size_t scratch_rows = c->logN > 14 ? 2 : 0;
    const int64_t chunk = chunk_of(c, batch, 4096, (size_t)2048 << 20, (scratch_rows + 4) * row * 8);
    void* ws = nullptr;
    int rc = ensure_ws(c, (size_t)chunk * (scratch_rows + 4) * row * 8, &ws);   // once, before any lane fork of the transforms
    if (rc) return rc;
    u64* U = (u64*)ws + (size_t)chunk * scratch_rows * row;
    u64* UH = U + (size_t)chunk * row;
    u64* P = UH + (size_t)chunk * row;
    const unsigned gx = (n + 255) / 256;
    for (int64_t b0 = 0; b0 < batch; b0 += chunk) {
        const unsigned nct = (unsigned)std::min(chunk, batch - b0);
        R.b0 = (u64)b0;
        u64* o = out + (size_t)b0 * 2 * row;
        const u64* m = msg ? msg + (size_t)b0 * row : nullptr;
        rc = rand ? launch(c, k_enc_fill<true>, dim3(gx, nct), dim3(256), 0, U, c->limbs_dev, (u32)level, logn, R)
                  : launch(c, k_enc_fill<false>, dim3(gx, nct), dim3(256), 0, U, c->limbs_dev, (u32)level, logn, R);
        if (rc) return rc;
        rc = run_ntt(c, false, U, UH, (int64_t)nct * level, sel);
        if (rc) return rc;
        rc = launch(c, k_enc_keymul, dim3(gx, (unsigned)level, nct), dim3(256), 0, P, UH, pk, c->limbs_dev, (u32)level, (u32)key_limbs, logn);
        if (rc) return rc;
        rc = run_ntt(c, true, P, o, (int64_t)nct * 2 * level, sel);
        if (rc) return rc;
        if (c->ws != ws) return fail(TFHE_E_HIP, "internal: a transform moved the workspace");
        rc = rand ? launch(c, k_enc_finish<true>, dim3(gx, 2 * nct), dim3(256), 0, o, m, c->limbs_dev, (u32)level, logn, R)
                  : launch(c, k_enc_finish<false>, dim3(gx, 2 * nct), dim3(256), 0, o, m, c->limbs_dev, (u32)level, logn, R);
        if (rc) return rc;
    }
    return TFHE_OK;
}

extern "C" int tfhe_decrypt_phase(tfhe_ctx* c, int key_limbs, int level, const uint64_t* secret, const uint64_t* ct, int polys, int ntt_in,
                                  uint64_t* out, int64_t batch) {
    if (!secret || !ct || !out) return fail(TFHE_E_BADARG, "null argument");
    if (batch < 0) return fail(TFHE_E_BADARG, "negative batch");
    if (ntt_in != 0 && ntt_in != 1) return fail(TFHE_E_BADARG, "ntt_in is 0 or 1");
    if (polys != 2 && polys != 3) return fail(TFHE_E_UNSUPPORTED, "decrypt_phase takes 2 or 3 components, got %d", polys);
    if (key_limbs < 1 || level < 1 || level > key_limbs) return fail(TFHE_E_LEVEL_MISMATCH, "level=%d outside [1, key_limbs=%d]", level, key_limbs);
    if ((const void*)out == (const void*)ct || (const void*)out == (const void*)secret) return fail(TFHE_E_BADARG, "out overlaps an operand");
    if (!c) return fail(TFHE_E_BADARG, "null context");
    if (key_limbs > c->L) return fail(TFHE_E_LEVEL_MISMATCH, "key_limbs=%d above the ring's %d moduli", key_limbs, c->L);
    const size_t N = (size_t)c->N;
    if ((u64)batch > (1ull << 40) / ((u64)3 * level * N)) return fail(TFHE_E_BADARG, "bad batch");
    const size_t out_bytes = (size_t)batch * level * N * 8;
    if (ranges_overlap(out, out_bytes, ct, (size_t)batch * polys * level * N * 8) || ranges_overlap(out, out_bytes, secret, (size_t)key_limbs * N * 8))
        return fail(TFHE_E_BADARG, "out overlaps an operand");
    if (batch == 0) return TFHE_OK;

    const limb_sel_t sel = first_limbs(level);
    // (three NTT-domain components at N = 2^14: the fused form does not fit the registers there, enc_core.h)
    if (fused_rows_ok(c, level) && !(c->logN == 14 && polys == 3 && ntt_in)) {
        const policy_split_t ps = policy_split(c, sel);
        const int64_t chunk = chunk_of(c, batch, ENC_CHUNK);
        for (int64_t b0 = 0; b0 < batch; b0 += chunk) {
            const int64_t nct = std::min(chunk, batch - b0);
            const int rc = both_policies(c, ps.all & ~ps.fpmask, ps.fpmask, [&](auto pol, u32 mask) {
                return dec_launch_fused<decltype(pol)>(c, mask, level, secret, ct, polys, ntt_in != 0, out, nct, (u64)b0);
            });
            if (rc) return rc;
        }
        return TFHE_OK;
    }
    if (c->logN > 17) return fail(TFHE_E_UNSUPPORTED, "N = 2^%d not supported (max 2^17)", c->logN);
    const u32 logn = (u32)c->logN, n = (u32)N;
    const size_t row = (size_t)level * N;
    const size_t scratch_rows = c->logN > 14 ? (size_t)polys : 0, f_rows = ntt_in ? 0 : (size_t)polys;
    const int64_t chunk = chunk_of(c, batch, 4096, (size_t)2048 << 20, (scratch_rows + f_rows + 1) * row * 8);
    void* ws = nullptr;
    int rc = ensure_ws(c, (size_t)chunk * (scratch_rows + f_rows + 1) * row * 8, &ws);
    if (rc) return rc;
    u64* F = (u64*)ws + (size_t)chunk * scratch_rows * row;
    u64* B = F + (size_t)chunk * f_rows * row;
    const unsigned gx = (n + 255) / 256;
    for (int64_t b0 = 0; b0 < batch; b0 += chunk) {
        const unsigned nct = (unsigned)std::min(chunk, batch - b0);
        const u64* src = ct + (size_t)b0 * polys * row;
        if (!ntt_in) {
            rc = run_ntt(c, false, src, F, (int64_t)nct * polys * level, sel);
            if (rc) return rc;
            src = F;
        }
        rc = launch(c, k_dec_keymul, dim3(gx, (unsigned)level, nct), dim3(256), 0, B, src, secret, c->limbs_dev, (u32)level, (u32)polys, logn);
        if (rc) return rc;
        rc = run_ntt(c, true, B, out + (size_t)b0 * row, (int64_t)nct * level, sel);
        if (rc) return rc;
        if (c->ws != ws) return fail(TFHE_E_HIP, "internal: a transform moved the workspace");
    }
    return TFHE_OK;
}
