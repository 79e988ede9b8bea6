// keygen_api.inc -- tfhe_evalkey_gen: every public, relinearisation and Galois key of a parameter set in one call (rlwe_she.jl:155-166,
// 273-304; modulusraising.jl:28-32); included by toyfhe_hip.hip.  The formula, the kernels and their ranges: keygen_core.h.
//
// Routing:
//   N = 2^12 .. 2^14, variant 0, key_limbs <= 32 : k_evalkey_fused, one (component, limb) item per workgroup pass; a ring that mixes
//                                                  the policies runs one launch per policy on the two lanes (the size test, the
//                                                  lanes and the launch: toyfhe_hip.hip, "the fused row kernels")
//   everything else                              : k_key_fill -> in-place nntt of the chunk's rows (one per key the chunk touches)
//                                                  -> k_key_finish
// The chunk counts COMPONENTS (key k, digit i): a component is two whole polynomials, the unit the batched transform takes.
// Staged: one small table (output pointers, Galois elements, gadget residues); the transforms' own scratch for N > 2^14.

namespace {

enum { KEY_CHUNK = 4096 };   // components per launch: grid dimensions stay below 65536, items far below 2^31

struct key_tab_t {           // the staged table, released (parked behind the stream's work) when the call returns
    void* p = nullptr;
    ~key_tab_t() { if (p) devalloc::release(p); }
};

template <class A>
int key_launch_fused(tfhe_ctx* c, u32 mask, int key_limbs, int64_t ncomp, const key_arg_t& K, const key_rand_t& R) {
    const limb_sel_t sel = limb_subset(key_limbs, mask);
    if (sel.n == 0) return TFHE_OK;
    const unsigned items = (unsigned)(ncomp * sel.n);
    auto kern = [&](auto lb) {
        constexpr int LOGB = decltype(lb)::value, LOGT = logt_for(LOGB);
        return R.mask_rand ? k_evalkey_fused<A, LOGB, LOGT, true> : k_evalkey_fused<A, LOGB, LOGT, false>;
    };
    return launch_fused_rows(c, items, (int64_t)items * 2, kern, c->limbs_dev, sel, items, K, R);
}

struct key_range_t {
    const char* lo;
    size_t bytes;
    bool out;
};

}  // namespace

extern "C" int tfhe_evalkey_gen(tfhe_ctx* c, int key_limbs, const uint64_t* secret, const uint64_t* old, const uint64_t* galois_elements,
                                int n_keys, const uint64_t* gadget, int n_digits, double sigma_e, uint64_t mult_e, uint64_t seed,
                                uint32_t stream_mask, uint32_t stream_noise, uint64_t mask_poly, uint64_t noise_poly, uint64_t poly_stride,
                                const uint64_t* mask_rand, const int32_t* noise_rand, uint64_t* const* evks) {
    // every check runs on the host before any device use, in the order the header states
    if (!secret || !evks) return fail(TFHE_E_BADARG, "null argument");
    if (n_keys < 0 || n_digits < 1) return fail(TFHE_E_BADARG, "n_keys=%d below 0 or n_digits=%d below 1", n_keys, n_digits);
    if (key_limbs < 1) return fail(TFHE_E_LEVEL_MISMATCH, "key_limbs=%d below 1", key_limbs);
    if ((mask_rand == nullptr) != (noise_rand == nullptr)) return fail(TFHE_E_BADARG, "mask_rand and noise_rand are given together or not at all");
    const u64 M = (u64)n_keys * (u64)n_digits;
    if (!mask_rand) {
        if (!(sigma_e >= 0) || sigma_e > 1e15) return fail(TFHE_E_BADARG, "sigma out of range");
        if (M) {
            const unsigned __int128 span = (unsigned __int128)(M - 1) * poly_stride, lim = (unsigned __int128)1 << 32;
            if (mask_poly + span >= lim || noise_poly + span >= lim) return fail(TFHE_E_BADARG, "polynomial counter reaches 2^32");
        }
        if (key_limbs > 256) return fail(TFHE_E_BADARG, "key_limbs=%d: the uniform stream's limb counter holds 256 limbs", key_limbs);
    }
    const bool need_g = gadget && !old;
    if (need_g && !galois_elements && n_keys > 0) return fail(TFHE_E_BADARG, "null argument: galois_elements");
    for (int k = 0; k < n_keys; k++) {
        if (!evks[k]) return fail(TFHE_E_BADARG, "null output %d", k);
        const void* o = (const void*)evks[k];
        if (o == (const void*)secret || (old && gadget && o == (const void*)old) || (mask_rand && (o == (const void*)mask_rand || o == (const void*)noise_rand)))
            return fail(TFHE_E_BADARG, "output %d overlaps an operand", k);
        for (int k2 = 0; k2 < k; k2++)
            if (evks[k2] == evks[k]) return fail(TFHE_E_BADARG, "output %d overlaps output %d", k, k2);
    }
    if (!c) return fail(TFHE_E_BADARG, "null context");
    if (key_limbs > c->L) return fail(TFHE_E_LEVEL_MISMATCH, "key_limbs=%d above the ring's %d moduli", key_limbs, c->L);
    const size_t N = (size_t)c->N;
    if (need_g)
        for (int k = 0; k < n_keys; k++) {
            const u64 g = galois_elements[k];
            if (g != 0 && ((g & 1) == 0 || g >= 2 * (u64)N)) return fail(TFHE_E_BADARG, "galois_elements[%d]=%llu is not 0 or odd and below 2N", k, (unsigned long long)g);
        }
    if (gadget)
        for (int i = 0; i < n_digits; i++)
            for (int j = 0; j < key_limbs; j++)
                if (gadget[(size_t)i * key_limbs + j] >= c->q[j]) return fail(TFHE_E_BADARG, "gadget residue of digit %d, limb %d is not a residue", i, j);
    const size_t row = (size_t)key_limbs * N;   // words of one polynomial
    if (M > (1ull << 40) / ((u64)2 * row)) return fail(TFHE_E_BADARG, "bad n_keys * n_digits");
    {
        std::vector<key_range_t> rg;
        rg.reserve((size_t)n_keys + 4);
        for (int k = 0; k < n_keys; k++) rg.push_back({(const char*)evks[k], (size_t)n_digits * 2 * row * 8, true});
        rg.push_back({(const char*)secret, row * 8, false});
        if (old && gadget) rg.push_back({(const char*)old, (size_t)n_keys * row * 8, false});
        if (mask_rand) {
            rg.push_back({(const char*)mask_rand, (size_t)M * row * 8, false});
            rg.push_back({(const char*)noise_rand, (size_t)M * N * 4, false});
        }
        std::sort(rg.begin(), rg.end(), [](const key_range_t& a, const key_range_t& b) { return a.lo < b.lo; });
        // sorted by start: a range that reaches into a later one reaches into the furthest-reaching earlier one's successor; the
        // operands may overlap one another, an output may overlap nothing
        const char *end_out = nullptr, *end_any = nullptr;
        for (const key_range_t& r : rg) {
            if (!r.bytes) continue;
            if ((r.out && end_any && r.lo < end_any) || (end_out && r.lo < end_out)) return fail(TFHE_E_BADARG, "an output overlaps an operand or another output");
            const char* hi = r.lo + r.bytes;
            if (!end_any || hi > end_any) end_any = hi;
            if (r.out && (!end_out || hi > end_out)) end_out = hi;
        }
    }
    if (n_keys == 0) return TFHE_OK;
    const bool fused = fused_rows_ok(c, key_limbs);
    if (!fused && c->logN > 17) return fail(TFHE_E_UNSUPPORTED, "N = 2^%d not supported (max 2^17)", c->logN);

    // the table: output pointers | Galois elements | gadget residues
    std::vector<u64> tab((size_t)2 * n_keys + (gadget ? (size_t)n_digits * key_limbs : 0));
    for (int k = 0; k < n_keys; k++) {
        tab[k] = (u64)(uintptr_t)evks[k];
        tab[(size_t)n_keys + k] = need_g ? galois_elements[k] : 0;
    }
    if (gadget) std::copy(gadget, gadget + (size_t)n_digits * key_limbs, tab.begin() + (size_t)2 * n_keys);
    key_tab_t dt;
    hipError_t e = devalloc::alloc(tab.size() * 8, &dt.p);
    if (e != hipSuccess) { dt.p = nullptr; return fail(TFHE_E_NOMEM, "hipMalloc(%zu): %s", tab.size() * 8, hipGetErrorString(e)); }
    e = hipMemcpyAsync(dt.p, tab.data(), tab.size() * 8, hipMemcpyHostToDevice, c->stream);   // pageable source: staged before the call returns
    if (e != hipSuccess) { (void)hipGetLastError(); return fail(TFHE_E_HIP, "hipMemcpyAsync: %s", hipGetErrorString(e)); }

    key_arg_t K{};
    K.secret = secret; K.old = gadget ? old : nullptr; K.tab = (const u64*)dt.p;
    K.n_keys = (u32)n_keys; K.n_digits = (u32)n_digits; K.key_limbs = (u32)key_limbs; K.gadget = gadget ? 1u : 0u;
    key_rand_t R{};
    R.mask_rand = mask_rand; R.noise_rand = noise_rand; R.sigma_e = sigma_e; R.mult_e = mult_e; R.seed = seed;
    R.mask_poly = mask_poly; R.noise_poly = noise_poly; R.poly_stride = poly_stride; R.stream_mask = stream_mask; R.stream_noise = stream_noise;
    const limb_sel_t sel = first_limbs(key_limbs);
    if (fused) {
        const policy_split_t ps = policy_split(c, sel);
        const int64_t chunk = chunk_of(c, (int64_t)M, KEY_CHUNK);
        for (int64_t m0 = 0; m0 < (int64_t)M; m0 += chunk) {
            const int64_t nc = std::min(chunk, (int64_t)M - m0);
            K.m0 = (u64)m0;
            const int rc = both_policies(c, ps.all & ~ps.fpmask, ps.fpmask, [&](auto pol, u32 mask) {
                return key_launch_fused<decltype(pol)>(c, mask, key_limbs, nc, K, R);
            });
            if (rc) return rc;
        }
        return TFHE_OK;
    }
    const u32 logn = (u32)c->logN, n = (u32)N;
    const unsigned gx = (n + 255) / 256;
    const int64_t chunk = chunk_of(c, (int64_t)M, KEY_CHUNK, (size_t)2048 << 20, 2 * row * 8);
    for (int64_t m0 = 0; m0 < (int64_t)M; m0 += chunk) {
        const int64_t nc = std::min(chunk, (int64_t)M - m0);
        K.m0 = (u64)m0;
        int rc = mask_rand ? launch(c, k_key_fill<true>, dim3(gx, (unsigned)nc), dim3(256), 0, c->limbs_dev, logn, K, R)
                           : launch(c, k_key_fill<false>, dim3(gx, (unsigned)nc), dim3(256), 0, c->limbs_dev, logn, K, R);
        if (rc) return rc;
        for (int64_t m = m0; m < m0 + nc;) {   // the chunk's rows lie in one piece per key
            const int64_t k = m / n_digits, i0 = m % n_digits, cnt = std::min<int64_t>(n_digits - i0, m0 + nc - m);
            u64* const p = evks[k] + (size_t)i0 * 2 * row;
            rc = run_ntt(c, false, p, p, cnt * 2 * key_limbs, sel);
            if (rc) return rc;
            m += cnt;
        }
        rc = launch(c, k_key_finish, dim3(gx, (unsigned)key_limbs, (unsigned)nc), dim3(256), 0, c->limbs_dev, logn, K);
        if (rc) return rc;
    }
    return TFHE_OK;
}
