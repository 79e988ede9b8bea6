// plain_api.inc -- BFV / BGV plaintext codecs (π, π⁻¹, bfv.jl:21-29, bgv.jl:21-25) and the BFV noise maximum
// (invariant_noise_budget, bfv.jl:137-166) on the device; included by toyfhe_hip.hip.  Bodies: plain_core.h.
//
// Kernels: one lane per coefficient, lanes of a wavefront on consecutive coefficients of one limb row (each limb load is one
// coalesced 512-byte row segment).  The limb / word loops are unrolled to the compile-time bound KM of plain_km(), so the
// per-lane arrays stay in registers up to 16 limbs.  The noise maximum is a two-pass reduction without atomics: every
// wavefront writes the maximum of its 64 coefficients (butterfly of cross-lane shuffles), then one workgroup per ciphertext
// reduces those partials in a fixed order.

struct tfhe_plain_plan {
    tfhe_ctx* ctx = nullptr;
    limb_sel_t sel;
    u64 t = 0;
    int nq = 0, nd = 0, km = 0;
    plain_tab_t* tab_dev = nullptr;
    std::vector<void*> allocs;
};

namespace {

#define PLAIN_BS 256
#define PLAIN_WAVES (PLAIN_BS / 64)
#define PLAIN_MAX_GRID_Y 65535

int plain_km(int k) { return k <= 1 ? 1 : k <= 2 ? 2 : k <= 4 ? 4 : k <= 8 ? 8 : k <= 16 ? 16 : TFHE_MAX_LIMBS; }

__global__ __launch_bounds__(PLAIN_BS) void k_plain_encode(const u64* __restrict__ m, u64* __restrict__ out,
                                                           const plain_tab_t* __restrict__ P, int bgv, u32 n) {
    const u32 k = blockIdx.x * PLAIN_BS + threadIdx.x, b = blockIdx.y;
    if (k >= n) return;
    const int L = P->cv.k;
    plain_encode_coeff(*P, bgv, m[(size_t)b * n + k], out + (size_t)b * L * n + k, n);
}

template <int KM, bool BGV>
__global__ __launch_bounds__(PLAIN_BS) void k_plain_decode(const u64* __restrict__ in, u64* __restrict__ out,
                                                           const plain_tab_t* __restrict__ P, u32 n) {
    const u32 k = blockIdx.x * PLAIN_BS + threadIdx.x, b = blockIdx.y;
    if (k >= n) return;
    const u64* c = in + (size_t)b * P->cv.k * n + k;
    out[(size_t)b * n + k] = BGV ? plain_bgv_decode_coeff<KM>(*P, c, n) : plain_bfv_decode_coeff<KM>(*P, c, n);
}

__device__ __forceinline__ u64 plain_shfl_xor(u64 v, int mask) {
    const int lo = __shfl_xor((int)(u32)v, mask, 64), hi = __shfl_xor((int)(u32)(v >> 32), mask, 64);
    return ((u64)(u32)hi << 32) | (u32)lo;
}
// w = max(w, the same array of lane ^ mask) over nd words, across the wavefront
template <int KM>
__device__ __forceinline__ void plain_wave_max(u64 (&w)[KM], int nd) {
#pragma unroll
    for (int mask = 1; mask < 64; mask <<= 1) {
        u64 o[KM];
#pragma unroll TFHE_PLAIN_UNROLL(KM)
        for (int i = 0; i < KM; i++) o[i] = i < nd ? plain_shfl_xor(w[i], mask) : 0;
        if (plain_cmp<KM>(o, w, nd) > 0) {
#pragma unroll TFHE_PLAIN_UNROLL(KM)
            for (int i = 0; i < KM; i++) w[i] = o[i];
        }
    }
}

// pass 1: part[b][word][G] (G = gridDim.x * PLAIN_WAVES partials per ciphertext) = max birem over one wavefront's coefficients
template <int KM>
__global__ __launch_bounds__(PLAIN_BS) void k_plain_noise_partial(const u64* __restrict__ in, u64* __restrict__ part,
                                                                  const plain_tab_t* __restrict__ P, u32 n) {
    const u32 k = blockIdx.x * PLAIN_BS + threadIdx.x, b = blockIdx.y;
    const int nd = P->nd;
    u64 w[KM];
    if (k < n) {
        plain_noise_coeff<KM>(*P, in + (size_t)b * P->cv.k * n + k, n, w);
    } else {
#pragma unroll TFHE_PLAIN_UNROLL(KM)
        for (int i = 0; i < KM; i++) w[i] = 0;
    }
    plain_wave_max<KM>(w, nd);
    const u32 lane = threadIdx.x & 63, G = gridDim.x * PLAIN_WAVES, g = blockIdx.x * PLAIN_WAVES + (threadIdx.x >> 6);
    if (lane == 0) {
#pragma unroll TFHE_PLAIN_UNROLL(KM)
        for (int i = 0; i < KM; i++)
            if (i < nd) part[((size_t)b * nd + i) * G + g] = w[i];
    }
}

// pass 2: one workgroup per ciphertext; out[b][word] = max over its G partials
template <int KM>
__global__ __launch_bounds__(PLAIN_BS) void k_plain_noise_reduce(const u64* __restrict__ part, u64* __restrict__ out, int nd, u32 G) {
    __shared__ u64 s[PLAIN_WAVES][KM];
    const u32 b = blockIdx.x;
    u64 w[KM];
#pragma unroll TFHE_PLAIN_UNROLL(KM)
    for (int i = 0; i < KM; i++) w[i] = 0;
    for (u32 g = threadIdx.x; g < G; g += PLAIN_BS) {
        u64 o[KM];
#pragma unroll TFHE_PLAIN_UNROLL(KM)
        for (int i = 0; i < KM; i++) o[i] = i < nd ? part[((size_t)b * nd + i) * G + g] : 0;
        if (plain_cmp<KM>(o, w, nd) > 0) {
#pragma unroll TFHE_PLAIN_UNROLL(KM)
            for (int i = 0; i < KM; i++) w[i] = o[i];
        }
    }
    plain_wave_max<KM>(w, nd);
    const u32 wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
#pragma unroll TFHE_PLAIN_UNROLL(KM)
        for (int i = 0; i < KM; i++) s[wave][i] = w[i];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int v = 1; v < PLAIN_WAVES; v++) {
            u64 o[KM];
#pragma unroll TFHE_PLAIN_UNROLL(KM)
            for (int i = 0; i < KM; i++) o[i] = s[v][i];
            if (plain_cmp<KM>(o, w, nd) > 0) {
#pragma unroll TFHE_PLAIN_UNROLL(KM)
                for (int i = 0; i < KM; i++) w[i] = o[i];
            }
        }
#pragma unroll TFHE_PLAIN_UNROLL(KM)
        for (int i = 0; i < KM; i++)
            if (i < nd) out[(size_t)b * nd + i] = w[i];
    }
}

#define PLAIN_KM_DISPATCH(km, X) \
    switch (km) {                \
        case 1: X(1); break;     \
        case 2: X(2); break;     \
        case 4: X(4); break;     \
        case 8: X(8); break;     \
        case 16: X(16); break;   \
        default: X(TFHE_MAX_LIMBS); break; \
    }

int plain_check(tfhe_plain_plan* p, int scheme, const void* a, const void* b, int64_t count) {
    if (count < 0) return fail(TFHE_E_BADARG, "negative count");
    if (scheme != TFHE_PLAIN_BFV && scheme != TFHE_PLAIN_BGV) return fail(TFHE_E_BADARG, "scheme %d is neither TFHE_PLAIN_BFV nor TFHE_PLAIN_BGV", scheme);
    if (!p || !a || !b) return fail(TFHE_E_BADARG, "null argument");
    return TFHE_OK;
}

}  // namespace

extern "C" {

int tfhe_plain_plan_create(tfhe_ctx* ctx, const int32_t* limb_idx, int limbs, uint64_t t, tfhe_plain_plan** out) {
    if (out) *out = nullptr;
    if (limbs < 1 || limbs > TFHE_MAX_LIMBS) return fail(TFHE_E_BADARG, "limbs=%d out of range [1,%d]", limbs, TFHE_MAX_LIMBS);
    if (t < 2 || t >= (1ull << 62)) return fail(TFHE_E_BADARG, "plaintext modulus t=%llu outside [2, 2^62)", (unsigned long long)t);
    if (!ctx || !out) return fail(TFHE_E_BADARG, "null argument");
    limb_sel_t sel;
    sel.n = limbs;
    for (int j = 0; j < limbs; j++) {
        const int v = limb_idx ? limb_idx[j] : j;
        if (v < 0 || v >= ctx->L) return fail(TFHE_E_BADARG, "limb_idx[%d]=%d outside the ring's %d moduli", j, v, ctx->L);
        for (int i = 0; i < j; i++)
            if (sel.idx[i] == v) return fail(TFHE_E_BADARG, "limb_idx[%d]=%d repeats limb_idx[%d]", j, v, i);
        sel.idx[j] = v;
    }
    std::vector<u64> qs(limbs);
    for (int j = 0; j < limbs; j++) qs[j] = ctx->q[sel.idx[j]];
    plain_host_t* H = new plain_host_t();
    std::string err;
    if (build_plain_host(qs, t, H, &err)) { delete H; return fail(TFHE_E_BADARG, "%s", err.c_str()); }
    tfhe_plain_plan* p = new tfhe_plain_plan();
    p->ctx = ctx; p->sel = sel; p->t = t;
    p->nq = H->tab.nq; p->nd = H->tab.nd; p->km = plain_km(limbs);
    plain_tab_t T = H->tab;
    auto up = [&](const std::vector<u64>& v, const u64** d) -> int {
        void* q = nullptr;
        hipError_t e = devalloc::malloc_retry(&q, std::max<size_t>(8, v.size() * 8));
        if (e != hipSuccess) return fail(TFHE_E_NOMEM, "allocating the plaintext-codec tables failed: %s", hipGetErrorString(e));
        p->allocs.push_back(q);
        e = hipMemcpy(q, v.data(), v.size() * 8, hipMemcpyHostToDevice);
        if (e != hipSuccess) return fail(TFHE_E_HIP, "hipMemcpy: %s", hipGetErrorString(e));
        *d = (const u64*)q;
        return TFHE_OK;
    };
    int rc = up(H->cv.C, &T.cv.C);
    if (!rc) rc = up(H->cv.M, &T.cv.M);
    if (!rc) rc = up(H->cv.Aw, &T.cv.Aw);
    delete H;
    if (!rc && devalloc::malloc_retry(&p->tab_dev, sizeof T) != hipSuccess) rc = fail(TFHE_E_NOMEM, "allocating the plaintext-codec table failed");
    if (!rc) {
        const hipError_t e = hipMemcpy(p->tab_dev, &T, sizeof T, hipMemcpyHostToDevice);
        if (e != hipSuccess) rc = fail(TFHE_E_HIP, "hipMemcpy: %s", hipGetErrorString(e));
    }
    if (rc) { tfhe_plain_plan_destroy(p); return rc; }
    *out = p;
    return TFHE_OK;
}

int tfhe_plain_plan_destroy(tfhe_plain_plan* p) {
    if (!p) return TFHE_OK;
    if (p->ctx && p->ctx->stream) hipStreamSynchronize(p->ctx->stream);  // no kernel of this plan still reads its tables
    for (void* d : p->allocs) hipFree(d);
    if (p->tab_dev) hipFree(p->tab_dev);
    delete p;
    return TFHE_OK;
}

int tfhe_plain_encode(tfhe_plain_plan* p, int scheme, const uint64_t* m, uint64_t* out, int64_t count) {
    int rc = plain_check(p, scheme, m, out, count);
    if (rc || count == 0) return rc;
    const u32 n = (u32)p->ctx->N;
    const int L = p->sel.n;
    const unsigned gx = (n + PLAIN_BS - 1) / PLAIN_BS;
    const int64_t chunk = chunk_of(p->ctx, count, PLAIN_MAX_GRID_Y);
    for (int64_t b0 = 0; b0 < count; b0 += chunk) {
        const int64_t nb = std::min(chunk, count - b0);
        rc = launch(p->ctx, k_plain_encode, dim3(gx, (unsigned)nb), dim3(PLAIN_BS), 0, m + (size_t)b0 * n, out + (size_t)b0 * L * n, p->tab_dev,
                    scheme == TFHE_PLAIN_BGV ? 1 : 0, n);
        if (rc) return rc;
    }
    return TFHE_OK;
}

int tfhe_plain_decode(tfhe_plain_plan* p, int scheme, const uint64_t* in, uint64_t* out, int64_t count) {
    int rc = plain_check(p, scheme, in, out, count);
    if (rc || count == 0) return rc;
    const u32 n = (u32)p->ctx->N;
    const int L = p->sel.n;
    const unsigned gx = (n + PLAIN_BS - 1) / PLAIN_BS;
    const int64_t chunk = chunk_of(p->ctx, count, PLAIN_MAX_GRID_Y);
    for (int64_t b0 = 0; b0 < count; b0 += chunk) {
        const int64_t nb = std::min(chunk, count - b0);
        const dim3 grid(gx, (unsigned)nb);
        const u64* src = in + (size_t)b0 * L * n;
        u64* dst = out + (size_t)b0 * n;
#define X(KM) rc = launch(p->ctx, scheme == TFHE_PLAIN_BGV ? k_plain_decode<KM, true> : k_plain_decode<KM, false>, grid, dim3(PLAIN_BS), 0, src, dst, p->tab_dev, n)
        PLAIN_KM_DISPATCH(p->km, X)
#undef X
        if (rc) return rc;
    }
    return TFHE_OK;
}

int tfhe_bfv_noise_max(tfhe_plain_plan* p, const uint64_t* in, uint64_t* out_words, int64_t count) {
    int rc = plain_check(p, TFHE_PLAIN_BFV, in, out_words, count);
    if (rc || count == 0) return rc;
    const u32 n = (u32)p->ctx->N;
    const int L = p->sel.n, nd = p->nd;
    const unsigned gx = (n + PLAIN_BS - 1) / PLAIN_BS;
    const u32 G = gx * PLAIN_WAVES;
    const size_t part_per_ct = (size_t)G * nd * 8;
    const int64_t chunk = chunk_of(p->ctx, count, PLAIN_MAX_GRID_Y, (size_t)64 << 20, part_per_ct);
    void* ws = nullptr;
    rc = ensure_ws(p->ctx, (size_t)chunk * part_per_ct, &ws);
    if (rc) return rc;
    u64* part = (u64*)ws;
    for (int64_t b0 = 0; b0 < count; b0 += chunk) {
        const int64_t nb = std::min(chunk, count - b0);
        const u64* src = in + (size_t)b0 * L * n;
        u64* dst = out_words + (size_t)b0 * nd;
#define X(KM)                                                                                                             \
    rc = launch(p->ctx, k_plain_noise_partial<KM>, dim3(gx, (unsigned)nb), dim3(PLAIN_BS), 0, src, part, p->tab_dev, n);   \
    if (!rc) rc = launch(p->ctx, k_plain_noise_reduce<KM>, dim3((unsigned)nb), dim3(PLAIN_BS), 0, part, dst, nd, G)
        PLAIN_KM_DISPATCH(p->km, X)
#undef X
        if (rc) return rc;
    }
    return TFHE_OK;
}

}  // extern "C"
