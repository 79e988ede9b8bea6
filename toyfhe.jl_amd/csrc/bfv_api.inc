// bfv_api.inc -- BFV plan (conversion tables) and the bfv_mul pipeline; included by toyfhe_hip.hip.

struct tfhe_bfv_plan {
    tfhe_ctx *small = nullptr, *big = nullptr;
    limb_sel_t sel_s, sel_b;
    u64 t = 0;
    bfv_tab_t tab;               // host copy (device pointers inside)
    bfv_tab_t* tab_dev = nullptr;
    std::vector<void*> allocs;
    int chunk = 256;
    void* ws = nullptr;
    size_t ws_bytes = 0;
    bool relin_ok = false;       // ℛ == limbs 0..ns-1 of the small ctx
    bfv_fast_tab_t* fast_dev = nullptr;  // register-resident fast path (superset mode, instantiated sizes)
    int fast_ns = 0, fast_np = 0;
    bool fast_narrow = false;  // all moduli below TFHE_FP_QMAX: the 26-bit-split / fp64 bodies (kernels specialised on it)
    bool use_fast = true;
    // narrow fast path: ℛbig's limb table with the contraction's per-limb input constants folded into the closing scaling of the
    // inverse transform (bfv_fold_kappa, bfv_tables.h).  Read by k_bfv_core_fused<.., OUTD> of this plan's multiplications only,
    // whose rows go to k_bfv_contract_fast<.., FOLDED>; the context's own table is never changed.
    ntt_limb_t* fold_dev = nullptr;
    hipEvent_t order_ev = nullptr;  // cross-stream ordering when ℛ and ℛbig live in contexts with different streams
};

namespace {

int upload(tfhe_bfv_plan* p, const std::vector<u64>& v, const u64** out) {
    void* d = nullptr;
    hipError_t e = devalloc::malloc_retry(&d, std::max<size_t>(8, v.size() * 8));
    if (e != hipSuccess) return fail(TFHE_E_HIP, "hipMalloc: %s", hipGetErrorString(e));
    p->allocs.push_back(d);
    e = hipMemcpy(d, v.data(), v.size() * 8, hipMemcpyHostToDevice);
    if (e != hipSuccess) return fail(TFHE_E_HIP, "hipMemcpy: %s", hipGetErrorString(e));
    *out = (const u64*)d;
    return TFHE_OK;
}

int upload_conv(tfhe_bfv_plan* p, const conv_host_t& H, conv_tab_t* T) {
    *T = H.tab;
    int rc = upload(p, H.C, &T->C);
    if (rc) return rc;
    rc = upload(p, H.M, &T->M);
    if (rc) return rc;
    return upload(p, H.Aw, &T->Aw);
}

// Work enqueued on `to`'s stream from here on runs after everything enqueued so far on `from`'s stream.  The contexts
// keep their own streams (a plan never re-points a context): the pipeline hops between them with one recorded event.
int stream_order(tfhe_bfv_plan* p, tfhe_ctx* from, tfhe_ctx* to) {
    if (from == to || from->stream == to->stream) return TFHE_OK;
    if (!p->order_ev) HIP_TRY(hipEventCreateWithFlags(&p->order_ev, hipEventDisableTiming));
    HIP_TRY(hipEventRecord(p->order_ev, from->stream));
    HIP_TRY(hipStreamWaitEvent(to->stream, p->order_ev, 0));
    return TFHE_OK;
}

int plan_ws(tfhe_bfv_plan* p, size_t bytes, void** out) {
    if (bytes > p->ws_bytes) {
        if (p->ws) {
            HIP_TRY(hipStreamSynchronize(p->big->stream));
            if (p->small->stream != p->big->stream) HIP_TRY(hipStreamSynchronize(p->small->stream));
            HIP_TRY(hipFree(p->ws));
            p->ws = nullptr; p->ws_bytes = 0;
        }
        hipError_t e = devalloc::malloc_retry(&p->ws, bytes);
        if (e != hipSuccess) return fail(TFHE_E_NOMEM, "BFV workspace hipMalloc(%zu) failed: %s", bytes, hipGetErrorString(e));
        p->ws_bytes = bytes;
    }
    *out = p->ws;
    return TFHE_OK;
}

// instantiated (NS, NP) pairs of the fast path
#define TFHE_FAST_PAIRS(X) X(8, 9) X(3, 4) X(2, 3) X(6, 7)
bool fast_has(int ns, int np) {
#define X(S, P_) if (ns == S && np == P_) return true;
    TFHE_FAST_PAIRS(X)
#undef X
    return false;
}
// lift_c2 (contraction of products, count = 3 * ciphertexts): c2 leaves as centred doubles for the fused key switch
// t_double (contraction, narrow bodies): the input rows are reduced doubles (k_bfv_core_fused<.., OUTD>)
// folded (with t_double): the rows also carry the per-limb input constants (k_bfv_core_fused run on the plan's folded limb table)
int launch_fast(tfhe_bfv_plan* p, bool contract, const u64* src, u64* dst, int64_t count, bool copy_shared = true, bool lift_c2 = false,
                bool t_double = false, bool folded = false) {
    const u32 n = (u32)p->big->N;
    const unsigned gx = (n + 255) / 256;
    const dim3 grid(gx * (unsigned)count);
    const bool lift3 = contract && lift_c2 && p->fast_narrow && count % 3 == 0;
    if ((t_double && !(contract && p->fast_narrow)) || (folded && !t_double)) return fail(TFHE_E_UNSUPPORTED, "internal: double-valued tensor rows need the narrow contraction");
    tfhe_ctx* const c = p->big;   // the conversions run on the stream of the big ring's context
#define X(S, P_)                                                                                                          \
    if (p->fast_ns == S && p->fast_np == P_) {                                                                            \
        if (!contract) {                                                                                                  \
            auto ek = p->fast_narrow ? k_bfv_expand_fast<S, P_, true> : k_bfv_expand_fast<S, P_, false>;                  \
            return launch(c, ek, grid, dim3(256), 0, src, dst, p->fast_dev, n, gx, copy_shared ? 1 : 0);                  \
        }                                                                                                                 \
        auto ck = lift3 && folded   ? k_bfv_contract_fast<S, P_, true, true, true, true>                                  \
                  : folded          ? k_bfv_contract_fast<S, P_, true, false, true, true>                                 \
                  : lift3 && t_double ? k_bfv_contract_fast<S, P_, true, true, true>                                      \
                  : t_double        ? k_bfv_contract_fast<S, P_, true, false, true>                                       \
                  : lift3           ? k_bfv_contract_fast<S, P_, true, true>                                              \
                  : p->fast_narrow  ? k_bfv_contract_fast<S, P_, true>                                                    \
                                    : k_bfv_contract_fast<S, P_, false>;                                                  \
        return launch(c, ck, grid, dim3(256), 0, src, dst, p->fast_dev, n, gx);                                           \
    }
    TFHE_FAST_PAIRS(X)
#undef X
    return TFHE_OK;
}

int launch_expand(tfhe_bfv_plan* p, const u64* src, u64* dst, int64_t count) {
    if (count == 0) return TFHE_OK;
    if (p->fast_dev && p->use_fast) return launch_fast(p, false, src, dst, count);
    const u32 n = (u32)p->big->N;
    const unsigned gx = (n + BFV_BS - 1) / BFV_BS;
    const size_t lds = (size_t)std::max(p->tab.nb, p->tab.ns) * BFV_BS * 8;
    return launch(p->big, k_bfv_expand, dim3(gx * (unsigned)count), dim3(BFV_BS), lds, src, dst, p->tab_dev, n, gx);
}
int launch_contract(tfhe_bfv_plan* p, const u64* src, u64* dst, int64_t count, bool lift_c2 = false, bool t_double = false, bool folded = false) {
    if (count == 0) return TFHE_OK;
    if (p->fast_dev && p->use_fast) return launch_fast(p, true, src, dst, count, true, lift_c2, t_double, folded);
    if (t_double) return fail(TFHE_E_UNSUPPORTED, "internal: double-valued tensor rows need the narrow contraction");
    if (lift_c2) return fail(TFHE_E_UNSUPPORTED, "internal: lifted output needs the narrow fast path");
    const u32 n = (u32)p->big->N;
    const unsigned gx = (n + BFV_BS - 1) / BFV_BS;
    const size_t lds = (size_t)(2 * p->tab.nb + p->tab.ns) * BFV_BS * 8;
    return launch(p->big, k_bfv_contract, dim3(gx * (unsigned)count), dim3(BFV_BS), lds, src, dst, p->tab_dev, n, gx);
}

// one chunk of c1*c2: c1,c2 [nct][2][ns][N] -> out3 [nct][3][ns][N]; E [nct][4][nb][N], T [nct][3][nb][N] scratch
int bfv_mul_chunk(tfhe_bfv_plan* p, const u64* c1, const u64* c2, u64* out3, int64_t nct, u64* E, u64* T, u64* scratch, bool lift_c2 = false) {
    const size_t N = (size_t)p->big->N;
    const int nb = p->tab.nb;
    u64* E1 = E;
    u64* E2 = E + (size_t)nct * 2 * nb * N;
    int rc;
    bool fused = false;  // transforms + tensor in one kernel (one scratch row per workgroup)
    bool t_double = false, folded = false;
    if (p->fast_dev && p->use_fast && bfv_core_fusable(p->big, p->sel_b)) {
        // the limbs ℛbig shares with ℛ are not copied by the expansion: the fused core reads them from the inputs
        core_alt_t alt{};
        alt.a = c1; alt.b = c2; alt.ns = p->tab.ns;
        for (int w = 0; w < nb; w++) alt.idx[w] = -1;
        for (int i = 0; i < p->tab.ns; i++) alt.idx[p->tab.pos_s[i]] = (signed char)i;
        rc = launch_fast(p, false, c1, E1, nct * 2, false);
        if (!rc) rc = launch_fast(p, false, c2, E2, nct * 2, false);
        if (rc) return rc;
        t_double = p->fast_narrow;   // the narrow contraction takes the tensor rows as reduced doubles (6 instructions fewer per word)
        // ... and, through the plan's limb table, already multiplied by the contraction's per-limb input constants
        folded = t_double && p->fold_dev != nullptr;
        rc = launch_bfv_core_fused(p->big, E1, E2, T, scratch, nct, p->sel_b, &fused, &alt, t_double, folded ? p->fold_dev : nullptr);
        if (rc) return rc;
        if (!fused) t_double = folded = false;   // (nothing was launched: the unfused route below runs on the context's table)
    } else {
        rc = launch_expand(p, c1, E1, nct * 2);            // mul_expand, bfv.jl:34
        if (rc) return rc;
        rc = launch_expand(p, c2, E2, nct * 2);
        if (rc) return rc;
        rc = launch_bfv_core_fused(p->big, E1, E2, T, scratch, nct, p->sel_b, &fused);
        if (rc) return rc;
    }
    if (!fused) {
        rc = run_ntt(p->big, false, E, E, nct * 4 * nb, p->sel_b);
        if (rc) return rc;
        rc = launch(p->big, k_tensor, row_grid((unsigned)(nct * nb), (size_t)N), dim3(256), 0, E1, E2, T, p->big->limbs_dev, p->sel_b, (u32)N);  // rlwe_she.jl:255-258
        if (rc) return rc;
        rc = run_ntt(p->big, true, T, T, nct * 3 * nb, p->sel_b);
        if (rc) return rc;
    }
    return launch_contract(p, T, out3, nct * 3, lift_c2, t_double, folded);  // mul_contract, bfv.jl:35-40 (c2 as centred doubles when relinearised next)
}

}  // namespace

extern "C" {

int tfhe_bfv_plan_create(tfhe_ctx* small, const int32_t* idx_s, int ns, tfhe_ctx* big, const int32_t* idx_b, int nb, uint64_t t,
                         tfhe_bfv_plan** out) {
    if (!small || !big || !out) return fail(TFHE_E_BADARG, "null argument");
    *out = nullptr;
    if (small->N != big->N) return fail(TFHE_E_PARAMS_MISMATCH, "ℛ and ℛbig have different degree");
    if (t < 2) return fail(TFHE_E_BADARG, "plaintext modulus must be >= 2");
    tfhe_bfv_plan* p = new tfhe_bfv_plan();
    p->small = small; p->big = big; p->t = t;
    int rc = make_sel(small, ns, idx_s, &p->sel_s);
    if (!rc) rc = make_sel(big, nb, idx_b, &p->sel_b);
    if (rc) { delete p; return rc; }
    std::vector<u64> qs(ns), pb(nb);
    for (int i = 0; i < ns; i++) qs[i] = small->q[p->sel_s.idx[i]];
    for (int j = 0; j < nb; j++) pb[j] = big->q[p->sel_b.idx[j]];
    p->relin_ok = true;
    for (int i = 0; i < ns; i++) if (p->sel_s.idx[i] != i) p->relin_ok = false;
    bfv_host_t* H = new bfv_host_t();
    std::string err;
    rc = build_bfv_host(qs, pb, t, H, &err);
    if (rc) { delete H; tfhe_bfv_plan_destroy(p); return fail(rc, "%s", err.c_str()); }
    bfv_tab_t& B = p->tab;
    B = H->tab;
    rc = upload_conv(p, H->E, &B.E);
    if (!rc) rc = upload_conv(p, H->C1, &B.C1);
    if (!rc) rc = upload_conv(p, H->C2, &B.C2);
    delete H;
    if (rc) { tfhe_bfv_plan_destroy(p); return rc; }
    if (B.mode == 0) {  // register-resident fast path when this (ns, np) is instantiated
        bfv_fast_host_t* F = new bfv_fast_host_t();
        if (build_bfv_fast_host(qs, pb, t, F) && fast_has(F->tab.ns, F->tab.np)) {
            bfv_fast_tab_t T = F->tab;
            rc = upload(p, F->Mq, &T.Mq);
            if (!rc) rc = upload(p, F->Aq, &T.Aq);
            if (!rc) rc = upload(p, F->Mp, &T.Mp);
            if (!rc) rc = upload(p, F->Ap, &T.Ap);
            if (!rc && devalloc::malloc_retry(&p->fast_dev, sizeof(bfv_fast_tab_t)) != hipSuccess) rc = fail(TFHE_E_HIP, "hipMalloc failed");
            if (!rc) {
                hipMemcpy(p->fast_dev, &T, sizeof T, hipMemcpyHostToDevice);
                p->fast_ns = T.ns; p->fast_np = T.np; p->fast_narrow = T.narrow != 0;
            }
            if (!rc && p->fast_narrow) {
                std::vector<ntt_limb_t> LT = big->limbs_host;   // (device pointers inside: the transform tables are the context's)
                u64 kappa[TFHE_FAST_MAX * 2];
                bfv_fold_kappa(T, kappa);
                for (int l = 0; l < nb; l++) bfv_fold_limb(&LT[p->sel_b.idx[l]], kappa[l]);
                if (devalloc::malloc_retry(&p->fold_dev, LT.size() * sizeof(ntt_limb_t)) != hipSuccess) rc = fail(TFHE_E_HIP, "hipMalloc failed");
                else hipMemcpy(p->fold_dev, LT.data(), LT.size() * sizeof(ntt_limb_t), hipMemcpyHostToDevice);
            }
        }
        delete F;
        if (rc) { tfhe_bfv_plan_destroy(p); return rc; }
    }
    if (devalloc::malloc_retry(&p->tab_dev, sizeof(bfv_tab_t)) != hipSuccess) { tfhe_bfv_plan_destroy(p); return fail(TFHE_E_HIP, "hipMalloc failed"); }
    hipMemcpy(p->tab_dev, &B, sizeof(bfv_tab_t), hipMemcpyHostToDevice);
    *out = p;
    return TFHE_OK;
}

int tfhe_bfv_plan_destroy(tfhe_bfv_plan* p) {
    if (!p) return TFHE_OK;
    // main_stream and the side lane, as tfhe_ctx_destroy does: ctx->stream is the side lane while another thread is inside a forked
    // call on that context (lanes_t), and the plan's own kernels were enqueued on main_stream
    auto drain = [](tfhe_ctx* c) {
        if (c->main_stream) hipStreamSynchronize(c->main_stream);
        if (c->side_stream) hipStreamSynchronize(c->side_stream);
    };
    if (p->big) drain(p->big);
    if (p->small && p->small != p->big) drain(p->small);
    if (p->order_ev) hipEventDestroy(p->order_ev);
    for (void* d : p->allocs) hipFree(d);
    if (p->tab_dev) hipFree(p->tab_dev);
    if (p->fast_dev) hipFree(p->fast_dev);
    if (p->fold_dev) hipFree(p->fold_dev);
    if (p->ws) hipFree(p->ws);
    delete p;
    return TFHE_OK;
}

int tfhe_bfv_plan_set_chunk(tfhe_bfv_plan* p, int chunk) {
    if (!p || chunk < 0) return fail(TFHE_E_BADARG, "bad argument");
    p->chunk = chunk ? chunk : 256;
    return TFHE_OK;
}

int tfhe_bfv_plan_workspace(const tfhe_bfv_plan* p, void** ptr, size_t* bytes) {
    if (!p || !ptr || !bytes) return fail(TFHE_E_BADARG, "null argument");
    *ptr = p->ws;
    *bytes = p->ws_bytes;
    return TFHE_OK;
}

int tfhe_bfv_plan_set_variant(tfhe_bfv_plan* p, int variant) {
    if (!p || variant < 0 || variant > 1) return fail(TFHE_E_BADARG, "variant must be 0 (auto) or 1 (general kernels)");
    p->use_fast = (variant == 0);
    return TFHE_OK;
}

// The conversions run on ℛbig's stream; callers order their work on ℛ's stream (the plan's "front" stream), so every
// entry point waits for ℛ's stream on the way in and makes ℛ's stream wait for the result on the way out.
int tfhe_bfv_expand(tfhe_bfv_plan* p, const uint64_t* src, uint64_t* dst, int64_t count) {
    if (!p || !src || !dst || count < 0) return fail(TFHE_E_BADARG, "bad argument");
    int rc = stream_order(p, p->small, p->big);
    if (!rc) rc = launch_expand(p, src, dst, count);
    if (!rc) rc = stream_order(p, p->big, p->small);
    return rc;
}
int tfhe_bfv_contract(tfhe_bfv_plan* p, const uint64_t* src, uint64_t* dst, int64_t count) {
    if (!p || !src || !dst || count < 0) return fail(TFHE_E_BADARG, "bad argument");
    int rc = stream_order(p, p->small, p->big);
    if (!rc) rc = launch_contract(p, src, dst, count);
    if (!rc) rc = stream_order(p, p->big, p->small);
    return rc;
}

static int bfv_mul_impl(tfhe_bfv_plan* p, const u64* evk, int n_digits, const u64* c1, const u64* c2, u64* out, int64_t batch) {
    if (!p || !c1 || !c2 || !out || batch < 0) return fail(TFHE_E_BADARG, "bad argument");
    const size_t N = (size_t)p->big->N;
    const int ns = p->tab.ns, nb = p->tab.nb;
    const bool relin = evk != nullptr;
    if (relin) {
        if (!p->relin_ok) return fail(TFHE_E_UNSUPPORTED, "relinearisation needs ℛ = limbs 0..ns-1 of the small context");
        if (n_digits < ns) return fail(TFHE_E_PARAMS_MISMATCH, "evaluation key has %d components, need %d", n_digits, ns);
    }
    const int64_t chunk = std::max<int64_t>(1, std::min<int64_t>(batch, p->chunk));
    // c2 goes from the contraction straight into the fused key switch: hand it over as centred doubles (the digit lift)
    const bool prelift = relin && p->fast_dev && p->use_fast && p->fast_narrow && ks_prelift_ok(p->small, ns);
    const size_t ntt_tmp = p->big->logN > 14 ? (size_t)chunk * 4 * nb * N * 8 : 0;  // run_ntt's own scratch lives in the ctx
    (void)ntt_tmp;
    void* ws = nullptr;
    const size_t scr_rows = (size_t)2 * std::max(256, p->big->num_cus);  // k_bfv_core_fused: one scratch row per workgroup (up to two per CU below 2^14)
    int rc = plan_ws(p, ((size_t)chunk * (7 * (size_t)nb + (relin ? 3 * (size_t)ns : 0)) + scr_rows) * N * 8, &ws);
    if (rc) return rc;
    u64* E = (u64*)ws;
    u64* T = E + (size_t)chunk * 4 * nb * N;
    u64* R = T + (size_t)chunk * 3 * nb * N;
    u64* SCR = R + (relin ? (size_t)chunk * 3 * ns * N : 0);
    // keyswitch(evk, c) on ℛ with RNS digits, rlwe_she.jl:315-347 (relin_window == 0).  The key is an argument of the call: it is
    // prepared (converted to doubles on the fused paths) once, for the largest chunk, and every chunk runs on that preparation --
    // where ℛ's context workspace, which holds the prepared key, is nobody else's between the chunks.  The plan's own workspace
    // (plan_ws) shares nothing with it; what does take it is a stand-alone transform of N > 2^14 (run_ntt_large) in
    // bfv_mul_chunk's unfused route when ℛbig lives in ℛ's context: there every chunk prepares for itself, as before.
    const bool key_once = p->small != p->big || p->big->logN <= 14;
    ks_prepared_t K;
    if (relin && key_once && batch > 0) {
        rc = ks_prepare(p->small, ns, ns, 0, evk, R, 3, out, chunk, 0, false, prelift, false, &K);
        if (rc) return rc;
    }
    for (int64_t b0 = 0; b0 < batch; b0 += chunk) {
        const int64_t nct = std::min(chunk, batch - b0);
        const u64* a = c1 + (size_t)b0 * 2 * ns * N;
        const u64* b = c2 + (size_t)b0 * 2 * ns * N;
        rc = stream_order(p, p->small, p->big);   // inputs (and the previous chunk's key switch, which reads R) are ℛ-stream work
        if (rc) return rc;
        if (!relin) {
            rc = bfv_mul_chunk(p, a, b, out + (size_t)b0 * 3 * ns * N, nct, E, T, SCR);
            if (rc) return rc;
        } else {
            rc = bfv_mul_chunk(p, a, b, R, nct, E, T, SCR, prelift);
            if (!rc) rc = stream_order(p, p->big, p->small);
            if (rc) return rc;
            u64* const o = out + (size_t)b0 * 2 * ns * N;
            if (!key_once) rc = ks_prepare(p->small, ns, ns, 0, evk, R, 3, o, nct, 0, false, prelift, false, &K);
            if (!rc) rc = ks_run(p->small, K, R, o, nct);
            if (rc) return rc;
        }
    }
    return relin ? TFHE_OK : stream_order(p, p->big, p->small);   // the result is ordered on ℛ's stream either way
}

int tfhe_bfv_mul(tfhe_bfv_plan* p, const uint64_t* c1, const uint64_t* c2, uint64_t* out, int64_t batch) {
    return bfv_mul_impl(p, nullptr, 0, c1, c2, out, batch);
}
int tfhe_bfv_mul_relin(tfhe_bfv_plan* p, const uint64_t* evk, int n_digits, const uint64_t* c1, const uint64_t* c2, uint64_t* out, int64_t batch) {
    if (!evk) return fail(TFHE_E_BADARG, "null evaluation key");
    return bfv_mul_impl(p, evk, n_digits, c1, c2, out, batch);
}

}  // extern "C"
