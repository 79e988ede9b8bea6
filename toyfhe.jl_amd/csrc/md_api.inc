// md_api.inc -- the diagonal matrix products tfhe_matmul_diag, tfhe_matmul_bsgs and tfhe_matmul_bsgs_blocks, the rotate-and-sum fold
// tfhe_rotate_sum and the rectangular product tfhe_matmul_bsgs_fold: the shared rotation phase (md_plan, md_bufs, md_rotations), its
// workspace, the fold (md_fold_plan, md_fold_run) and the five entry points; included by toyfhe_hip.hip after ks_api.inc, whose key-sum, digit and
// rotation helpers (ks_digits_fwd, ks_inner_launch, keyswitch_impl, ks_rot_prepared_bytes) it calls.  Kernels: kernels.h k_md_*.
// At the end: the same rotation phase on grouped-digit keys (mdg_plan, mdg_bufs, mdg_rotations; kernels ks_group_core.h k_mdg_*) with its
// entry points tfhe_matmul_diag_grouped and tfhe_matmul_bsgs_grouped, and the fold on such keys (mdg_fold_plan, mdg_fold_run; kernels
// k_mdg_fold_gather, k_mdg_fold_finish) with tfhe_rotate_sum_grouped and tfhe_matmul_bsgs_fold_grouped, on the hoisting helpers of ks_api.inc (ksg_*).

// tfhe_matmul_diag, evaluation-domain form: U[grp][j] = NTT_j( [P[grp]] mod q_j ) (x P^-1 unless *scaled comes back false) for
// the `groups` special-limb rows P (coefficient domain, canonical) and the limbs j of `sl`.  At N = 2^16 the lift rides on the
// forward transforms' loads (ntt_io_t::lift_unsigned: k_ntt_fwd_quad for the fp64-size limbs, k_ntt_fwd_top_lift + the u64 block
// kernels for the others) and the factor P^-1 is left to k_md_acc; otherwise k_md_lift writes the scaled lifts to `LF` and plain
// transforms follow.
// Whether the unsigned lift can ride on the forward transforms' loads (ntt_io_t::lift_unsigned) for these target limbs and this
// special prime: N = 2^15 / 2^16 through the pair / quad kernels (+ top-stage lift for the u64 limbs); N <= 2^14 through
// run_ntt's digit-lift mode -- except when every target limb is fp64-size and the special prime is not (the uniform fp64 policy
// reads its source as one double).
static bool md_lift_is_fused(const tfhe_ctx* c, const ks_arg_t& A, const limb_sel_t& sl) {
    const int level = A.level;
    if (level > 32 || c->logN > 16) return false;
    if (c->logN >= 15) return c->variant == 0;
    const bool special_fp = c->limbs_host[A.w.idx[level]].Wd != nullptr;
    return special_fp || !sel_fp(c, sl, 0);
}
static int md_lift_fwd(tfhe_ctx* c, const ks_arg_t& A, const limb_sel_t& sl, const rescale_arg_t& ra, const u64* P, u64* LF, u64* U,
                       int64_t groups, bool* scaled) {
    const int level = A.level;
    const u32 n = (u32)c->N;
    const int64_t rows = groups * level;
    if (LF == nullptr) {   // the caller sized the workspace for the fused form (md_lift_is_fused)
        ntt_io_t io = io_plain();
        io.mode = 1; io.level = 1; io.nw = (u32)level; io.polys = 1; io.lift_unsigned = 1;
        *scaled = false;
        if (c->logN <= 14) return run_ntt(c, false, P, U, rows, sl, &io);
        const int x = c->logN - 14;
        const policy_split_t ps = policy_split(c, sl);
        const u32 tmask = ps.fpmask, tall = ps.all;   // fp64-size target limbs
        const bool special_fp = c->limbs_host[A.w.idx[level]].Wd != nullptr;
        if ((rows << x) > 0x7fffffffll || (((uintptr_t)P | (uintptr_t)U) & 15u) != 0) return fail(TFHE_E_BADARG, "md_lift_fwd: row count / alignment");
        int rc;
        void* tmp = nullptr;
        if (tmask != tall) {   // (before the fork: growing the workspace synchronises)
            rc = ws_scratch(c, (size_t)rows * c->N * 8, &tmp);
            if (rc) return rc;
        }
        lanes_t lanes(c, tmask != 0 && tmask != tall);   // both kinds of limbs: side by side
        if (tmask) {   // the fp64-size limbs: one kernel per row (pair) (ArithFpWide reads a source above 2^52 in two halves)
            ntt_io_t a = io;
            a.limb_mask = tmask == tall ? 0u : tmask;
            lanes.use(1);
            rc = run_ntt_large(c, false, P, U, rows, sl, a, &a, true, !special_fp);
            if (rc) return rc;
            lanes.use(0);
        }
        if (tmask != tall) {   // the larger limbs: lift fused into the top stages (into the transform scratch), then the u64 block kernels
            ntt_io_t w = io;
            w.limb_mask = tmask ? (tall & ~tmask) : 0u;
            rc = launch_top_lift(c, P, (u64*)tmp, rows, sl, w);
            if (rc) return rc;
            ntt_io_t ib = io_plain();
            ib.limb_mask = w.limb_mask;
            rc = launch_block_fwd<ArithInt, 14>(c, (const u64*)tmp, U, rows, sl, x, ib);
            if (rc) return rc;
        }
        return TFHE_OK;
    }
    const int rc = launch(c, k_md_lift, row_grid((unsigned)rows, (size_t)c->N), dim3(256), 0, P, LF, c->limbs_dev, sl, ra, n);
    if (rc) return rc;
    *scaled = true;
    return run_ntt(c, false, LF, U, rows, sl);
}

// the bound on the per-call workspace of the diagonal products (tfhe_matmul_diag, tfhe_matmul_bsgs)
static size_t md_ws_cap(const tfhe_ctx* c) {
    // The keys of all R rotations are read once per chunk (2.8 GB at N = 2^16, 6 limbs + special prime, 63 rotations): a chunk as
    // large as the memory allows (32 GiB of workspace unless TFHE_MD_WS_GIB says otherwise; halved while the allocation fails)
    static const size_t ws_cap_env = env_gib("TFHE_MD_WS_GIB", 32);
    // ... and never more than half of what the device has free right now (counting what this context and the allocator's cache
    // already hold, both of which the allocation below can reuse): other contexts, BFV plans and processes keep their room
    size_t ws_cap = ws_cap_env;
    {
        // (hipMemGetInfo is a driver round trip -- milliseconds in a process with many allocations -- and this call sits in the
        // launch path of a host-bound circuit: the reading is kept for two seconds)
        // (r05, ADVICE r04: the reading and the allocator's cached bytes are those of THIS context's device -- a process driving
        // several GPUs computed the cap from whichever device had asked last and from the cache summed over all of them)
        struct mi_t { size_t free_bytes = 0; std::chrono::steady_clock::time_point at{}; };
        static std::mutex mi_mu;
        static std::map<int, mi_t> mi_dev;
        size_t fr = 0, tot = 0;
        bool have = false;
        const int cur_dev = devalloc::current_device();          // what hipMemGetInfo reads and where the workspace will be allocated
        {
            std::lock_guard<std::mutex> g(mi_mu);
            mi_t& mi = mi_dev[cur_dev];
            const auto now = std::chrono::steady_clock::now();
            if (mi.free_bytes && now - mi.at < std::chrono::seconds(2)) { fr = mi.free_bytes; have = true; }
            else if (hipMemGetInfo(&fr, &tot) == hipSuccess) { mi.free_bytes = fr; mi.at = now; have = true; }
            else (void)hipGetLastError();
        }
        if (have) {
            size_t cached = 0;
            {
                devalloc::state_t& as = devalloc::S();
                std::lock_guard<std::mutex> g(as.mu);
                auto it = as.devs.find(cur_dev);
                if (it != as.devs.end()) cached = it->second.cached_bytes;
            }
            ws_cap = std::min(ws_cap, std::max<size_t>((fr + c->ws_bytes + cached) / 2, (size_t)1 << 30));
        }
    }
    return ws_cap;
}

// The workspace of one call by its layout: the largest chunk of the batch that md_ws_cap admits, halved while the allocation
// fails; the layout is in force from the allocation until this object goes.
struct md_ws_t {
    ws_borrow_t borrow;   // a workspace above ws_keep_bytes() is this call's: back to the allocator on every return path
    const ws_layout_t& L;
    int rc = TFHE_OK;
    int64_t chunk;
    void* ws = nullptr;
    ws_scope_t scope;
    md_ws_t(tfhe_ctx* c, int64_t batch, const ws_layout_t& layout)
        : borrow(c), L(layout), chunk(chunk_of(c, batch, 512, md_ws_cap(c), layout.per_ct_bytes())) {
        for (bool first_try = true;; first_try = false) {
            const size_t need = L.bytes(chunk);
            if (first_try && need > ws_keep_bytes() && need > c->ws_bytes) borrow.begin();
            rc = ensure_ws(c, need, &ws, borrow.active);
            if (rc != TFHE_E_NOMEM || chunk == 1) break;
            chunk = (chunk + 1) / 2;
        }
        if (!rc) scope.set(c->ws_scratch, L.region0(chunk));
    }
    u64* at(ws_region_t h) const { return L.at(ws, chunk, h); }
    ws_span_t region0() const { return ws_span_t{ws, L.region0(chunk)}; }   // what a nested user is handed
};

// The rotation phase of a diagonal product -- everything up to the accumulation -- is shared by tfhe_matmul_diag and
// tfhe_matmul_bsgs: what it consists of is decided once per call (md_plan), its buffers are laid out per chunk (md_bufs), and
// md_rotations runs it over one chunk.
struct md_plan_t {
    ks_arg_t A; limb_sel_t sl; rescale_arg_t ra; rot_tail_arg_t G;
    int Lk, level, nw, R;
    // With a special prime the rotations are finished in the evaluation domain (k_md_*: only the special limb of every key sum is
    // inverse-transformed); TFHE_MD_COEFF=1 keeps the coefficient-domain tail (k_ks_rot_tail) for comparisons.
    bool eval_form;
    bool need_lf;        // the untransformed lifts: only where the lift is not fused into the transforms' loads
    // The phase's rows of a chunk, from wherever the caller puts them (no region 0 of its own): digits (level nw rows per ciphertext),
    // S / T (R 2 nw), ROT: rotated ciphertexts (R 2 level), X: the ciphertext's own transform (2 level); evaluation-domain form: LF, the
    // lifted special limbs before their transforms (R 2 level, where the lift is not fused), and PB, the special limbs themselves (R 2)
    ws_layout_t L;
    ws_region_t dig, S, ROT, X, LF, PB;
    size_t ntt_rows;     // rows of the largest stand-alone transform, per ciphertext
};
static md_plan_t md_plan(const tfhe_ctx* c, int Lk, int level, int special, const uint64_t* galois, int R) {
    md_plan_t P{};
    const int nw = special ? level + 1 : level;
    P.Lk = Lk; P.level = level; P.nw = nw; P.R = R;
    P.A = make_ks_arg(Lk, level, special, 2);
    P.sl = first_limbs(level);
    if (special) {
        special_inv_table(c, Lk, level, P.ra.qlinv);
        std::copy(P.ra.qlinv, P.ra.qlinv + level, P.A.pinv);
    }
    for (int r = 0; r < R; r++) P.G.g[r] = galois[r];
    static const bool md_coeff = env_flag("TFHE_MD_COEFF", false);
    P.eval_form = special && R > 0 && !md_coeff;
    P.need_lf = P.eval_form && !(md_lift_is_fused(c, P.A, P.sl) && (size_t)R * 2 * level * 4 * 512 <= 0x7fffffffull);
    P.L = ws_layout_t((size_t)c->N);
    P.dig = P.L.rows((size_t)level * nw); P.S = P.L.rows((size_t)R * 2 * nw); P.ROT = P.L.rows((size_t)R * 2 * level);
    P.X = P.L.rows((size_t)2 * level); P.LF = P.L.rows(P.need_lf ? (size_t)R * 2 * level : 0); P.PB = P.L.rows(P.eval_form ? (size_t)R * 2 : 0);
    P.ntt_rows = std::max<size_t>({(size_t)level * nw, (size_t)R * 2 * nw, (size_t)2 * level});
    return P;
}
// ROT: the transformed rotated ciphertexts [R][nb][2][level][N], in the evaluation-domain form the lifts U of the same shape
struct md_bufs_t { u64 *dig, *S, *ROT, *X, *LF, *PB; };
static md_bufs_t md_bufs(const md_plan_t& P, u64* base, int64_t chunk) {
    const auto at = [&](ws_region_t h) { return P.L.at(base, chunk, h); };
    return md_bufs_t{at(P.dig), at(P.S), at(P.ROT), at(P.X),
                     P.need_lf ? at(P.LF) : nullptr,   // lifted special limbs, untransformed (same shape as U)
                     at(P.PB)};                        // [R][nb][2][N]
}
// The coefficient tail of the rotation phase (no special prime, or TFHE_MD_COEFF=1; R >= 1): ROT = rotate(gk_r, cin) for every r, in the
// COEFFICIENT domain, [R][nb][2][level][N] -- where the products transform them next (md_rotations) and the fold adds them as they are
static int md_rotations_coeff(tfhe_ctx* c, const md_plan_t& P, const uint64_t* const* evks, const u64* cin, int64_t nb, const md_bufs_t& B) {
    const int R = P.R;
    int rc = ks_digits_fwd(c, P.A, cin, B.dig, nb);
    if (rc) return rc;
    rc = ks_inner_launch(c, P.A, P.Lk, nullptr, B.dig, B.S, nb, evks, R);   // key sums of the unrotated digits against every prepared key
    if (rc) return rc;
    rc = run_ntt(c, true, B.S, B.S, (int64_t)R * nb * 2 * P.nw, P.A.w);
    if (rc) return rc;
    return launch(c, k_ks_rot_tail, dim3(8 * TFHE_ROT_TAIL_SLOTS), dim3(256), 0, B.S, cin, B.ROT, c->limbs_dev, P.A, P.ra, P.G, (u32)c->N, (u32)nb,
                  (u32)((int64_t)R * nb * 2));
}
// X = NTT(cin) and, per rotation r: evaluation-domain form -- V in S (k_ks_inner<.., EPI>) and the lifts U in ROT, *scaled telling
// whether U carries the factor P^-1 already (md_lift_fwd); otherwise NTT(rotate(gk_r, cin)) in ROT
static int md_rotations(tfhe_ctx* c, const md_plan_t& P, const uint64_t* const* evks, const u64* cin, int64_t nb, const md_bufs_t& B, bool* scaled) {
    const int Lk = P.Lk, level = P.level, nw = P.nw, R = P.R;
    const u32 n = (u32)c->N;
    int rc;
    if (P.eval_form) {
        const u32 groups = (u32)((int64_t)R * nb * 2);
        rc = run_ntt(c, false, cin, B.X, nb * 2 * level, P.sl);
        if (rc) return rc;
        rc = ks_digits_fwd(c, P.A, cin, B.dig, nb);
        if (rc) return rc;
        rc = ks_inner_launch(c, P.A, Lk, nullptr, B.dig, B.S, nb, evks, R, B.X);   // limbs j < level leave as V = S' P^-1 + X0 [s = 0]
        if (rc) return rc;
        rc = launch(c, k_md_special_perm, dim3(8 * TFHE_ROT_TAIL_SLOTS), dim3(256), 0, B.S, B.PB, P.G, n, (u32)nw, (u32)level, (u32)nb, groups);
        if (rc) return rc;
        limb_sel_t sp{};
        sp.n = 1;
        sp.idx[0] = Lk - 1;
        rc = run_ntt(c, true, B.PB, B.PB, (int64_t)groups, sp);
        if (rc) return rc;
        return md_lift_fwd(c, P.A, P.sl, P.ra, B.PB, B.LF, B.ROT, (int64_t)groups, scaled);
    }
    if (R) {
        rc = md_rotations_coeff(c, P, evks, cin, nb, B);
        if (rc) return rc;
        rc = run_ntt(c, false, B.ROT, B.ROT, (int64_t)R * nb * 2 * level, P.sl);
        if (rc) return rc;
    }
    return run_ntt(c, false, cin, B.X, nb * 2 * level, P.sl);
}

// ---- diagonal matrix-vector product (infer.jl:140-149, test/ckks_matmul.jl:33-41) in one call ---------------------------
// out = diag_0 (.) c + sum_r diag_{r+1} (.) rotate(gk_r, c): the hoisted rotations of tfhe_rotate_many (one digit decomposition
// of c) with every step -- key sums, inverse transforms, automorphism + tail, forward transforms, accumulation -- run over ALL
// rotations at once instead of rotation by rotation (R x more rows per launch: about 15 launches per product instead of
// about 8 R + 2 R + 2), and the rotated ciphertexts never return to the caller.  Same arithmetic, term by term, as
// rotate_many -> nntt -> dot: bit-identical results.
int tfhe_matmul_diag(tfhe_ctx* c, int Lk, int level, int special, const uint64_t* const* evks, int n_digits, const uint64_t* galois,
                     int n_rot, const uint64_t* diags, const uint64_t* ct, uint64_t* out, int64_t batch) {
    if (!evks || !galois || !diags || n_rot < 0) return fail(TFHE_E_BADARG, "null argument");
    if (n_rot > TFHE_DOT_MAX) return fail(TFHE_E_UNSUPPORTED, "tfhe_matmul_diag takes at most %d rotations per call", TFHE_DOT_MAX);
    for (int r = 0; r < n_rot; r++) {
        int rc = ks_check(c, Lk, level, special, evks[r], n_digits, ct, 2, out, batch);
        if (!rc) rc = galois_check(c, galois[r]);
        if (rc) return rc;
    }
    if (n_rot == 0) {
        int rc = ks_check(c, Lk, level, special, diags, n_digits, ct, 2, out, batch);
        if (rc) return rc;
    }
    if (batch == 0) return TFHE_OK;
    const size_t N = (size_t)c->N;
    const md_plan_t P = md_plan(c, Lk, level, special, galois, n_rot);
    // workspace: [ region 0: transform scratch | the rotation phase (md_bufs) ]
    ws_layout_t L(N);
    L.scratch(P.ntt_rows);
    const ws_region_t phase = L.rows(P.L.rows_per_ct());
    const md_ws_t W(c, batch, L);
    if (W.rc) return W.rc;
    const int64_t chunk = W.chunk;
    const md_bufs_t B = md_bufs(P, W.at(phase), chunk);
    for (int64_t b0 = 0; b0 < batch; b0 += chunk) {
        const int64_t nb = std::min(chunk, batch - b0);
        bool scaled = true;
        int rc = md_rotations(c, P, evks, ct + (size_t)b0 * 2 * level * N, nb, B, &scaled);
        if (rc) return rc;
        u64* const o = out + (size_t)b0 * 2 * level * N;   // one sum (ngiant1 = 1), written where it belongs
        if (P.eval_form) {
            auto acc = scaled ? k_md_acc<false, 1> : k_md_acc<true, 1>;
            rc = launch(c, acc, dim3(8 * TFHE_MD_SLOTS), dim3(256), 0, B.X, B.S, B.ROT, diags, o, c->limbs_dev, P.sl, P.G, P.ra, (u32)N, (u32)P.nw,
                        (u32)P.R, (u32)nb, 1u);
        } else {
            rc = launch(c, k_md_acc_dense<1>, row_grid((unsigned)(nb * 2 * level), N), dim3(256), 0, B.X, B.ROT, diags, o, c->limbs_dev, P.sl,
                        (u32)N, (u32)P.R, (u32)(nb * 2 * level), 1u);
        }
        if (rc) return rc;
    }
    return TFHE_OK;
}

// ---- the same product by baby and giant steps ------------------------------------------------------------------------------
// With the rotation index written k = j n1 + i,  sum_k d_k (.) rho^k(x) = sum_j rho^(j n1)( sum_i rho^(-j n1)(d_k) (.) rho^i(x) ):
// n_baby + n_giant keys and key sums instead of one per diagonal; the plaintext diagonals arrive pre-rotated.
//     inner_j = sum_{i = 0 .. n_baby} diags[j][i] (.) NTT(r_i(ct))       (r_0 = identity, r_i = rotate(baby key i - 1, .))
//     out     = INTT(inner_0) + sum_{j = 1 .. n_giant} rotate(giant key j - 1, INTT(inner_j))
// The baby phase is tfhe_matmul_diag's up to its accumulation (md_rotations); the accumulations with n_giant + 1 outputs are
// k_md_acc / k_md_acc_dense, tiled; one batched inverse transform covers all inner sums; the giant rotations go through the
// prepared-key key switch (keyswitch_impl), one per giant step over the chunk; k_bsgs_sum adds up.  Exact arithmetic on canonical
// residues throughout: the words of tfhe_rotate_many -> tfhe_nntt -> tfhe_dot -> tfhe_inntt -> tfhe_rotate_prepared -> tfhe_add.
// ---- the rotate-and-sum fold ---------------------------------------------------------------------------------------------------
// F_0 = the input;  F_{t+1} = F_t + sum_{u < sizes[t]} rotate(key_{t,u}, F_t): log2(n / m) steps of it add up the n / m partial sums a
// product by m extended diagonals leaves (tfhe_matmul_bsgs_fold), and by itself it is the sum of slots (tfhe_rotate_sum).  One step over
// a chunk is the rotation phase of a diagonal product over the group's keys (md_rotations) followed by
//   with a special prime   k_md_fold (the value and its rotations added in the evaluation domain) and ONE inverse transform of the
//                          sum, 2 level rows per ciphertext instead of 2 level per rotation;
//   without one            k_bsgs_sum over the rows k_ks_rot_tail left in the coefficient domain (md_rotations_coeff): no transform.
// Every group goes this way, a group of one included: its other route, the giant steps' prepared-key key switch followed by k_bsgs_sum,
// is the same key sums and tail plus a pass over the ciphertext, and has not been measured against this one.
// Exact arithmetic on canonical residues: the words of tfhe_rotate_many(prepared) over the group's keys -> tfhe_add, group by group.
struct md_fold_t {
    const uint64_t* const* evks;   // all groups back to back
    const uint64_t* galois;
    const int* sizes;
    int n_groups;
    std::vector<md_plan_t> plans;  // one per group
    size_t rows = 0, ntt_rows = 0; // the largest group's (md_plan_t)
};
static md_fold_t md_fold_plan(const tfhe_ctx* c, int Lk, int level, int special, const uint64_t* const* evks, const uint64_t* galois,
                              const int* sizes, int n_groups) {
    md_fold_t F{evks, galois, sizes, n_groups, {}, 0, 0};
    F.plans.reserve((size_t)n_groups);
    for (int t = 0, off = 0; t < n_groups; off += sizes[t], t++) {
        F.plans.push_back(md_plan(c, Lk, level, special, galois + off, sizes[t]));
        F.rows = std::max(F.rows, F.plans.back().L.rows_per_ct());
        F.ntt_rows = std::max(F.ntt_rows, F.plans.back().ntt_rows);
    }
    return F;
}
// All steps over one chunk.  `in`: F_0, [nb][2][level][N]; it may be FB[1] (step t reads FB[(t - 1) & 1] and writes FB[t & 1]), the
// last step writes `out` (+ bias on component 0).  `base`: F.rows rows per ciphertext of the chunk, laid out per group (md_bufs).
static int md_fold_run(tfhe_ctx* c, const md_fold_t& F, u64* base, int64_t chunk, u64* const FB[2], const u64* in, int64_t nb, const u64* bias,
                       u64* out) {
    const size_t N = (size_t)c->N;
    const u64* src = in;
    for (int t = 0, off = 0; t < F.n_groups; off += F.sizes[t], t++) {
        const md_plan_t& P = F.plans[(size_t)t];
        const md_bufs_t B = md_bufs(P, base, chunk);
        const bool last = t + 1 == F.n_groups;
        const size_t ct_words = (size_t)nb * 2 * P.level * N;
        const dim3 rows = row_grid((unsigned)(nb * 2 * P.level), N);
        u64* dst = last ? out : FB[t & 1];
        int rc;
        if (P.eval_form) {
            bool scaled = true;
            rc = md_rotations(c, P, F.evks + off, src, nb, B, &scaled);
            if (rc) return rc;
            u64* const sum = last && bias ? FB[t & 1] : dst;   // (the bias is a coefficient-domain row: added after the inverse transform)
            auto fold = scaled ? k_md_fold<false> : k_md_fold<true>;
            rc = launch(c, fold, dim3(8 * TFHE_MD_SLOTS), dim3(256), 0, (const u64*)B.X, (const u64*)B.S, (const u64*)B.ROT, sum, c->limbs_dev, P.sl,
                        P.G, P.ra, (u32)N, (u32)P.nw, (u32)P.R, (u32)nb);
            if (rc) return rc;
            rc = run_ntt(c, true, sum, sum, nb * 2 * P.level, P.sl);
            if (rc) return rc;
            if (sum != dst) {
                rc = launch(c, k_bsgs_sum, rows, dim3(256), 0, (const u64*)sum, (const u64*)sum, dst, c->limbs_dev, P.sl, (u32)N, 0u, ct_words, bias);
                if (rc) return rc;
            }
        } else {
            rc = md_rotations_coeff(c, P, F.evks + off, src, nb, B);
            if (rc) return rc;
            rc = launch(c, k_bsgs_sum, rows, dim3(256), 0, src, (const u64*)B.ROT, dst, c->limbs_dev, P.sl, (u32)N, (u32)P.R, ct_words,
                        last ? bias : (const u64*)nullptr);
            if (rc) return rc;
        }
        src = dst;
    }
    return TFHE_OK;
}

// the output tile: 4 giant steps per pass, fewer where there are fewer sums (log2)
static int bsgs_log_tile(int ngiant1) { return ngiant1 >= 3 ? 2 : ngiant1 - 1; }
// The device side of both entry points, after their host checks: n_in inputs, each with its own diagonals, feed ONE set of inner
// sums per chunk.  Input 0 of every chunk runs the unseeded accumulation (INNER still holds the previous chunk's sums), the others the
// seeded form, which continues from the reduced words in INNER; the baby-phase buffers are reused input after input (one stream, in
// order: md_lift_fwd's side lane has joined when md_rotations returns).  The giant rotations, the inverse transform and the closing
// sum (+ bias on component 0) then run once per chunk, whatever n_in.
static int matmul_bsgs_run(tfhe_ctx* c, int Lk, int level, int special, const uint64_t* const* baby_evks, const uint64_t* baby_galois, int n_baby,
                           const uint64_t* const* giant_evks, const uint64_t* giant_galois, int n_giant, const uint64_t* const* diags,
                           const uint64_t* const* cts, int n_in, const uint64_t* bias, uint64_t* out, int64_t batch, const md_fold_t* fold = nullptr) {
    const size_t N = (size_t)c->N;
    const int ng1 = n_giant + 1;
    const md_plan_t P = md_plan(c, Lk, level, special, baby_galois, n_baby);
    // One allocation: [ region 0 | the baby phase (md_bufs) | inner sums [ng1][chunk][2][level][N] | giant results [n_giant][chunk][2][level][N]
    // (| F [2][chunk][2][level][N] with fold steps) ].
    // Region 0 holds the scratch of the largest stand-alone transform (the baby phase's, the inner sums' inverse, the fold's) and is the
    // span the giant rotations' key switch lays out its own block in.  Nothing scales with n_in.
    // With fold steps (tfhe_matmul_bsgs_fold) the baby-phase region is as large as the largest fold group needs -- the fold runs when the
    // baby phase of the chunk is over -- and two ping-pong ciphertext buffers F follow the giant results: the closing sum writes F_0 into
    // FB[1] instead of `out`, and the last fold step writes `out`, with the bias.
    const size_t ct_rows = (size_t)2 * level;
    std::function<size_t(int64_t)> nested;
    if (n_giant) nested = [=](int64_t chunk) { return ks_rot_prepared_bytes(c, Lk, level, special, chunk); };
    ws_layout_t L(N);
    L.scratch(std::max({P.ntt_rows, (size_t)ng1 * ct_rows, fold ? fold->ntt_rows : (size_t)0}), nested);
    const ws_region_t phase = L.rows(std::max(P.L.rows_per_ct(), fold ? fold->rows : (size_t)0));
    const ws_region_t inner = L.rows((size_t)ng1 * ct_rows), gout = L.rows((size_t)n_giant * ct_rows);
    const ws_region_t f0 = L.rows(fold ? ct_rows : 0), f1 = L.rows(fold ? ct_rows : 0);
    const md_ws_t W(c, batch, L);
    if (W.rc) return W.rc;
    const int64_t chunk = W.chunk;
    const ws_span_t span = W.region0();
    const md_bufs_t B = md_bufs(P, W.at(phase), chunk);
    u64 *const INNER = W.at(inner), *const GOUT = W.at(gout);
    u64* const FB[2] = {W.at(f0), W.at(f1)};
    int rc;
    for (int64_t b0 = 0; b0 < batch; b0 += chunk) {
        const int64_t nb = std::min(chunk, batch - b0);
        const size_t ct_words = (size_t)nb * 2 * level * N;   // one inner sum / one giant result of this chunk
        for (int m = 0; m < n_in; m++) {
            bool scaled = true;
            rc = md_rotations(c, P, baby_evks, cts[m] + (size_t)b0 * 2 * level * N, nb, B, &scaled);
            if (rc) return rc;
            const u64* const dm = diags[m];
            rc = dispatch_int<0, 2>(bsgs_log_tile(ng1), [&](auto lg) {
                constexpr int NG = 1 << decltype(lg)::value;
                if (P.eval_form) {
                    auto acc = m == 0 ? (scaled ? k_md_acc<false, NG> : k_md_acc<true, NG>)
                                      : (scaled ? k_md_acc<false, NG, true> : k_md_acc<true, NG, true>);
                    return launch(c, acc, dim3(8 * TFHE_MD_SLOTS), dim3(256), 0, B.X, B.S, B.ROT, dm, INNER, c->limbs_dev, P.sl, P.G, P.ra, (u32)N,
                                  (u32)P.nw, (u32)P.R, (u32)nb, (u32)ng1);
                }
                auto acc = m == 0 ? k_md_acc_dense<NG> : k_md_acc_dense<NG, true>;
                return launch(c, acc, row_grid((unsigned)(nb * 2 * level), N), dim3(256), 0, B.X, B.ROT, dm, INNER, c->limbs_dev, P.sl, (u32)N,
                              (u32)P.R, (u32)(nb * 2 * level), (u32)ng1);
            });
            if (rc) return rc;
        }
        rc = run_ntt(c, true, INNER, INNER, (int64_t)ng1 * nb * 2 * level, P.sl);
        if (rc) return rc;
        for (int j = 1; j <= n_giant; j++) {   // (the nested call lays out its block in region 0)
            rc = keyswitch_impl(c, Lk, level, special, giant_evks[j - 1], INNER + (size_t)j * ct_words, 2, GOUT + (size_t)(j - 1) * ct_words, nb,
                                giant_galois[j - 1], true, false, true, &span);
            if (rc) return rc;
        }
        u64* const o = out + (size_t)b0 * 2 * level * N;
        rc = launch(c, k_bsgs_sum, row_grid((unsigned)(nb * 2 * level), N), dim3(256), 0, (const u64*)INNER, (const u64*)GOUT,
                    fold ? FB[1] : o, c->limbs_dev, P.sl, (u32)N, (u32)n_giant, ct_words, fold ? (const u64*)nullptr : (const u64*)bias);
        if (rc) return rc;
        if (fold) {
            rc = md_fold_run(c, *fold, W.at(phase), chunk, FB, FB[1], nb, bias, o);
            if (rc) return rc;
        }
    }
    return TFHE_OK;
}
int tfhe_matmul_bsgs(tfhe_ctx* c, int Lk, int level, int special, const uint64_t* const* baby_evks, const uint64_t* baby_galois, int n_baby,
                     const uint64_t* const* giant_evks, const uint64_t* giant_galois, int n_giant, int n_digits, const uint64_t* diags,
                     const uint64_t* ct, uint64_t* out, int64_t batch) {
    // host checks that need no ring first, then the context, then the ring's
    if (!baby_evks || !baby_galois || !giant_evks || !giant_galois || !diags || !ct || !out) return fail(TFHE_E_BADARG, "null argument");
    if (n_baby < 0 || n_baby > TFHE_DOT_MAX) return fail(TFHE_E_BADARG, "n_baby=%d outside [0,%d]", n_baby, TFHE_DOT_MAX);
    if (n_giant < 0 || n_giant > TFHE_DOT_MAX) return fail(TFHE_E_BADARG, "n_giant=%d outside [0,%d]", n_giant, TFHE_DOT_MAX);
    for (int r = 0; r < n_baby; r++)
        if (!baby_evks[r]) return fail(TFHE_E_BADARG, "null baby key %d", r);
    for (int r = 0; r < n_giant; r++)
        if (!giant_evks[r]) return fail(TFHE_E_BADARG, "null giant key %d", r);
    for (int r = 0; r < n_baby + n_giant; r++)
        if (((r < n_baby ? baby_galois[r] : giant_galois[r - n_baby]) & 1) == 0) return fail(TFHE_E_BADARG, "galois element must be odd and below 2N");
    if ((const void*)out == (const void*)ct || (const void*)out == (const void*)diags) return fail(TFHE_E_BADARG, "out overlaps an operand");
    if (!c) return fail(TFHE_E_BADARG, "null context");
    int rc = ks_check(c, Lk, level, special, diags, n_digits, ct, 2, out, batch);
    if (rc) return rc;
    for (int r = 0; r < n_baby + n_giant; r++)
        if ((rc = galois_check(c, r < n_baby ? baby_galois[r] : giant_galois[r - n_baby]))) return rc;
    const size_t N = (size_t)c->N;
    const size_t ct_bytes = (size_t)batch * 2 * level * N * 8;
    if (ranges_overlap(out, ct_bytes, ct, ct_bytes) || ranges_overlap(out, ct_bytes, diags, (size_t)(n_giant + 1) * (n_baby + 1) * level * N * 8))
        return fail(TFHE_E_BADARG, "out overlaps an operand");
    if (batch == 0) return TFHE_OK;
    return matmul_bsgs_run(c, Lk, level, special, baby_evks, baby_galois, n_baby, giant_evks, giant_galois, n_giant, &diags, &ct, 1, nullptr, out, batch);
}

// ---- the block-row product: several inputs, one set of giant rotations -------------------------------------------------------
// out = sum_m M_m x_m (+ bias) for n_in ciphertext inputs, each with its own diagonals, over ONE key set.  The rotation is linear:
//     sum_m sum_j rho^(j n1)( inner_{m,j} ) = sum_j rho^(j n1)( sum_m inner_{m,j} ),
// so the inner sums of all inputs are added -- in the accumulation itself, seeded -- before they are inverse-transformed and rotated:
// n_giant giant key switches and n_giant + 1 inverse-transformed sums instead of n_in times as many, one pass over the output.
// The words are those of ONE tfhe_dot over all n_in (n_baby + 1) terms per giant step, not those of n_in calls of
// tfhe_matmul_bsgs added up: the contraction by the special prime rounds once per giant step here.
int tfhe_matmul_bsgs_blocks(tfhe_ctx* c, int Lk, int level, int special, const uint64_t* const* baby_evks, const uint64_t* baby_galois, int n_baby,
                            const uint64_t* const* giant_evks, const uint64_t* giant_galois, int n_giant, int n_digits,
                            const uint64_t* const* diags, const uint64_t* const* cts, int n_in, const uint64_t* bias, uint64_t* out, int64_t batch) {
    // host checks that need no ring first (nulls, counts, parity, equal starts), then the context, then the ring's
    if (!baby_evks || !baby_galois || !giant_evks || !giant_galois || !diags || !cts || !out) return fail(TFHE_E_BADARG, "null argument");
    const auto within = [](int n) { return n < 0 ? 0 : (n > TFHE_DOT_MAX ? TFHE_DOT_MAX : n); };   // (an array is read no further than a valid count reaches)
    for (int r = 0; r < within(n_baby); r++)
        if (!baby_evks[r]) return fail(TFHE_E_BADARG, "null baby key %d", r);
    for (int r = 0; r < within(n_giant); r++)
        if (!giant_evks[r]) return fail(TFHE_E_BADARG, "null giant key %d", r);
    for (int m = 0; m < within(n_in); m++) {
        if (!diags[m]) return fail(TFHE_E_BADARG, "null diagonals of input %d", m);
        if (!cts[m]) return fail(TFHE_E_BADARG, "null ciphertext of input %d", m);
    }
    if (n_baby < 0 || n_baby > TFHE_DOT_MAX) return fail(TFHE_E_BADARG, "n_baby=%d outside [0,%d]", n_baby, TFHE_DOT_MAX);
    if (n_giant < 0 || n_giant > TFHE_DOT_MAX) return fail(TFHE_E_BADARG, "n_giant=%d outside [0,%d]", n_giant, TFHE_DOT_MAX);
    if (n_in < 1 || n_in > TFHE_DOT_MAX) return fail(TFHE_E_BADARG, "n_in=%d outside [1,%d]", n_in, TFHE_DOT_MAX);
    for (int r = 0; r < n_baby + n_giant; r++)
        if (((r < n_baby ? baby_galois[r] : giant_galois[r - n_baby]) & 1) == 0) return fail(TFHE_E_BADARG, "galois element must be odd and below 2N");
    if ((const void*)out == (const void*)bias) return fail(TFHE_E_BADARG, "out overlaps an operand");
    for (int m = 0; m < n_in; m++)
        if ((const void*)out == (const void*)cts[m] || (const void*)out == (const void*)diags[m]) return fail(TFHE_E_BADARG, "out overlaps an operand");
    if (!c) return fail(TFHE_E_BADARG, "null context");
    int rc = ks_check(c, Lk, level, special, diags[0], n_digits, cts[0], 2, out, batch);
    if (rc) return rc;
    for (int r = 0; r < n_baby + n_giant; r++)
        if ((rc = galois_check(c, r < n_baby ? baby_galois[r] : giant_galois[r - n_baby]))) return rc;
    const size_t N = (size_t)c->N;
    const size_t ct_bytes = (size_t)batch * 2 * level * N * 8, diag_bytes = (size_t)(n_giant + 1) * (n_baby + 1) * level * N * 8;
    if (bias && ranges_overlap(out, ct_bytes, bias, (size_t)level * N * 8)) return fail(TFHE_E_BADARG, "out overlaps an operand");
    for (int m = 0; m < n_in; m++)
        if (ranges_overlap(out, ct_bytes, cts[m], ct_bytes) || ranges_overlap(out, ct_bytes, diags[m], diag_bytes))
            return fail(TFHE_E_BADARG, "out overlaps an operand");
    if (batch == 0) return TFHE_OK;
    return matmul_bsgs_run(c, Lk, level, special, baby_evks, baby_galois, n_baby, giant_evks, giant_galois, n_giant, diags, cts, n_in, bias, out, batch);
}

// ---- rotate-and-sum, and the product of a rectangular matrix ------------------------------------------------------------------------
// the checks of a fold's host arrays that need no ring, after the null arrays: the group count, the group sizes, their sum, the keys
static int fold_check_host(const uint64_t* const* evks, const int* sizes, int n_groups) {
    if (n_groups < 0 || n_groups > TFHE_DOT_MAX) return fail(TFHE_E_BADARG, "n_fold_groups=%d outside [0,%d]", n_groups, TFHE_DOT_MAX);
    int total = 0;
    for (int t = 0; t < n_groups; t++) {
        if (sizes[t] < 1) return fail(TFHE_E_BADARG, "fold group %d has size %d, below 1", t, sizes[t]);
        if (sizes[t] > TFHE_DOT_MAX || (total += sizes[t]) > TFHE_DOT_MAX) return fail(TFHE_E_BADARG, "more than %d fold keys", TFHE_DOT_MAX);
    }
    for (int r = 0; r < total; r++)
        if (!evks[r]) return fail(TFHE_E_BADARG, "null fold key %d", r);
    return TFHE_OK;
}
static int fold_total(const int* sizes, int n_groups) {
    int total = 0;
    for (int t = 0; t < n_groups; t++) total += sizes[t];
    return total;
}
int tfhe_rotate_sum(tfhe_ctx* c, int Lk, int level, int special, const uint64_t* const* evks, const uint64_t* galois, const int* group_sizes,
                    int n_groups, int n_digits, const uint64_t* ct, uint64_t* out, int64_t batch) {
    // host checks that need no ring first (nulls, counts, parity, equal starts), then the context, then the ring's
    if (!evks || !galois || !group_sizes || !ct || !out) return fail(TFHE_E_BADARG, "null argument");
    int rc = fold_check_host(evks, group_sizes, n_groups);
    if (rc) return rc;
    const int total = fold_total(group_sizes, n_groups);
    for (int r = 0; r < total; r++)
        if ((galois[r] & 1) == 0) return fail(TFHE_E_BADARG, "galois element must be odd and below 2N");
    if ((const void*)out == (const void*)ct) return fail(TFHE_E_BADARG, "out overlaps an operand");
    if (!c) return fail(TFHE_E_BADARG, "null context");
    rc = ks_check(c, Lk, level, special, ct, n_digits, ct, 2, out, batch);
    if (rc) return rc;
    for (int r = 0; r < total; r++)
        if ((rc = galois_check(c, galois[r]))) return rc;
    const size_t N = (size_t)c->N;
    const size_t ct_bytes = (size_t)batch * 2 * level * N * 8;
    if (ranges_overlap(out, ct_bytes, ct, ct_bytes)) return fail(TFHE_E_BADARG, "out overlaps an operand");
    if (batch == 0) return TFHE_OK;
    if (n_groups == 0) {   // out = ct
        const limb_sel_t sl = first_limbs(level);
        for (int64_t b0 = 0; b0 < batch; b0 += 0x10000) {   // (the row count of one launch stays far below 2^31)
            const int64_t nb = std::min<int64_t>(0x10000, batch - b0);
            const u64* s = ct + (size_t)b0 * 2 * level * N;
            rc = launch(c, k_bsgs_sum, row_grid((unsigned)(nb * 2 * level), N), dim3(256), 0, s, s, out + (size_t)b0 * 2 * level * N, c->limbs_dev,
                        sl, (u32)N, 0u, (size_t)0, (const u64*)nullptr);
            if (rc) return rc;
        }
        return TFHE_OK;
    }
    const md_fold_t F = md_fold_plan(c, Lk, level, special, evks, galois, group_sizes, n_groups);
    // One allocation: [ region 0: transform scratch | the rotation phase of the largest group (md_bufs) | two ping-pong ciphertext buffers F ].
    ws_layout_t L(N);
    L.scratch(F.ntt_rows);
    const ws_region_t phase = L.rows(F.rows), f0 = L.rows((size_t)2 * level), f1 = L.rows((size_t)2 * level);
    const md_ws_t W(c, batch, L);
    if (W.rc) return W.rc;
    const int64_t chunk = W.chunk;
    u64* const FB[2] = {W.at(f0), W.at(f1)};
    for (int64_t b0 = 0; b0 < batch; b0 += chunk) {
        const int64_t nb = std::min(chunk, batch - b0);
        rc = md_fold_run(c, F, W.at(phase), chunk, FB, ct + (size_t)b0 * 2 * level * N, nb, nullptr, out + (size_t)b0 * 2 * level * N);
        if (rc) return rc;
    }
    return TFHE_OK;
}

// out = fold( sum_m M_m x_m ) + bias: tfhe_matmul_bsgs_blocks without its bias, the fold steps over the chunk's result while it is
// still in the workspace, and the bias -- AFTER the fold, which would multiply it -- with the last step's store.  For an m x n matrix,
// m | n, the diagonals are the m extended ones and the fold's log2(n / m) steps add up the n / m partial sums (she.rect_diagonals).
int tfhe_matmul_bsgs_fold(tfhe_ctx* c, int Lk, int level, int special, const uint64_t* const* baby_evks, const uint64_t* baby_galois, int n_baby,
                          const uint64_t* const* giant_evks, const uint64_t* giant_galois, int n_giant, int n_digits,
                          const uint64_t* const* diags, const uint64_t* const* cts, int n_in, const uint64_t* const* fold_evks,
                          const uint64_t* fold_galois, const int* fold_group_sizes, int n_fold_groups, const uint64_t* bias, uint64_t* out,
                          int64_t batch) {
    // the checks of tfhe_matmul_bsgs_blocks, in its order, with the fold's among them
    if (!baby_evks || !baby_galois || !giant_evks || !giant_galois || !diags || !cts || !fold_evks || !fold_galois || !fold_group_sizes || !out)
        return fail(TFHE_E_BADARG, "null argument");
    const auto within = [](int n) { return n < 0 ? 0 : (n > TFHE_DOT_MAX ? TFHE_DOT_MAX : n); };   // (an array is read no further than a valid count reaches)
    for (int r = 0; r < within(n_baby); r++)
        if (!baby_evks[r]) return fail(TFHE_E_BADARG, "null baby key %d", r);
    for (int r = 0; r < within(n_giant); r++)
        if (!giant_evks[r]) return fail(TFHE_E_BADARG, "null giant key %d", r);
    for (int m = 0; m < within(n_in); m++) {
        if (!diags[m]) return fail(TFHE_E_BADARG, "null diagonals of input %d", m);
        if (!cts[m]) return fail(TFHE_E_BADARG, "null ciphertext of input %d", m);
    }
    if (n_baby < 0 || n_baby > TFHE_DOT_MAX) return fail(TFHE_E_BADARG, "n_baby=%d outside [0,%d]", n_baby, TFHE_DOT_MAX);
    if (n_giant < 0 || n_giant > TFHE_DOT_MAX) return fail(TFHE_E_BADARG, "n_giant=%d outside [0,%d]", n_giant, TFHE_DOT_MAX);
    if (n_in < 1 || n_in > TFHE_DOT_MAX) return fail(TFHE_E_BADARG, "n_in=%d outside [1,%d]", n_in, TFHE_DOT_MAX);
    int rc = fold_check_host(fold_evks, fold_group_sizes, n_fold_groups);
    if (rc) return rc;
    const int n_fold = fold_total(fold_group_sizes, n_fold_groups);
    const auto element = [&](int r) { return r < n_baby ? baby_galois[r] : (r < n_baby + n_giant ? giant_galois[r - n_baby] : fold_galois[r - n_baby - n_giant]); };
    for (int r = 0; r < n_baby + n_giant + n_fold; r++)
        if ((element(r) & 1) == 0) return fail(TFHE_E_BADARG, "galois element must be odd and below 2N");
    if ((const void*)out == (const void*)bias) return fail(TFHE_E_BADARG, "out overlaps an operand");
    for (int m = 0; m < n_in; m++)
        if ((const void*)out == (const void*)cts[m] || (const void*)out == (const void*)diags[m]) return fail(TFHE_E_BADARG, "out overlaps an operand");
    if (!c) return fail(TFHE_E_BADARG, "null context");
    rc = ks_check(c, Lk, level, special, diags[0], n_digits, cts[0], 2, out, batch);
    if (rc) return rc;
    for (int r = 0; r < n_baby + n_giant + n_fold; r++)
        if ((rc = galois_check(c, element(r)))) return rc;
    const size_t N = (size_t)c->N;
    const size_t ct_bytes = (size_t)batch * 2 * level * N * 8, diag_bytes = (size_t)(n_giant + 1) * (n_baby + 1) * level * N * 8;
    if (bias && ranges_overlap(out, ct_bytes, bias, (size_t)level * N * 8)) return fail(TFHE_E_BADARG, "out overlaps an operand");
    for (int m = 0; m < n_in; m++)
        if (ranges_overlap(out, ct_bytes, cts[m], ct_bytes) || ranges_overlap(out, ct_bytes, diags[m], diag_bytes))
            return fail(TFHE_E_BADARG, "out overlaps an operand");
    if (batch == 0) return TFHE_OK;
    if (n_fold_groups == 0)
        return matmul_bsgs_run(c, Lk, level, special, baby_evks, baby_galois, n_baby, giant_evks, giant_galois, n_giant, diags, cts, n_in, bias, out, batch);
    const md_fold_t F = md_fold_plan(c, Lk, level, special, fold_evks, fold_galois, fold_group_sizes, n_fold_groups);
    return matmul_bsgs_run(c, Lk, level, special, baby_evks, baby_galois, n_baby, giant_evks, giant_galois, n_giant, diags, cts, n_in, bias, out, batch, &F);
}

// ---- the rotation phase on grouped-digit keys -------------------------------------------------------------------------------------
// md_plan / md_bufs / md_rotations for keys with grouped RNS digits and K = n_special special primes (ks_group_core.h).  The K-step
// contraction of one ciphertext limb is affine in its word, tail_j(x) = x Pinv_j + tail_j(0) with Pinv_j = prod_t p_t^-1 mod q_j, NTT_j
// is linear and sigma_g is the permutation pi_g in the evaluation domain, so exactly as for one special prime (kernels.h, above
// k_md_special_perm)
//     NTT_j(rotate_grouped(gk, c))_s [k] = V_s,j[pi_g k] - U_s,j[k]
//     V_s,j = S'_s,j Pinv_j + NTT_j(c_0) [s = 0]                       the key-sum kernels' epilogue (EPI), unpermuted
//     y     = ks_group_tail_special<K>( INTT_{p_u}( S'_s,p_u o pi_g ), u < K )      k_mdg_special_perm, K inverse transforms
//     U_s,j = NTT_j( negmod( ks_group_tail_limb<K>(0, y) ) )             k_mdg_lift, `level` forward transforms in place
// The special limbs are permuted BEFORE their inverse transform: the unsigned representatives the floors take are the rotated
// polynomial's (the point k_ks_group_rot_tail makes about signs).  K inverse and `level` forward transforms per key-sum component
// instead of level + K inverse, the tail and `level` forward.  Exact arithmetic on canonical residues: the words of
// tfhe_rotate_many_grouped -> tfhe_nntt.  U carries its scale: k_md_acc<false, ..> reads V, U, X as the per-limb phase leaves them.
// The coefficient route (K = 0, no rotations, or TFHE_MD_COEFF=1): ksg_hoist_tile -> forward transforms, for k_md_acc_dense.
struct mdg_plan_t {
    ksg_hoist_t H;
    ks_arg_t A;          // H.P.A with pinv[j] = Pinv_j: the key sums' epilogue
    limb_sel_t sl, sp;   // the ciphertext's limbs; the K special primes
    rot_tail_arg_t G;
    rescale_arg_t ra;    // (k_md_acc's USCALE factors: unused, U carries its scale)
    int Lk, level, K, nw, R;
    bool eval_form;
    // The phase's rows of a chunk, from wherever the caller puts them (no region 0 of its own): digits (d nw rows per ciphertext), key
    // sums (max(R, giant) 2 nw), ROT: U / rotated ciphertexts (R 2 level), X: the ciphertext's own transform (2 level), PB: the permuted
    // special limbs (R 2 K)
    ws_layout_t L;
    ws_region_t dig, S, ROT, X, PB;
    size_t ntt_rows;     // rows of the largest stand-alone transform, per ciphertext
};
// giant: the digits and ONE key sum are also wanted when there is no baby step (the giant rotations of tfhe_matmul_bsgs_grouped reuse
// the two regions once the baby phase of the chunk is over)
static int mdg_plan(tfhe_ctx* c, int Lk, int level, int k, int group, const uint64_t* galois, int R, bool giant, mdg_plan_t* P) {
    *P = mdg_plan_t{};
    const int rc = ksg_hoist_plan(c, Lk, level, k, group, std::max(R, giant ? 1 : 0), &P->H);
    if (rc) return rc;
    const ks_group_arg_t& G = P->H.P.G;
    P->Lk = Lk; P->level = level; P->K = k; P->nw = G.nw; P->R = R;
    P->sl = first_limbs(level);
    P->sp.n = k;
    for (int t = 0; t < k; t++) P->sp.idx[t] = G.w.idx[level + t];
    P->A = P->H.P.A;
    for (int j = 0; j < level && k > 0; j++) {
        const u64 qj = c->q[j];
        u64 pinv = 1 % qj;
        for (int t = 0; t < k; t++) pinv = hostmath::mulmod_slow(pinv, G.inv[t][j].w, qj);
        P->A.pinv[j] = hostmath::make_tw(pinv, qj);
    }
    for (int r = 0; r < R; r++) P->G.g[r] = galois[r];
    static const bool md_coeff = env_flag("TFHE_MD_COEFF", false);
    P->eval_form = k >= 1 && R >= 1 && !md_coeff;
    const size_t ct_rows = (size_t)2 * level;
    const size_t dig_rows = (R || giant) ? P->H.dig_rows : 0, S_rows = (size_t)std::max(R, giant ? 1 : 0) * 2 * G.nw;
    P->L = ws_layout_t((size_t)c->N);
    P->dig = P->L.rows(dig_rows); P->S = P->L.rows(S_rows); P->ROT = P->L.rows((size_t)R * ct_rows);
    P->X = P->L.rows(ct_rows); P->PB = P->L.rows((size_t)R * 2 * k);
    P->ntt_rows = std::max({dig_rows, S_rows, (size_t)R * ct_rows, ct_rows});
    return TFHE_OK;
}
// S: the key sums -- V in the EPI layout (evaluation-domain form) or [R][nb][2][nw][N];  ROT: U, or the transformed rotated
// ciphertexts, [R][nb][2][level][N];  PB: [R][nb][2][K][N]
struct mdg_bufs_t { u64 *dig, *S, *ROT, *X, *PB; };
static mdg_bufs_t mdg_bufs(const mdg_plan_t& P, u64* base, int64_t chunk) {
    const auto at = [&](ws_region_t h) { return P.L.at(base, chunk, h); };
    return mdg_bufs_t{at(P.dig), at(P.S), at(P.ROT), at(P.X), at(P.PB)};
}
// X = NTT(cin) and, per rotation r: evaluation-domain form -- V in S and U in ROT; otherwise NTT(rotate_grouped(gk_r, cin)) in ROT
static int mdg_rotations(tfhe_ctx* c, const mdg_plan_t& P, const uint64_t* const* evks, const u64* cin, int64_t nb, const mdg_bufs_t& B) {
    const int level = P.level, R = P.R;
    const size_t N = (size_t)c->N;
    const u32 n = (u32)N;
    const bool v2 = N % 2 == 0 && ((uintptr_t)cin & 15u) == 0;
    int rc = run_ntt(c, false, cin, B.X, nb * 2 * level, P.sl);
    if (rc || R == 0) return rc;
    rc = ksg_digits_fwd(c, P.H.P, cin, B.dig, nb, v2);
    if (rc) return rc;
    if (!P.eval_form) {
        rc = ksg_hoist_tile(c, P.H, evks, P.G.g, R, cin, nb, B.dig, B.S, B.ROT, (size_t)nb * 2 * level * N);
        if (rc) return rc;
        return run_ntt(c, false, B.ROT, B.ROT, (int64_t)R * nb * 2 * level, P.sl);
    }
    const int64_t groups = (int64_t)R * nb * 2;
    rc = ks_inner_launch(c, P.A, P.Lk, nullptr, B.dig, B.S, nb, evks, R, B.X, level);   // limbs j < level leave as V = S' Pinv + X0 [s = 0]
    if (rc) return rc;
    rc = launch(c, k_mdg_special_perm, dim3(8 * TFHE_ROT_TAIL_SLOTS), dim3(256), 0, (const u64*)B.S, B.PB, P.G, n, (u32)P.nw, (u32)level, (u32)P.K,
                (u32)nb, (u32)groups);
    if (rc) return rc;
    rc = run_ntt(c, true, B.PB, B.PB, groups * P.K, P.sp);
    if (rc) return rc;
    const bool lv2 = N % 2 == 0 && (((uintptr_t)B.PB | (uintptr_t)B.ROT) & 15u) == 0;
    const u32 gx = lv2 ? (n / 2 + 255) / 256 : (n + 255) / 256;
    rc = dispatch_int<1, TFHE_KSG_MAX_SPECIAL>(P.K, [&](auto kc) {
        constexpr int K = decltype(kc)::value;
        auto lift = lv2 ? k_mdg_lift<K, 2> : k_mdg_lift<K, 1>;
        return launch(c, lift, dim3((unsigned)(groups * gx)), dim3(256), 0, (const u64*)B.PB, B.ROT, c->limbs_dev, P.H.P.G, n, gx);
    });
    if (rc) return rc;
    return run_ntt(c, false, B.ROT, B.ROT, groups * level, P.sl);
}
// the accumulation after mdg_rotations over one chunk: ngiant1 sums into `inner`, tiled (bsgs_log_tile); seeded: continue from `inner`
static int mdg_accumulate(tfhe_ctx* c, const mdg_plan_t& P, const mdg_bufs_t& B, const u64* diags, u64* inner, int64_t nb, int ngiant1, bool seeded) {
    const size_t N = (size_t)c->N;
    const int level = P.level;
    return dispatch_int<0, 2>(bsgs_log_tile(ngiant1), [&](auto lg) {
        constexpr int NG = 1 << decltype(lg)::value;
        if (P.eval_form) {
            auto acc = seeded ? k_md_acc<false, NG, true> : k_md_acc<false, NG>;
            return launch(c, acc, dim3(8 * TFHE_MD_SLOTS), dim3(256), 0, (const u64*)B.X, (const u64*)B.S, (const u64*)B.ROT, diags, inner, c->limbs_dev,
                          P.sl, P.G, P.ra, (u32)N, (u32)P.nw, (u32)P.R, (u32)nb, (u32)ngiant1);
        }
        auto acc = seeded ? k_md_acc_dense<NG, true> : k_md_acc_dense<NG>;
        return launch(c, acc, row_grid((unsigned)(nb * 2 * level), N), dim3(256), 0, (const u64*)B.X, (const u64*)B.ROT, diags, inner, c->limbs_dev,
                      P.sl, (u32)N, (u32)P.R, (u32)(nb * 2 * level), (u32)ngiant1);
    });
}

// ---- the diagonal product on grouped-digit keys -----------------------------------------------------------------------------------
// out = diags[0] (.) NTT(c) + sum_r diags[r+1] (.) NTT(rotate_grouped(gk_r, c)): mdg_rotations over all n_rot <= 64 keys, then one
// accumulation (ngiant1 = 1) written where it belongs.  The words of tfhe_rotate_many_grouped -> tfhe_nntt -> tfhe_dot on either route.
// workspace: [ region 0: transform scratch | digits: [chunk][d][nw][N] | S / V: [chunk][R][2][nw][N] | ROT / U: [chunk][R][2][level][N] | X: [chunk][2][level][N]
//              | PB: [chunk][R][2][K][N] ]
int tfhe_matmul_diag_grouped(tfhe_ctx* c, int key_limbs, int level, int n_special, int group, const uint64_t* const* evks, int n_digits,
                             const uint64_t* galois_elements, int n_rot, const uint64_t* diags, const uint64_t* ct, uint64_t* out, int64_t batch) {
    bool nothing = false;
    int rc = ksg_many_check(c, true, key_limbs, level, n_special, group, evks, n_digits, galois_elements, n_rot, diags, ct, out, batch, &nothing);
    if (rc || nothing) return rc;
    mdg_plan_t P;
    rc = mdg_plan(c, key_limbs, level, n_special, group, galois_elements, n_rot, false, &P);
    if (rc) return rc;
    const size_t N = (size_t)c->N, ct_words = (size_t)2 * level * N;
    ws_layout_t L(N);
    L.scratch(P.ntt_rows);
    const ws_region_t phase = L.rows(P.L.rows_per_ct());
    const md_ws_t W(c, batch, L);
    if (W.rc) return W.rc;
    const int64_t chunk = W.chunk;
    const mdg_bufs_t B = mdg_bufs(P, W.at(phase), chunk);
    for (int64_t b0 = 0; b0 < batch; b0 += chunk) {
        const int64_t nb = std::min(chunk, batch - b0);
        rc = mdg_rotations(c, P, evks, ct + (size_t)b0 * ct_words, nb, B);
        if (rc) return rc;
        rc = mdg_accumulate(c, P, B, diags, out + (size_t)b0 * ct_words, nb, 1, false);
        if (rc) return rc;
    }
    return TFHE_OK;
}

// ---- the rotate-and-sum fold on grouped-digit keys ----------------------------------------------------------------------------------
// md_fold_t / md_fold_plan / md_fold_run for grouped keys: one mdg_plan_t per fold step with R = the step's size.  One step over a chunk,
//   evaluation route (K >= 1, TFHE_MDG_FOLD_EVAL=1):  X = NTT(F), the digits, V = the key sums with the Pinv epilogue, the permuted special limbs and their K
//                          inverse transforms as in mdg_rotations; then k_mdg_fold_gather writes E = X + sum_r V_r o pi_r into the
//                          step's ROT region (which this route does not otherwise use: R 2 level >= 2 level rows), ONE inverse
//                          transform of E, and k_mdg_fold_finish takes the lifts off in the coefficient domain, adds the bias in
//                          the last step and writes the step's result: no k_mdg_lift, no forward transform of a lift, no bias pass.
//                          Per ciphertext and step d nw + 2 level forward and R 2 K + 2 level inverse rows.
//   coefficient route (the default -- see mdg_fold_eval; K = 0 and TFHE_MD_COEFF=1 know no other):  the digits, ksg_hoist_tile into ROT in the
//                          coefficient domain, k_bsgs_sum (+ bias in the last step).  d nw forward and R 2 nw inverse rows.
// Exact arithmetic on canonical residues, NTT_j linear: the words of tfhe_rotate_many_grouped over the step's keys -> tfhe_add, step by step.
// Which route a fold step takes where both exist.  Measured (profiles/matmul_rect_grouped_bench.txt, profiles/LOG.md): the evaluation
// route is ahead in steps of three keys (fold radix 4) and behind in steps of one key (radix 2: at R = 1 it transforms MORE rows,
// d nw + 2 level + 2 K + 2 level against d nw + 2 nw), so it did not win at every measured shape and the coefficient route is the
// default.  TFHE_MDG_FOLD_EVAL=1 asks for the evaluation route (read once per process); TFHE_MD_COEFF=1 wins over it.
static bool mdg_fold_eval(int k) {
    static const bool md_coeff = env_flag("TFHE_MD_COEFF", false);
    static const bool fold_eval = env_flag("TFHE_MDG_FOLD_EVAL", false);
    return k >= 1 && !md_coeff && fold_eval;
}
struct mdg_fold_t {
    const uint64_t* const* evks;   // all steps back to back
    const uint64_t* galois;
    const int* sizes;
    int n_steps;
    std::vector<mdg_plan_t> plans; // one per step
    size_t rows = 0, ntt_rows = 0; // the largest step's (mdg_plan_t)
};
static int mdg_fold_plan(tfhe_ctx* c, int Lk, int level, int k, int group, const uint64_t* const* evks, const uint64_t* galois, const int* sizes,
                         int n_steps, mdg_fold_t* F) {
    *F = mdg_fold_t{evks, galois, sizes, n_steps, {}, 0, 0};
    F->plans.resize((size_t)n_steps);
    for (int t = 0, off = 0; t < n_steps; off += sizes[t], t++) {
        mdg_plan_t& P = F->plans[(size_t)t];
        const int rc = mdg_plan(c, Lk, level, k, group, galois + off, sizes[t], false, &P);
        if (rc) return rc;
        P.eval_form = mdg_fold_eval(k);
        F->rows = std::max(F->rows, P.L.rows_per_ct());
        F->ntt_rows = std::max(F->ntt_rows, P.ntt_rows);
    }
    return TFHE_OK;
}
// All steps over one chunk.  `in`: F_0, [nb][2][level][N]; it may be FB[1] (step t reads FB[(t - 1) & 1] and writes FB[t & 1]), the
// last step writes `out` (+ bias on component 0).  `base`: F.rows rows per ciphertext of the chunk, laid out per step (mdg_bufs).
static int mdg_fold_run(tfhe_ctx* c, const mdg_fold_t& F, u64* base, int64_t chunk, u64* const FB[2], const u64* in, int64_t nb, const u64* bias,
                        u64* out) {
    const size_t N = (size_t)c->N;
    const u32 n = (u32)N;
    const u64* src = in;
    for (int t = 0, off = 0; t < F.n_steps; off += F.sizes[t], t++) {
        const mdg_plan_t& P = F.plans[(size_t)t];
        const mdg_bufs_t B = mdg_bufs(P, base, chunk);
        const bool last = t + 1 == F.n_steps;
        const int level = P.level, R = P.R;
        const size_t ct_words = (size_t)nb * 2 * level * N;
        u64* const dst = last ? out : FB[t & 1];
        const u64* const bs = last ? bias : (const u64*)nullptr;
        int rc;
        if (P.eval_form) {
            rc = run_ntt(c, false, src, B.X, nb * 2 * level, P.sl);
            if (rc) return rc;
        }
        rc = ksg_digits_fwd(c, P.H.P, src, B.dig, nb, N % 2 == 0 && ((uintptr_t)src & 15u) == 0);
        if (rc) return rc;
        if (P.eval_form) {
            const int64_t groups = (int64_t)R * nb * 2;
            rc = ks_inner_launch(c, P.A, P.Lk, nullptr, B.dig, B.S, nb, F.evks + off, R, B.X, level);   // limbs j < level leave as V = S' Pinv + X0 [s = 0]
            if (rc) return rc;
            rc = launch(c, k_mdg_special_perm, dim3(8 * TFHE_ROT_TAIL_SLOTS), dim3(256), 0, (const u64*)B.S, B.PB, P.G, n, (u32)P.nw, (u32)level,
                        (u32)P.K, (u32)nb, (u32)groups);
            if (rc) return rc;
            rc = run_ntt(c, true, B.PB, B.PB, groups * P.K, P.sp);
            if (rc) return rc;
            u64* const E = B.ROT;
            rc = launch(c, k_mdg_fold_gather, dim3(8 * TFHE_MD_SLOTS), dim3(256), 0, (const u64*)B.X, (const u64*)B.S, E, c->limbs_dev, P.sl, P.G, n,
                        (u32)P.nw, (u32)R, (u32)nb);
            if (rc) return rc;
            rc = run_ntt(c, true, E, E, nb * 2 * level, P.sl);
            if (rc) return rc;
            const bool v2 = N % 2 == 0 && (((uintptr_t)B.PB | (uintptr_t)E | (uintptr_t)dst | (uintptr_t)bs) & 15u) == 0;
            const u32 gx = v2 ? (n / 2 + 255) / 256 : (n + 255) / 256;
            rc = dispatch_int<1, TFHE_KSG_MAX_SPECIAL>(P.K, [&](auto kc) {
                constexpr int K = decltype(kc)::value;
                auto finish = v2 ? k_mdg_fold_finish<K, 2> : k_mdg_fold_finish<K, 1>;
                return launch(c, finish, dim3((unsigned)(nb * 2 * gx)), dim3(256), 0, (const u64*)B.PB, (const u64*)E, bs, dst, c->limbs_dev, P.H.P.G, n,
                              gx, (u32)R, (u32)nb);
            });
            if (rc) return rc;
        } else {
            rc = ksg_hoist_tile(c, P.H, F.evks + off, P.G.g, R, src, nb, B.dig, B.S, B.ROT, ct_words);
            if (rc) return rc;
            rc = launch(c, k_bsgs_sum, row_grid((unsigned)(nb * 2 * level), N), dim3(256), 0, src, (const u64*)B.ROT, dst, c->limbs_dev, P.sl, n, (u32)R,
                        ct_words, bs);
            if (rc) return rc;
        }
        src = dst;
    }
    return TFHE_OK;
}

// ---- the product by baby and giant steps on grouped-digit keys -------------------------------------------------------------------
// tfhe_matmul_bsgs_blocks on prepared grouped Galois keys, with matmul_bsgs_run's structure and its one borrowed block:
//     inner_j = sum_m sum_{i = 0 .. n_baby} diags[m][j][i] (.) NTT(r_i(cts[m]))            mdg_rotations + mdg_accumulate per input (seeded after the first)
//     out     = INTT(inner_0) + sum_{j >= 1} rotate_grouped(giant key j - 1, INTT(inner_j)) (+ bias on component 0)
// One batched inverse transform covers all inner sums.  Giant step j is a hoisted rotation with a tile of one key: ksg_digits_fwd on
// INNER_j, ksg_hoist_tile into GOUT_j -- in the digit and key-sum regions of the baby phase, which is over by then (one stream, in
// order), so no nested workspace.  k_bsgs_sum adds up.  The words of tfhe_rotate_many_grouped -> tfhe_nntt -> tfhe_dot -> tfhe_inntt ->
// tfhe_rotate_grouped -> tfhe_add.
// With fold steps (tfhe_matmul_bsgs_fold_grouped) the closing sum writes F_0 into FB[1] without the bias, the steps ping-pong FB[0] / FB[1]
// (mdg_fold_run, in the phase region: the baby phase of the chunk is over) and the last step writes `out`, with the bias.
// workspace: [ region 0: transform scratch | the baby phase (mdg_bufs) or the largest fold step's, whichever is larger | inner sums
//              [ng1][chunk][2][level][N] | giant results [n_giant][chunk][2][level][N] (| F [2][chunk][2][level][N] with fold steps) ]
static int matmul_bsgs_grouped_run(tfhe_ctx* c, int Lk, int level, int n_special, int group, const uint64_t* const* baby_evks,
                                   const uint64_t* baby_galois, int n_baby, const uint64_t* const* giant_evks, const uint64_t* giant_galois, int n_giant,
                                   const uint64_t* const* diags, const uint64_t* const* cts, int n_in, const uint64_t* bias, uint64_t* out,
                                   int64_t batch, const mdg_fold_t* fold = nullptr) {
    const int ng1 = n_giant + 1;
    mdg_plan_t P;
    int rc = mdg_plan(c, Lk, level, n_special, group, baby_galois, n_baby, n_giant > 0, &P);
    if (rc) return rc;
    const size_t N = (size_t)c->N, ct_rows = (size_t)2 * level;
    ws_layout_t L(N);
    L.scratch(std::max({P.ntt_rows, (size_t)ng1 * ct_rows, fold ? fold->ntt_rows : (size_t)0}));
    const ws_region_t phase = L.rows(std::max(P.L.rows_per_ct(), fold ? fold->rows : (size_t)0));
    const ws_region_t inner = L.rows((size_t)ng1 * ct_rows), gout = L.rows((size_t)n_giant * ct_rows);
    const ws_region_t f0 = L.rows(fold ? ct_rows : 0), f1 = L.rows(fold ? ct_rows : 0);
    const md_ws_t W(c, batch, L);
    if (W.rc) return W.rc;
    const int64_t chunk = W.chunk;
    const mdg_bufs_t B = mdg_bufs(P, W.at(phase), chunk);
    u64 *const INNER = W.at(inner), *const GOUT = W.at(gout);
    u64* const FB[2] = {W.at(f0), W.at(f1)};
    for (int64_t b0 = 0; b0 < batch; b0 += chunk) {
        const int64_t nb = std::min(chunk, batch - b0);
        const size_t ct_words = (size_t)nb * 2 * level * N;   // one inner sum / one giant result of this chunk
        for (int m = 0; m < n_in; m++) {
            rc = mdg_rotations(c, P, baby_evks, cts[m] + (size_t)b0 * 2 * level * N, nb, B);
            if (rc) return rc;
            rc = mdg_accumulate(c, P, B, diags[m], INNER, nb, ng1, m > 0);
            if (rc) return rc;
        }
        rc = run_ntt(c, true, INNER, INNER, (int64_t)ng1 * nb * 2 * level, P.sl);
        if (rc) return rc;
        for (int j = 1; j <= n_giant; j++) {
            const u64* const src = INNER + (size_t)j * ct_words;
            rc = ksg_digits_fwd(c, P.H.P, src, B.dig, nb, N % 2 == 0 && ((uintptr_t)src & 15u) == 0);
            if (rc) return rc;
            rc = ksg_hoist_tile(c, P.H, giant_evks + (j - 1), giant_galois + (j - 1), 1, src, nb, B.dig, B.S, GOUT + (size_t)(j - 1) * ct_words, ct_words);
            if (rc) return rc;
        }
        u64* const o = out + (size_t)b0 * 2 * level * N;
        rc = launch(c, k_bsgs_sum, row_grid((unsigned)(nb * 2 * level), N), dim3(256), 0, (const u64*)INNER, (const u64*)GOUT, fold ? FB[1] : o,
                    c->limbs_dev, P.sl, (u32)N, (u32)n_giant, ct_words, fold ? (const u64*)nullptr : bias);
        if (rc) return rc;
        if (fold) {
            rc = mdg_fold_run(c, *fold, W.at(phase), chunk, FB, FB[1], nb, bias, o);
            if (rc) return rc;
        }
    }
    return TFHE_OK;
}
int tfhe_matmul_bsgs_grouped(tfhe_ctx* c, int key_limbs, int level, int n_special, int group, const uint64_t* const* baby_evks,
                             const uint64_t* baby_galois, int n_baby, const uint64_t* const* giant_evks, const uint64_t* giant_galois, int n_giant,
                             int n_digits, const uint64_t* const* diags, const uint64_t* const* cts, int n_in, const uint64_t* bias, uint64_t* out,
                             int64_t batch) {
    bool nothing = false;
    {
        char msg[160];
        const int rc = ks_group_bsgs_check(!c || !baby_evks || !baby_galois || !giant_evks || !giant_galois || !diags || !cts || !out, c ? c->L : 0,
                                           c ? c->N : 0, key_limbs, level, n_special, group, n_digits, batch, baby_evks, baby_galois, n_baby, giant_evks,
                                           giant_galois, n_giant, diags, cts, n_in, (uintptr_t)bias, (uintptr_t)out, &nothing, msg, sizeof msg,
                                           TFHE_DOT_MAX);
        if (rc) return fail(rc, "%s", msg);
    }
    if (nothing) return TFHE_OK;
    return matmul_bsgs_grouped_run(c, key_limbs, level, n_special, group, baby_evks, baby_galois, n_baby, giant_evks, giant_galois, n_giant, diags, cts,
                                   n_in, bias, out, batch);
}

// ---- rotate-and-sum and the rectangular product on grouped-digit keys ------------------------------------------------------------
// tfhe_rotate_sum / tfhe_matmul_bsgs_fold with every rotation a tfhe_rotate_grouped (mdg_fold_plan, mdg_fold_run).
// workspace of tfhe_rotate_sum_grouped: [ region 0: transform scratch | the largest fold step (mdg_bufs) | two ping-pong ciphertext buffers F ]
int tfhe_rotate_sum_grouped(tfhe_ctx* c, int key_limbs, int level, int n_special, int group, const uint64_t* const* evks,
                            const uint64_t* galois_elements, const int* group_sizes, int n_groups, int n_digits, const uint64_t* ct, uint64_t* out,
                            int64_t batch) {
    bool nothing = false;
    {
        char msg[160];
        const int rc = ks_group_fold_check(false, !c || !evks || !galois_elements || !group_sizes || !ct || !out, c ? c->L : 0, c ? c->N : 0, key_limbs,
                                           level, n_special, group, n_digits, batch, nullptr, nullptr, 0, nullptr, nullptr, 0, nullptr, &ct, 1, evks,
                                           galois_elements, group_sizes, n_groups, 0, (uintptr_t)out, &nothing, msg, sizeof msg, TFHE_DOT_MAX);
        if (rc) return fail(rc, "%s", msg);
    }
    if (nothing) return TFHE_OK;
    const size_t N = (size_t)c->N, ct_words = (size_t)2 * level * N;
    int rc;
    if (n_groups == 0) {   // out = ct
        const limb_sel_t sl = first_limbs(level);
        for (int64_t b0 = 0; b0 < batch; b0 += 0x10000) {   // (the row count of one launch stays far below 2^31)
            const int64_t nb = std::min<int64_t>(0x10000, batch - b0);
            const u64* s = ct + (size_t)b0 * ct_words;
            rc = launch(c, k_bsgs_sum, row_grid((unsigned)(nb * 2 * level), N), dim3(256), 0, s, s, out + (size_t)b0 * ct_words, c->limbs_dev, sl, (u32)N,
                        0u, (size_t)0, (const u64*)nullptr);
            if (rc) return rc;
        }
        return TFHE_OK;
    }
    mdg_fold_t F;
    rc = mdg_fold_plan(c, key_limbs, level, n_special, group, evks, galois_elements, group_sizes, n_groups, &F);
    if (rc) return rc;
    ws_layout_t L(N);
    L.scratch(F.ntt_rows);
    const ws_region_t phase = L.rows(F.rows), f0 = L.rows((size_t)2 * level), f1 = L.rows((size_t)2 * level);
    const md_ws_t W(c, batch, L);
    if (W.rc) return W.rc;
    const int64_t chunk = W.chunk;
    u64* const FB[2] = {W.at(f0), W.at(f1)};
    for (int64_t b0 = 0; b0 < batch; b0 += chunk) {
        const int64_t nb = std::min(chunk, batch - b0);
        rc = mdg_fold_run(c, F, W.at(phase), chunk, FB, ct + (size_t)b0 * ct_words, nb, nullptr, out + (size_t)b0 * ct_words);
        if (rc) return rc;
    }
    return TFHE_OK;
}
int tfhe_matmul_bsgs_fold_grouped(tfhe_ctx* c, int key_limbs, int level, int n_special, int group, const uint64_t* const* baby_evks,
                                  const uint64_t* baby_galois, int n_baby, const uint64_t* const* giant_evks, const uint64_t* giant_galois, int n_giant,
                                  int n_digits, const uint64_t* const* diags, const uint64_t* const* cts, int n_in, const uint64_t* const* fold_evks,
                                  const uint64_t* fold_galois, const int* fold_group_sizes, int n_fold_groups, const uint64_t* bias, uint64_t* out,
                                  int64_t batch) {
    bool nothing = false;
    {
        char msg[160];
        const int rc = ks_group_fold_check(true, !c || !baby_evks || !baby_galois || !giant_evks || !giant_galois || !diags || !cts || !fold_evks ||
                                                     !fold_galois || !fold_group_sizes || !out,
                                           c ? c->L : 0, c ? c->N : 0, key_limbs, level, n_special, group, n_digits, batch, baby_evks, baby_galois, n_baby,
                                           giant_evks, giant_galois, n_giant, diags, cts, n_in, fold_evks, fold_galois, fold_group_sizes, n_fold_groups,
                                           (uintptr_t)bias, (uintptr_t)out, &nothing, msg, sizeof msg, TFHE_DOT_MAX);
        if (rc) return fail(rc, "%s", msg);
    }
    if (nothing) return TFHE_OK;
    if (n_fold_groups == 0)
        return matmul_bsgs_grouped_run(c, key_limbs, level, n_special, group, baby_evks, baby_galois, n_baby, giant_evks, giant_galois, n_giant, diags,
                                       cts, n_in, bias, out, batch);
    mdg_fold_t F;
    const int rc = mdg_fold_plan(c, key_limbs, level, n_special, group, fold_evks, fold_galois, fold_group_sizes, n_fold_groups, &F);
    if (rc) return rc;
    return matmul_bsgs_grouped_run(c, key_limbs, level, n_special, group, baby_evks, baby_galois, n_baby, giant_evks, giant_galois, n_giant, diags, cts,
                                   n_in, bias, out, batch, &F);
}
