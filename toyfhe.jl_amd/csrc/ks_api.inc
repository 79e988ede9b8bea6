// ks_api.inc -- the key switch: tfhe_keyswitch, the rotations and tfhe_keyswitch_window; included by toyfhe_hip.hip before
// md_api.inc (the diagonal products), bfv_api.inc and mul_api.inc, which call keyswitch_impl, ks_prelift_ok and ks_plan.
//
// Key switching (rlwe_she.jl:315-347).  By linearity of the NTT the expanded inputs never need transforming:
// out_s = c_s + INTT(S_s)  (plain)   or   c_s + modswitch-part of INTT(S_s)  (ModulusRaised),
// with S_s = Σ_i evk_{i,s} ⊙ NTT(digit_i)  (see k_ks_inner, k_ks_rescale_add); the buffers are laid out at ks_plan_t, through ws_layout.h.

// whether the fused key switches (k_ks_fused at N = 2^13 / 2^14, k_ks_fused_sub at 2^15 / 2^16) take this ring and level
static bool ks_fused14(const tfhe_ctx* c, int Lk, int level, int special) {
    const limb_sel_t w = working_limbs(Lk, level, special);
    if (c->variant != 0) return false;
    if (c->logN == 14) return sel_fp(c, w, 0);
    if (c->logN == 13) {  // the 256 x 32 geometry: same fused kernel (it takes 256 VGPRs + 222 AGPRs: one workgroup per CU)
        static const bool on = env_flag("TFHE_FUSED13", true);
        return on && sel_fp(c, w, 0);
    }
    if (c->logN == 16) {  // k_ks_fused_sub at X = 2
        static const bool on16 = env_flag("TFHE_FUSED16", true);
        return on16 && level >= 2 && sel_fp(c, w, 2);
    }
    return c->logN == 15 && level >= 2 && sel_fp(c, w, 1);  // k_ks_fused_sub
}
// pre-lifted c[end] rows (centred doubles from the BFV contraction) are understood by k_ks_fused only
static bool ks_prelift_ok(const tfhe_ctx* c, int level) {
    if (c->logN != 14 || !ks_fused14(c, level, level, 0)) return false;
    u64 lo = ~0ull, hi = 0;  // the bit-cast lift keeps |digit| <= q_i / 2 unreduced: needs q_i <= 2 q_j for every pair
    for (int j = 0; j < level; j++) { lo = std::min(lo, c->q[j]); hi = std::max(hi, c->q[j]); }
    return hi <= 2 * lo;
}
// the top stages of an N = 2^15 / 2^16 forward transform with the lift of ntt_io_t mode 1 fused into their loads (the u64 limbs of
// rings that mix modulus sizes), into the transform scratch `t`
static int launch_top_lift(tfhe_ctx* c, const u64* src, u64* t, int64_t rows, const limb_sel_t& sel, const ntt_io_t& io) {
    const int x = c->logN - 14;
    const dim3 tg((unsigned)((((c->N >> x) + 255) / 256) * rows));
    return dispatch_int<1, 2>(x, [&](auto xc) {
        return launch(c, k_ntt_fwd_top_lift<decltype(xc)::value>, tg, dim3(256), 0, src, t, c->limbs_dev, sel, c->logN, io);
    });
}
// Part A of the unfused key switch: the NTT-domain RNS digits of c[end], dig [batch][level][nw][N]
// (centred lift of limb i into every working limb, rlwe_she.jl:326-329, then forward transforms).
static int ks_digits_fwd(tfhe_ctx* c, const ks_arg_t& A, const u64* ct, u64* dig, int64_t batch) {
    const int level = A.level, nw = A.nw, polys = A.polys;
    const u32 n = (u32)c->N;
    int rc;
    const bool lift_fused = c->logN <= 14 || ((c->logN == 15 || c->logN == 16) && c->variant == 0 && sel_fp(c, A.w, c->logN - 14) &&
                                              (((uintptr_t)ct | (uintptr_t)dig) & 15u) == 0);
    // rings that mix fp64-size moduli with larger ones (infer.jl:97-112: 60-bit q0 and special prime next to 40-bit primes)
    // at N = 2^15 / 2^16: the fp64-size working limbs take the lift-fused one-kernel transforms (the fp64 lift reads source
    // limbs of either size), the others go through the digit buffer and the u64 kernels
    const policy_split_t ps = policy_split(c, A.w);
    const u32 fpmask = ps.fpmask, allmask = ps.all;
    const bool lift_mixed = !lift_fused && nw <= 32 && (c->logN == 15 || c->logN == 16) && c->variant == 0 && ps.mixed_fp() &&
                            (((uintptr_t)ct | (uintptr_t)dig) & 15u) == 0;
    if (lift_fused) {
        // digits: centred lift of limb i of c[end] into every working limb, fused into the forward NTT's loads
        ntt_io_t io = io_plain();
        io.mode = 1; io.level = (u32)level; io.nw = (u32)nw; io.polys = (u32)polys;
        rc = run_ntt(c, false, ct, dig, batch * level * nw, A.w, &io);
        if (rc) return rc;
    } else if (lift_mixed) {
        ntt_io_t io = io_plain();
        io.mode = 1; io.level = (u32)level; io.nw = (u32)nw; io.polys = (u32)polys; io.limb_mask = fpmask;
        const int64_t rows = batch * level * nw;
        const int x = c->logN - 14;
        void* tmp = nullptr;
        rc = ws_scratch(c, (size_t)rows * c->N * 8, &tmp);   // (before the fork: growing the workspace synchronises)
        if (rc) return rc;
        lanes_t lanes(c);   // the fp64-size working limbs on the side lane, beside the u64 ones
        lanes.use(1);
        rc = run_ntt_large(c, false, ct, dig, rows, A.w, io, &io, true, true);
        if (rc) return rc;
        lanes.use(0);
        // the larger working limbs: lift fused into the top-stage kernel (into the transform scratch), then the u64 block kernels
        ntt_io_t iw = io;
        iw.limb_mask = allmask & ~fpmask;
        rc = launch_top_lift(c, ct, (u64*)tmp, rows, A.w, iw);
        if (rc) return rc;
        ntt_io_t ib = io_plain();
        ib.limb_mask = allmask & ~fpmask;
        rc = launch_block_fwd<ArithInt, 14>(c, (const u64*)tmp, dig, rows, A.w, x, ib);
        if (rc) return rc;
    } else {
        rc = launch(c, k_ks_digits, row_grid((unsigned)(batch * level * nw), (size_t)c->N), dim3(256), 0, ct, dig, c->limbs_dev, A, n, 0u);
        if (rc) return rc;
        rc = run_ntt(c, false, dig, dig, batch * level * nw, A.w);
        if (rc) return rc;
    }
    return TFHE_OK;
}

// S_s = sum_i evk_{i,s} (.) digit_i over the working limbs (NTT domain), S: [batch][2][nw][N]
// keys != nullptr: `nkeys` keys against the same digits in one launch, key r writing S + r * batch*2*nw*N (tfhe_matmul_diag)
static int ks_inner_launch(tfhe_ctx* c, const ks_arg_t& A, int Lk, const u64* evk, const u64* dig, u64* S, int64_t batch,
                           const uint64_t* const* keys = nullptr, int nkeys = 0, const u64* epi_x = nullptr, int epi_level = 0) {
    const int nw = A.nw;
    ks_keys_t K{};
    if (keys) {
        K.n = nkeys;
        K.s_stride = (size_t)batch * 2 * nw * (size_t)c->N;
        for (int r = 0; r < nkeys; r++) K.key[r] = keys[r];
        evk = keys[0];
        K.epi_x = epi_x;
        K.epi_level = epi_level ? epi_level : A.level;   // (grouped-digit keys: A.level counts digits, the caller names the ciphertext's limbs)
    }
    const unsigned gy = keys ? (unsigned)nkeys : 1u;
    const u32 n = (u32)c->N;
    const unsigned gx = (n + 255) / 256;
    // enough workgroups to fill the chip: split the batch into slices (the key is re-read once per slice)
    // (several keys in one launch multiply the grid by gy)
    const unsigned bsplit = (unsigned)std::max<int64_t>(1, std::min<int64_t>(batch, (4096 + nw * gx * gy - 1) / (nw * gx * gy)));
    // working limbs below 2^52: the two-coefficient, carry-free kernel; the others: the generic one (more than 32 working
    // limbs: all or nothing, see mask_of)
    // several keys: groups of eight x-blocks (one per XCD), each followed by its keys (ks_multi_key_block)
    auto multi = [&](unsigned nx) { return keys ? dim3(((nx + 7u) / 8u) * 8u * gy) : dim3(nx); };
    const policy_split_t ps = policy_split(c, A.w);
    const u32 nmask = n % 2 != 0 ? 0u : ps.narrow, amask = ps.all;
    lanes_t lanes(c, nmask != 0 && nmask != amask);   // both kernels: side by side (disjoint working limbs)
    if (nmask) {
        lanes.use(1);
        const unsigned gx2 = (n / 2 + 255) / 256;
        const unsigned bs2 = (unsigned)std::max<int64_t>(1, std::min<int64_t>(batch, (4096 + nw * gx2 * gy - 1) / (nw * gx2 * gy)));
        auto kn = epi_x ? k_ks_inner_n2<8, true> : k_ks_inner_n2<8, false>;
        const int rc = launch(c, kn, multi((unsigned)nw * gx2 * bs2), dim3(256), 0, evk, dig, S, c->limbs_dev, A, Lk, n, (u32)batch, bs2,
                              nmask == amask ? 0u : nmask, K);
        if (rc) return rc;
    }
    if (nmask != amask) {
        lanes.use(0);
        auto kg = epi_x ? k_ks_inner<8, true> : k_ks_inner<8, false>;
        return launch(c, kg, multi((unsigned)nw * gx * bsplit), dim3(256), 0, evk, dig, S, c->limbs_dev, A, Lk, n, (u32)batch, bsplit,
                      nmask ? (amask & ~nmask) : 0u, K);
    }
    return TFHE_OK;
}
// the inverse top stages of N = 2^15 / 2^16 over the sub-block results T together with the tail ("+ c" / the special-prime
// contraction); g_tail != 0: the automorphism rides on the tail's stores (XCD-cooperative scatter, k_ks_top_tail_rot)
static int launch_top_tail(tfhe_ctx* c, const ks_arg_t& A, const rescale_arg_t& ra, const u64* T, const u64* ct, u64* out, int64_t batch, u64 g_tail) {
    const u32 n = (u32)c->N, add_s = A.polys == 3 ? 2u : 1u;
    return dispatch_int<1, 2>(c->logN - 14, [&](auto xc) {
        constexpr int X = decltype(xc)::value;
        if (g_tail)
            return launch(c, k_ks_top_tail_rot<X>, dim3(8 * TFHE_ROT_TAIL_SLOTS), dim3(256), 0, T, ct, out, c->limbs_dev, A, ra, n, add_s, g_tail, (u32)(batch * 2));
        return launch(c, k_ks_top_tail<X>, row_grid((unsigned)(batch * 2 * A.level), (size_t)c->N >> X), dim3(256), 0, T, ct, out, c->limbs_dev, A, ra, n, add_s);
    });
}
// The tail of every form that leaves whole key sums S ([batch][2][nw][N], NTT domain): out_s = ct_s + INTT(S_s), with the special
// prime the ModulusRaised contraction of INTT(S) (k_ks_rescale_add).  `A` is the row bookkeeping (level = ciphertext limbs); `ct`
// only supplies the addends.  S is transformed in place with the special prime and left as it is otherwise.
static int ks_plain_tail(tfhe_ctx* c, const ks_arg_t& A, const rescale_arg_t& ra, u64* S, const u64* ct, u64* out, int64_t batch) {
    const int level = A.level, polys = A.polys;
    const u32 n = (u32)c->N;
    const u32 add_s = polys == 3 ? 2u : 1u;  // c2 starts from zero for a 2-element input (rlwe_she.jl:324)
    const dim3 tail_grid = row_grid((unsigned)(batch * 2 * level), (size_t)c->N);
    int rc;
    if (A.special) {
        rc = run_ntt(c, true, S, S, batch * 2 * A.nw, A.w);
        if (rc) return rc;
        return launch(c, k_ks_rescale_add, tail_grid, dim3(256), 0, S, ct, out, c->limbs_dev, A, ra, n, add_s);
    }
    if (c->logN <= 14) {  // out = c + INTT(S), the addition fused into the inverse NTT's stores
        ntt_io_t io = io_plain();
        io.mode = 2; io.gsz = (u32)(2 * level); io.src_gstride = io.gsz; io.dst_gstride = io.gsz;
        io.add_rows = add_s * (u32)level; io.add_gstride = (u32)(polys * level); io.addend = ct;
        return run_ntt(c, true, S, out, batch * 2 * A.nw, A.w, &io);
    }
    rc = run_ntt(c, true, S, out, batch * 2 * A.nw, A.w);
    if (rc) return rc;
    return launch(c, k_ks_add_ct, tail_grid, dim3(256), 0, ct, out, c->limbs_dev, A, n, add_s);
}

// ---- the plan of one key switch ----------------------------------------------------------------------------------------
// Everything a call decides -- its route, how a rotation is carried, what is done to the key, the chunk and the workspace -- is
// decided once, by ks_plan; keyswitch_impl and ks_chunk read the plan, and so does whoever sizes a span for them (tfhe_mul_relin,
// matmul_bsgs_run).  Every environment switch of the key switch is read here or in ks_fused14, once per process.
//   KS_ROW: k_ks_fused, N = 2^13 / 2^14    KS_SUB: k_ks_fused_sub, N = 2^15 / 2^16, then the inverse top stages with the tail
//   KS_THREE: digit transforms (ks_digits_fwd), key sums (ks_inner_launch), inverse transforms + tail
enum ks_path_t { KS_ROW, KS_SUB, KS_THREE };
//   KS_ROT_COPY: do_galois into the workspace first, then a plain key switch of the copy    KS_ROT_TAIL: the rotation rides on the
//   final stores    KS_ROT_HOISTED: a prepared key on a path that cannot do that: the call is handed to tfhe_rotate_many
enum ks_rot_t { KS_ROT_NONE, KS_ROT_COPY, KS_ROT_TAIL, KS_ROT_HOISTED };
struct ks_plan_t {
    ks_arg_t A;
    rescale_arg_t ra;    // P^-1 mod q_j (special prime): not part of the decision, keyswitch_impl fills it for ks_chunk
    int Lk; ks_path_t path;
    bool two_launch;     // KS_ROW with the special prime: SPMODE 1, then 2 / 3; otherwise one launch (+ k_ks_rescale_add)
    bool prelifted;      // KS_ROW: c[end] arrives as centred doubles (the BFV contraction)
    bool fps;            // KS_SUB: every working modulus below TFHE_FPS_QMAX -- the range plan of that size class (ArithFpS)
    bool tail16;         // KS_THREE at N = 2^16: paired sub-block inverse + k_ks_top_tail<2>
    bool two_lanes;      // KS_THREE at N = 2^16: the two policies as two lanes from the lift to the inverse, ONE join before the tail
    ks_rot_t rot;
    u64 g_tail;          // KS_ROT_TAIL: the Galois element, otherwise 0
    bool key_perm;       // the key is permuted by g^-1: in k_evk_to_f64 on the fused paths, by k_ntt_perm on KS_THREE (else read in place)
    // workspace: [ region 0: transform scratch | S: [chunk][2][nw][N] | NTT'd digits: [chunk][level][nw][N], or T: [chunk][2][nw][N] on the
    // fused paths | rotated copy: [chunk][polys][level][N] ], then the key as doubles (k_evk_to_f64, fused paths) or permuted (k_ntt_perm)
    int64_t chunk;
    size_t N;
    ws_layout_t L;
    ws_region_t rS, rdig, rrot, rkey;   // the regions above, in that order
};
// `batch` is the CALL's batch; `ct` / `out` are the caller's operands (read for rotations and for the alignment of the lift's loads;
// none given: taken as disjoint and aligned -- whoever sizes a span for a call on operands of its own, ks_rot_prepared_bytes).
// key_prepared (rotations only, tfhe_rotate_prepared): the key is the output of tfhe_galois_key_prepare for `galois` -- the paths
// that finish the rotation in their tail consume it as it is (no per-call k_ntt_perm / permuting conversion); the others take the
// hoisted form of tfhe_rotate_many, which is defined on prepared keys (same bits)
static ks_plan_t ks_plan(const tfhe_ctx* c, int Lk, int level, int special, int polys, int64_t batch, const u64* ct = nullptr,
                         const u64* out = nullptr, u64 galois = 0, bool rotate = false, bool prelifted = false, bool key_prepared = false) {
    ks_plan_t P{};
    P.A = make_ks_arg(Lk, level, special, polys);
    const ks_arg_t& A = P.A;
    const int nw = A.nw;
    const size_t N = (size_t)c->N;
    P.Lk = Lk; P.N = N; P.prelifted = prelifted;   // (pre-lifted rows: KS_ROW only, keyswitch_impl checks)
    const bool f14 = ks_fused14(c, Lk, level, special);
    P.path = !f14 ? KS_THREE : (c->logN <= 14 ? KS_ROW : KS_SUB);
    if (P.path == KS_ROW) {
        // TFHE_KS_TAIL=1 keeps the one-launch form with k_ks_rescale_add (comparisons)
        static const bool ks_tail = env_flag("TFHE_KS_TAIL", false);
        P.two_launch = special && !prelifted && !ks_tail;
    } else if (P.path == KS_SUB) {
        // moduli below 2^42 (the 40-bit chains of the reference's CKKS rings): the range plan of that size class -- no forward
        // sweeps, no reduced product operands, one sweep per inverse (ArithFpS): cfg#3 36.5 k -> 38.1 k key switches/s
        bool small = true;
        for (int j = 0; j < nw; j++) small = small && c->q[A.w.idx[j]] < TFHE_FPS_QMAX;
        static const bool fps_on = env_flag("TFHE_FPS", true);
        P.fps = small && fps_on;
    } else {
        // two lanes: only when the digit transforms, the key sums and the inverse sub-block transforms all split the working limbs
        // the same way (fp64-size = "narrow"); otherwise every step forks and joins by itself
        const policy_split_t ps = policy_split(c, A.w);
        P.tail16 = c->logN == 16 && c->variant == 0 && ps.fpmask != 0 && level >= 2;
        P.two_lanes = P.tail16 && nw <= 32 && ps.mixed_fp() && ps.fpmask == ps.narrow;
    }
    // Rotations finished in the final stores: no rotated copy of the input -- the key sums are those of the unrotated digits
    // against the key permuted by g^-1, the automorphism rides on the stores.  Same bits (the hoisting identity of tfhe_rotate_many).
    //   KS_SUB, KS_THREE with tail16 : k_ks_top_tail_rot, one (ciphertext, component) per XCD at a time: the CALL's batch >= 8
    //   KS_ROW at 2^14, two launches : k_ks_fused SPMODE 3 -- each workgroup scatters the row it owns
    // The stores scatter into `out` while other workgroups still read the unrotated `ct`: the two RANGES must be disjoint (r05,
    // ADVICE r04: pointer inequality let a partially overlapping out / ct race).  TFHE_ROT_TAIL=0 keeps the separate pass.
    if (rotate) {
        static const bool rot_tail_on = env_flag("TFHE_ROT_TAIL", true);
        const bool io_disjoint = !ct || (const char*)(out + (size_t)batch * 2 * level * N) <= (const char*)ct ||
                                 (const char*)(ct + (size_t)batch * polys * level * N) <= (const char*)out;
        const bool can = P.path == KS_ROW ? (c->logN == 14 && P.two_launch) : (batch >= 8 && (P.path == KS_SUB || P.tail16));
        P.rot = (can && rot_tail_on && io_disjoint) ? KS_ROT_TAIL : (key_prepared ? KS_ROT_HOISTED : KS_ROT_COPY);
    }
    if (P.rot == KS_ROT_HOISTED) return P;   // tfhe_rotate_many plans for itself
    if (P.rot == KS_ROT_TAIL) P.g_tail = galois;
    P.key_perm = P.rot == KS_ROT_TAIL && !key_prepared;
    // the lift's 16-byte loads: of the caller's `ct` unless the rotated copy takes its place.  The workspace needs no test (ensure_ws
    // hands out whole hipMalloc blocks, its own or the pool's, devalloc::alloc_ws: 256-byte aligned), nor does a chunk: every region
    // and chunk offset is a multiple of 8 N bytes
    P.two_lanes = P.two_lanes && (P.rot == KS_ROT_COPY || ((uintptr_t)ct & 15u) == 0);
    // chunk the batch so that the digit tensor stays at a few GiB.  The fused key switches never write the digit rows: at
    // N = 2^15 the "digit" buffer only carries the sub-block sums T (2 nw rows per ciphertext), so a whole batch is one launch
    // (cfg#3, 512 ciphertexts: 248 + 248 + 16 before -- the 16 ran as two nearly empty item rounds of k_ks_fused_sub)
    P.L = ws_layout_t(N);
    // the digit transforms (level nw rows), the mixed lift and the key sums' inverse (2 nw) take region 0; the fused paths run no
    // stand-alone transform
    P.L.scratch(f14 ? 0 : (size_t)std::max(2, level) * nw);
    P.rS = P.L.rows((size_t)2 * nw);
    P.rdig = P.L.rows(f14 ? (size_t)2 * nw : (size_t)level * nw);
    P.rrot = P.L.rows(rotate ? (size_t)polys * level : 0);
    P.chunk = chunk_of(c, batch, 512, (size_t)8192 << 20, P.L.per_ct_bytes());
    P.rkey = P.L.tail(f14 ? (size_t)level * 2 * nw * N * 8 : (P.key_perm ? (size_t)level * 2 * Lk * N * 8 : 0));
    return P;
}

// One chunk of `batch` ciphertexts by the plan.  `key`: the caller's key or the workspace copy keyswitch_impl made; `ct`: the
// chunk's input -- the rotated copy under KS_ROT_COPY, the UNrotated input under KS_ROT_TAIL
static int ks_chunk(tfhe_ctx* c, const ks_plan_t& P, const u64* key, const u64* ct, u64* out, int64_t batch, u64* S, u64* dig) {
    const ks_arg_t& A = P.A;
    const int Lk = P.Lk, level = A.level, nw = A.nw, special = A.special;
    const u64* const none = nullptr;
    int rc;
    if (P.path == KS_ROW) {
        // everything in one kernel: digit lift, forward transforms, key inner product and the two inverse transforms;
        // with the special prime the transformed sums go to S and the contraction kernel finishes (modulusraising.jl:42)
        const unsigned items = (unsigned)(batch * nw);
        const int64_t transforms = (int64_t)items * (level + 2);  // limb transforms inside the fused launch(es): `level` forward + 2 inverse per item
        // two launches: the special limb of every ciphertext first (its coefficient rows t_P into S), then the ciphertext limbs with
        // the ModulusRaised contraction and "+ c" in their final store (k_ks_fused SPMODE 1 / 2, ArithFpMD).  No T, no tail kernel.
        if (P.two_launch) {
            {
                std::lock_guard<std::mutex> zg(c->zero_mu);         // a failed attempt (transient out-of-memory) is retried by the next call
                if (!c->zero_row) {
                    void* z = nullptr;
                    if (devalloc::malloc_retry(&z, (size_t)c->N * 8) == hipSuccess) {
                        if (hipMemset(z, 0, (size_t)c->N * 8) == hipSuccess) c->zero_row = (u64*)z;
                        else { (void)hipGetLastError(); (void)hipFree(z); }
                    } else (void)hipGetLastError();
                }
                if (!c->zero_row) return fail(TFHE_E_NOMEM, "allocating the zero row failed");
            }
            ks_arg_t A2 = A;   // these two launches only: P^-1 mod q_j, and the Galois element of a rotation finished in the store
            std::copy(P.ra.qlinv, P.ra.qlinv + level, A2.pinv);
            A2.rot_g = (u32)(P.g_tail & (2 * (u64)c->N - 1));
            const unsigned it1 = (unsigned)batch, it2 = (unsigned)(batch * level);
            auto launch2 = [&](auto k1, auto k2, int LOGT, size_t lds, unsigned per_cu) -> int {   // both launches in ONE profiled region
                prof_scope p(c, transforms);
                const int r1 = launch(c, k1, dim3(cu_grid(c, it1, per_cu)), dim3(1u << LOGT), lds, key, ct, S, c->limbs_dev, A2, Lk, it1, none, none);
                if (r1) return r1;
                return launch(c, k2, dim3(cu_grid(c, it2, per_cu)), dim3(1u << LOGT), lds, key, ct, out, c->limbs_dev, A2, Lk, it2, (const u64*)S, (const u64*)c->zero_row);
            };
            if (c->logN == 13) {
                constexpr int LOGT = logt_for(13);
                return launch2(k_ks_fused<ArithFp, 13, LOGT, false, 1>, k_ks_fused<ArithFp, 13, LOGT, false, 2>, LOGT, fused_lds_bytes<13, LOGT>(), 2u);
            }
            constexpr int LOGT = logt_for(14);
            // SPMODE 3: a rotation finished in the second launch's stores (`ct` is the unrotated input)
            auto k1 = k_ks_fused<ArithFp, 14, LOGT, false, 1>, k2 = !P.g_tail ? k_ks_fused<ArithFp, 14, LOGT, false, 2> : k_ks_fused<ArithFp, 14, LOGT, false, 3>;
            return launch2(k1, k2, LOGT, fused_lds_bytes<14, LOGT>(), 1u);
        }
        if (c->logN == 14) {
            constexpr int LOGT = logt_for(14);
            auto fk = P.prelifted ? k_ks_fused<ArithFp, 14, LOGT, true> : k_ks_fused<ArithFp, 14, LOGT, false>;
            rc = launch_prof(c, transforms, fk, dim3(cu_grid(c, items)), dim3(1 << LOGT), fused_lds_bytes<14, LOGT>(), key, ct,
                             special ? S : out, c->limbs_dev, A, Lk, items, none, none);
        } else {  // N = 2^13: 256 threads x 32 elements, 65 KiB of LDS; 478 registers per thread, so one workgroup per CU is resident
                  // (capped to two resident workgroups it measured 5 % slower, DESIGN.md section 8)
            constexpr int LOGT = logt_for(13);
            rc = launch_prof(c, transforms, k_ks_fused<ArithFp, 13, LOGT, false>, dim3(cu_grid(c, items, 2u)), dim3(1 << LOGT), fused_lds_bytes<13, LOGT>(),
                             key, ct, special ? S : out, c->limbs_dev, A, Lk, items, none, none);
        }
        if (rc || !special) return rc;
        return launch(c, k_ks_rescale_add, row_grid((unsigned)(batch * 2 * level), (size_t)c->N), dim3(256), 0, S, ct, out, c->limbs_dev, A, P.ra, (u32)c->N, A.polys == 3 ? 2u : 1u);
    }
    if (P.path == KS_SUB) {
        // N = 2^15 / 2^16 on fp64-size moduli: per-sub-block fused key switch (k_ks_fused_sub) into T = dig ([batch][2][nw] rows,
        // level >= 2 makes room), then the inverse top stages over T together with the tail.  At 2^16 (X = 2) the four quarters
        // of a digit row stream through the LDS (dma_stream_load, no spills: 33.0 k against 32.1 k key switches/s for the
        // three-kernel path on 7 x 50 bit; with register loads the X = 2 load phase either spilled 237 registers or ran as 32
        // serial rounds: 26-28 k).  At 2^15 the register loads stay (the streamed form measured 36.2 k against 40.2 k, cfg#3).
        constexpr int LOGT = logt_for(14);
        const size_t lds = (size_t)lds_words<14, LOGT>() * 8;
        const int x = c->logN - 14;
        auto fk = x == 2 ? (P.fps ? k_ks_fused_sub<ArithFpS, 14, LOGT, 2> : k_ks_fused_sub<ArithFp, 14, LOGT, 2>)
                         : (P.fps ? k_ks_fused_sub<ArithFpS, 14, LOGT, 1> : k_ks_fused_sub<ArithFp, 14, LOGT, 1>);
        const unsigned items = (unsigned)((batch * nw) << x);
        rc = launch_prof(c, (int64_t)batch * nw * (level + 2), fk, dim3(cu_grid(c, items)), dim3(1 << LOGT), lds, key, ct, dig, c->limbs_dev, A, Lk, items);
        if (rc) return rc;
        // inverse top stage + "+ c" / special-prime contraction in one pass over the sub-block results
        return launch_top_tail(c, A, P.ra, dig, ct, out, batch, P.g_tail);
    }
    // the steps up to the inverse sub-block transforms stay on their lanes; the join comes before the tail, which reads every limb
    lanes_t outer(c, P.two_lanes);
    rc = ks_digits_fwd(c, A, ct, dig, batch);
    if (rc) return rc;
    rc = ks_inner_launch(c, A, Lk, key, dig, S, batch);
    if (rc) return rc;
    if (P.tail16) {
        // N = 2^16: the paired sub-block inverse into the (now free) digit buffer, then the two inverse top stages together with
        // the tail (k_ks_top_tail<2>) instead of k_ntt_inv_top<2> + k_ks_rescale_add / k_ks_add_ct.  Rings of mixed modulus sizes:
        // the larger limbs' sub-blocks come from the u64 block kernel (same sub-block layout, lazy [0, 2q) outputs).
        const policy_split_t ps = policy_split(c, A.w);
        const u32 fpm = ps.fpmask, amask = ps.all;
        {
            lanes_t lanes(c, fpm != amask);
            lanes.use(1);
            rc = launch_subpair<ArithFp>(c, true, S, dig, batch * 2 * nw, A.w, 2, fpm == amask ? 0u : fpm);
            if (rc) return rc;
            if (fpm != amask) {
                lanes.use(0);
                ntt_io_t iw = io_plain();
                iw.limb_mask = amask & ~fpm;
                rc = launch_block_inv<ArithInt, 14>(c, S, dig, batch * 2 * nw, A.w, 2, iw);
                if (rc) return rc;
            }
        }
        outer.join();
        return launch_top_tail(c, A, P.ra, dig, ct, out, batch, P.g_tail);
    }
    outer.join();
    return ks_plain_tail(c, A, P.ra, S, ct, out, batch);
}

static int ks_check(tfhe_ctx* c, int Lk, int level, int special, const void* evk, int n_digits, const void* ct, int polys, const void* out, int64_t batch) {
    if (!c || !evk || !ct || !out) return fail(TFHE_E_BADARG, "null argument");
    if (polys != 2 && polys != 3) return fail(TFHE_E_BADARG, "keyswitch needs a 2- or 3-element ciphertext (rlwe_she.jl:318), got %d", polys);
    if (Lk < 1 || Lk > c->L) return fail(TFHE_E_LEVEL_MISMATCH, "key_limbs=%d outside [1,%d]", Lk, c->L);
    const int maxlevel = special ? Lk - 1 : Lk;
    if (level < 1 || level > maxlevel) return fail(TFHE_E_LEVEL_MISMATCH, "level=%d outside [1,%d]", level, maxlevel);
    if (n_digits < level) return fail(TFHE_E_PARAMS_MISMATCH, "evaluation key has %d components, level %d needs %d", n_digits, level, level);
    if (batch < 0) return fail(TFHE_E_BADARG, "negative batch");
    return TFHE_OK;
}
// every entry point that takes a Galois element but tfhe_rotate
static int galois_check(const tfhe_ctx* c, u64 g) {
    if ((g & 1) == 0 || g >= 2 * (u64)c->N) return fail(TFHE_E_BADARG, "galois element must be odd and below 2N");
    return TFHE_OK;
}
static u64 inv_mod_2n(u64 g, u64 twoN) {  // g odd, twoN a power of two: Newton iteration
    u64 x = g;
    for (int i = 0; i < 6; i++) x *= 2 - g * x;
    return x & (twoN - 1);
}
// A key switch in two steps.  ks_prepare: the plan, the workspace and what is done to the KEY (k_evk_to_f64 on the fused paths,
// k_ntt_perm for a rotation finished in the tail) -- everything that depends on the key and the shape only.  ks_run: the ciphertexts.
// One preparation serves any number of runs of at most the prepared `batch` each with the same key (tfhe_bfv_mul_relin: one per
// chunk of its own pipeline).  `span`: a nested call's block -- its caller's region 0 -- instead of the context's own; without one the
// regions below, the key among them, are ours from the preparation to the last run only if no other entry point of this context runs
// between them (tfhe_bfv_mul_relin sees to that).
struct ks_prepared_t {
    ks_plan_t P;
    const u64* key;      // the caller's key, or the workspace copy
    u64 *S, *dig, *rot;
    u64 galois;
    int polys;
};
static int ks_prepare(tfhe_ctx* c, int Lk, int level, int special, const u64* evk, const u64* ct, int polys, const u64* out, int64_t batch,
                      u64 galois, bool rotate, bool prelifted, bool key_prepared, ks_prepared_t* K, const ws_span_t* span = nullptr) {
    if (prelifted && (rotate || special || !ks_prelift_ok(c, level))) return fail(TFHE_E_UNSUPPORTED, "internal: pre-lifted rows need the fused key switch");
    K->P = ks_plan(c, Lk, level, special, polys, batch, ct, out, galois, rotate, prelifted, key_prepared);
    ks_plan_t& P = K->P;
    K->key = evk; K->galois = galois; K->polys = polys;
    if (P.rot == KS_ROT_HOISTED) return TFHE_OK;   // the caller hands the call to tfhe_rotate_many
    if (special) special_inv_table(c, Lk, level, P.ra.qlinv);
    const size_t N = P.N;
    void* ws = nullptr;
    int rc = ws_begin(c, P.L, P.chunk, span, &ws, nullptr);   // (in force while the ciphertexts run: ks_run)
    if (rc) return rc;
    K->S = P.L.at(ws, P.chunk, P.rS); K->dig = P.L.at(ws, P.chunk, P.rdig); K->rot = P.L.at(ws, P.chunk, P.rrot);
    u64* const kw = P.L.at(ws, P.chunk, P.rkey);
    const u64 ginv = P.key_perm ? inv_mod_2n(galois, 2 * (u64)c->N) : (u64)0;
    if (P.path != KS_THREE) {
        rc = launch(c, k_evk_to_f64, row_grid((unsigned)(level * 2 * P.A.nw), N), dim3(256), 0, evk, kw, c->limbs_dev, P.A, Lk, (u32)N, c->logN <= 14 ? 1 : 0,
                    c->logN == 16 ? 2 : 0, ginv, 1);
    } else if (P.key_perm) {
        rc = launch(c, k_ntt_perm, row_grid((unsigned)(level * 2 * Lk), N), dim3(256), 0, evk, kw, ginv, (u32)N);
    }
    if (rc) return rc;
    if (P.path != KS_THREE || P.key_perm) K->key = kw;
    return TFHE_OK;
}
// `batch` ciphertexts (at most the prepared batch) by a prepared key switch
static int ks_run(tfhe_ctx* c, const ks_prepared_t& K, const u64* ct, u64* out, int64_t batch) {
    const ks_plan_t& P = K.P;
    const int level = P.A.level, polys = K.polys;
    const size_t N = P.N;
    const ws_scope_t scope(c->ws_scratch, P.L.region0(P.chunk));
    for (int64_t b0 = 0; b0 < batch; b0 += P.chunk) {
        const int64_t nb = std::min(P.chunk, batch - b0);
        const u64* cin = ct + (size_t)b0 * polys * level * N;
        if (P.rot == KS_ROT_COPY) {
            const int rc = do_galois(c, cin, K.rot, K.galois, nb * polys * level, first_limbs(level));
            if (rc) return rc;
            cin = K.rot;
        }
        const int rc = ks_chunk(c, P, K.key, cin, out + (size_t)b0 * 2 * level * N, nb, K.S, K.dig);
        if (rc) return rc;
    }
    return TFHE_OK;
}
static int rotate_many_run(tfhe_ctx* c, int Lk, int level, int special, const uint64_t* const* evks, int n_digits, int prepared, const uint64_t* galois,
                           int n_rot, const uint64_t* ct, uint64_t* out, int64_t batch, const ws_span_t* span);
static int keyswitch_impl(tfhe_ctx* c, int Lk, int level, int special, const u64* evk, const u64* ct, int polys, u64* out, int64_t batch,
                          u64 galois, bool rotate, bool prelifted = false, bool key_prepared = false, const ws_span_t* span = nullptr) {
    ks_prepared_t K;
    const int rc = ks_prepare(c, Lk, level, special, evk, ct, polys, out, batch, galois, rotate, prelifted, key_prepared, &K, span);
    if (rc) return rc;
    if (K.P.rot == KS_ROT_HOISTED) {
        const uint64_t* one[1] = {evk};
        return rotate_many_run(c, Lk, level, special, one, level, 1, &galois, 1, ct, out, batch, span);
    }
    return ks_run(c, K, ct, out, batch);
}

int tfhe_keyswitch(tfhe_ctx* c, int Lk, int level, int special, const uint64_t* evk, int n_digits, const uint64_t* ct, int polys, uint64_t* out, int64_t batch) {
    int rc = ks_check(c, Lk, level, special, evk, n_digits, ct, polys, out, batch);
    if (rc) return rc;
    return keyswitch_impl(c, Lk, level, special, evk, ct, polys, out, batch, 0, false);
}
// Hoisted rotations: rotate(gk_r, c) for r < n_rot from ONE digit decomposition.  The centred RNS digits commute with the
// automorphism (a signed permutation of coefficients; the centred representative of -x is the negative of that of x, q odd),
// and in the NTT domain the automorphism is the permutation galois_ntt_pos.  With the key rows permuted by g^-1 once per key
// (tfhe_galois_key_prepare) the inner product runs coalesced on the transformed digits of the UNrotated ciphertext and yields
// sigma_g^-1 of the sums; the automorphism is applied after the inverse transform, over 2 nw rows instead of level nw:
// level * nw forward transforms once instead of per rotation.  Bit-identical to n_rot calls of tfhe_rotate.
// evk_out = the Galois key of x -> x^g with every NTT-domain row permuted by g^-1 (tfhe_rotate_many with prepared = 1)
int tfhe_galois_key_prepare(tfhe_ctx* c, int Lk, int n_digits, uint64_t g, const uint64_t* evk, uint64_t* evk_out) {
    if (!c || !evk || !evk_out || evk == evk_out) return fail(TFHE_E_BADARG, "null or aliased argument");
    if (Lk < 1 || Lk > c->L || n_digits < 1) return fail(TFHE_E_LEVEL_MISMATCH, "key shape outside the ring");
    if (int rc = galois_check(c, g)) return rc;
    const u64 ginv = inv_mod_2n(g, 2 * (u64)c->N);
    return launch(c, k_ntt_perm, row_grid((unsigned)(n_digits * 2 * Lk), (size_t)c->N), dim3(256), 0, evk, evk_out, ginv, (u32)c->N);
}

// the workspace of the hoisted rotations for a call of `batch` ciphertexts (also read by whoever nests such a call in a span of its
// own, ks_rot_prepared_bytes): [ region 0: transform scratch (digits level nw rows, key sums 2 nw) | S: [chunk][2][nw][N] | digits:
// [chunk][level][nw][N] | T: [chunk][2][nw][N] | rotated input: [chunk][2][level][N] ], then one prepared key where the caller's are plain
struct rotate_many_ws_t {
    ws_layout_t L;
    ws_region_t S, dig, T, rot, keytmp;
    int64_t chunk;
};
static rotate_many_ws_t rotate_many_ws(const tfhe_ctx* c, int level, int nw, int64_t batch, size_t key_bytes) {
    rotate_many_ws_t W{};
    W.L = ws_layout_t((size_t)c->N);
    W.L.scratch((size_t)std::max(2, level) * nw);
    W.S = W.L.rows((size_t)2 * nw); W.dig = W.L.rows((size_t)level * nw); W.T = W.L.rows((size_t)2 * nw); W.rot = W.L.rows((size_t)2 * level);
    W.keytmp = W.L.tail(key_bytes);
    W.chunk = chunk_of(c, batch, 512, (size_t)8192 << 20, W.L.per_ct_bytes());
    return W;
}
// the span a prepared-key rotation of `batch` ciphertexts may ask of its caller (matmul_bsgs_run, whose operands are its own: disjoint
// and aligned): the larger of the two routes ks_plan picks between by the batch -- finished in the tail, or handed to the hoisted form
static size_t ks_rot_prepared_bytes(const tfhe_ctx* c, int Lk, int level, int special, int64_t batch) {
    const ks_plan_t P = ks_plan(c, Lk, level, special, 2, batch, nullptr, nullptr, 1, true, false, true);   // (KS_ROT_HOISTED: an empty layout)
    const rotate_many_ws_t W = rotate_many_ws(c, level, special ? level + 1 : level, batch, 0);
    return std::max(P.L.bytes(P.chunk), W.L.bytes(W.chunk));
}
int tfhe_rotate_many(tfhe_ctx* c, int Lk, int level, int special, const uint64_t* const* evks, int n_digits, int prepared,
                     const uint64_t* galois, int n_rot, const uint64_t* ct, uint64_t* out, int64_t batch) {
    if (!evks || !galois || n_rot < 0) return fail(TFHE_E_BADARG, "null argument");
    if (n_rot == 0) return TFHE_OK;
    for (int r = 0; r < n_rot; r++) {
        int rc = ks_check(c, Lk, level, special, evks[r], n_digits, ct, 2, out, batch);
        if (!rc) rc = galois_check(c, galois[r]);
        if (rc) return rc;
    }
    return rotate_many_run(c, Lk, level, special, evks, n_digits, prepared, galois, n_rot, ct, out, batch, nullptr);
}
// the rotations after the host checks; `span`: a nested call's block instead of the context's own (keyswitch_impl)
static int rotate_many_run(tfhe_ctx* c, int Lk, int level, int special, const uint64_t* const* evks, int n_digits, int prepared, const uint64_t* galois,
                           int n_rot, const uint64_t* ct, uint64_t* out, int64_t batch, const ws_span_t* span) {
    const int nw = special ? level + 1 : level, polys = 2;
    const size_t N = (size_t)c->N;
    if (!prepared && c->logN <= 14 && ks_fused14(c, Lk, level, special)) {
        // N = 2^14 on fp64-size moduli: the fused key switch (digits never leave the registers) beats the hoisted three-kernel
        // path (measured 126 k against 110 k rotations/s at 6 limbs + special prime) -- same bits either way
        for (int r = 0; r < n_rot; r++) {
            int rc = keyswitch_impl(c, Lk, level, special, evks[r], ct, 2, out + (size_t)r * batch * 2 * level * N, batch, galois[r], true, false, false, span);
            if (rc) return rc;
        }
        return TFHE_OK;
    }
    const ks_arg_t A = make_ks_arg(Lk, level, special, polys);
    const rotate_many_ws_t W = rotate_many_ws(c, level, nw, batch, prepared ? 0 : (size_t)n_digits * 2 * Lk * N * 8);
    const int64_t chunk = W.chunk;
    void* ws = nullptr;
    ws_scope_t scope;
    int rc = ws_begin(c, W.L, chunk, span, &ws, &scope);
    if (rc) return rc;
    u64 *S = W.L.at(ws, chunk, W.S), *dig = W.L.at(ws, chunk, W.dig), *T = W.L.at(ws, chunk, W.T), *rot = W.L.at(ws, chunk, W.rot);
    u64* keytmp = W.L.at(ws, chunk, W.keytmp);
    const limb_sel_t sl = first_limbs(level);
    rescale_arg_t ra{};
    if (special) special_inv_table(c, Lk, level, ra.qlinv);
    auto tail_grid = [&](int64_t nb) { return row_grid((unsigned)(nb * 2 * level), N); };
    for (int64_t b0 = 0; b0 < batch; b0 += chunk) {
        const int64_t nb = std::min(chunk, batch - b0);
        const u64* cin = ct + (size_t)b0 * polys * level * N;
        rc = ks_digits_fwd(c, A, cin, dig, nb);
        if (rc) return rc;
        for (int r = 0; r < n_rot; r++) {
            const u64* key = evks[r];
            if (!prepared) {
                rc = tfhe_galois_key_prepare(c, Lk, n_digits, galois[r], evks[r], keytmp);
                if (rc) return rc;
                key = keytmp;
            }
            rc = do_galois(c, cin, rot, galois[r], nb * polys * level, sl);   // the addend sigma_g(c_1) (and sigma_g(c_2), unused)
            if (rc) return rc;
            // key sums up to the key's permutation, S' = sigma_g^-1(S); the automorphism is applied to INTT(S') BEFORE the tail (the
            // ModulusRaised floor does not commute with sign changes), into T -- not over the digits, which the next rotation reuses
            u64* const o = out + ((size_t)r * batch + b0) * 2 * level * N;
            rc = ks_inner_launch(c, A, Lk, key, dig, S, nb);
            if (rc) return rc;
            rc = run_ntt(c, true, S, S, nb * 2 * nw, A.w);
            if (rc) return rc;
            rc = do_galois(c, S, T, galois[r], nb * 2 * nw, A.w);
            if (rc) return rc;
            if (special) {
                rc = launch(c, k_ks_rescale_add, tail_grid(nb), dim3(256), 0, T, rot, o, c->limbs_dev, A, ra, (u32)N, 1u);
            } else {
                HIP_TRY(hipMemcpyAsync(o, T, (size_t)nb * 2 * level * N * 8, hipMemcpyDeviceToDevice, c->stream));
                rc = launch(c, k_ks_add_ct, tail_grid(nb), dim3(256), 0, rot, o, c->limbs_dev, A, (u32)N, 1u);
            }
            if (rc) return rc;
        }
    }
    return TFHE_OK;
}

int tfhe_rotate(tfhe_ctx* c, int Lk, int level, int special, const uint64_t* evk, int n_digits, uint64_t g, const uint64_t* ct, uint64_t* out, int64_t batch) {
    int rc = ks_check(c, Lk, level, special, evk, n_digits, ct, 2, out, batch);
    if (rc) return rc;
    if ((g & 1) == 0) return fail(TFHE_E_BADARG, "galois element must be odd");   // deliberately not galois_check: this entry point never bounded g
    return keyswitch_impl(c, Lk, level, special, evk, ct, 2, out, batch, g, true);
}
// the same with the key as tfhe_galois_key_prepare left it (r06): a caller that rotates by ONE Galois element again and again
// (infer.jl:140-149: 63 chained rotations per matrix product, one key) prepares it once instead of once per call
int tfhe_rotate_prepared(tfhe_ctx* c, int Lk, int level, int special, const uint64_t* evk_prepared, int n_digits, uint64_t g, const uint64_t* ct, uint64_t* out,
                         int64_t batch) {
    int rc = ks_check(c, Lk, level, special, evk_prepared, n_digits, ct, 2, out, batch);
    if (rc) return rc;
    if ((rc = galois_check(c, g))) return rc;
    return keyswitch_impl(c, Lk, level, special, evk_prepared, ct, 2, out, batch, g, true, false, true);
}

// ---- digit-window key switch (relin_window != 0, rlwe_she.jl:330-338) -----------------------------------------------
static int ksw_table(tfhe_ctx* c, int level, const conv_tab_t** out) {
    *out = nullptr;
    if (level == 1) return TFHE_OK;
    std::lock_guard<std::mutex> g(c->ksw_mu);
    auto it = c->ksw_tabs.find(level);
    if (it != c->ksw_tabs.end()) { *out = it->second; return TFHE_OK; }
    conv_host_t H;
    build_conv_host(std::vector<u64>(c->q.begin(), c->q.begin() + level), std::vector<u64>(), &H);
    conv_tab_t T = H.tab;
    auto up = [&](const std::vector<u64>& v, const u64** d) -> bool {
        *d = nullptr;
        if (v.empty()) return true;
        void* p = nullptr;
        if (devalloc::malloc_retry(&p, v.size() * 8) != hipSuccess) return false;
        c->ksw_allocs.push_back(p);
        if (hipMemcpy(p, v.data(), v.size() * 8, hipMemcpyHostToDevice) != hipSuccess) return false;
        *d = (const u64*)p;
        return true;
    };
    void* dt = nullptr;
    if (!up(H.C, &T.C) || !up(H.M, &T.M) || !up(H.Aw, &T.Aw) || devalloc::malloc_retry(&dt, sizeof T) != hipSuccess)
        return fail(TFHE_E_NOMEM, "allocating the window-digit tables failed");
    c->ksw_allocs.push_back(dt);
    HIP_TRY(hipMemcpy(dt, &T, sizeof T, hipMemcpyHostToDevice));
    c->ksw_tabs[level] = (conv_tab_t*)dt;
    *out = (conv_tab_t*)dt;
    return TFHE_OK;
}

int tfhe_keyswitch_window(tfhe_ctx* c, int key_limbs, int level, int special, int window_bits, const uint64_t* evk, int n_windows,
                          const uint64_t* ct, int polys, uint64_t* out, int64_t batch) {
    if (!c || !evk || !ct || !out) return fail(TFHE_E_BADARG, "null argument");
    if (polys != 2 && polys != 3) return fail(TFHE_E_BADARG, "keyswitch needs a 2- or 3-element ciphertext (rlwe_she.jl:318), got %d", polys);
    const int Lk = key_limbs;
    if (Lk < 1 || Lk > c->L) return fail(TFHE_E_BADARG, "key_limbs=%d outside [1,%d]", Lk, c->L);
    if (level < 1 || level > (special ? Lk - 1 : Lk)) return fail(TFHE_E_LEVEL_MISMATCH, "level=%d outside [1,%d]", level, special ? Lk - 1 : Lk);
    if (batch < 0) return fail(TFHE_E_BADARG, "negative batch");
    hostmath::bigint Q = hostmath::big_from(1);
    u64 qmin = special ? c->q[Lk - 1] : ~0ull;
    for (int j = 0; j < level; j++) { Q = hostmath::big_mul_u64(Q, c->q[j]); qmin = std::min(qmin, c->q[j]); }
    if (window_bits < 1 || window_bits > 32 || (qmin >> window_bits) == 0)
        return fail(TFHE_E_BADARG, "window of %d bits: need 1 <= w <= 32 and 2^w below every modulus", window_bits);
    int qbits = 0;
    for (int w = (int)Q.size() - 1; w >= 0 && !qbits; w--)
        if (Q[w]) qbits = w * 64 + hostmath::bitlen(Q[w]);
    // ndigits(modulus of the CIPHERTEXT ring, base = 2^w), rlwe_she.jl:333; a key made for a larger ring (a higher level, or the
    // ModulusRaised key ring Q P, modulusraising.jl:28-32) has more components: the loop rlwe_she.jl:340 uses the first `need`
    const int need = (qbits + window_bits - 1) / window_bits;
    if (n_windows < need)
        return fail(TFHE_E_PARAMS_MISMATCH, "evaluation key has %d components, a %d-bit modulus in %d-bit windows has %d digits", n_windows, qbits, window_bits, need);
    if (batch == 0) return TFHE_OK;
    const conv_tab_t* T = nullptr;
    int rc = ksw_table(c, level, &T);
    if (rc) return rc;
    const size_t N = (size_t)c->N;
    const u32 n = (u32)c->N;
    const int nw = special ? level + 1 : level;  // working limbs: [0 .. level-1] (+ the special prime, downswitch_keyelement modulusraising.jl:43-49)
    // workspace: [ region 0: transform scratch (the digits' transforms; need >= 2) | S: [chunk][2][nw][N] | digits: [chunk][need][nw][N] ]
    ws_layout_t L(N);
    L.scratch((size_t)need * nw);
    const ws_region_t rS = L.rows((size_t)2 * nw), rdig = L.rows((size_t)need * nw);
    const int64_t chunk = chunk_of(c, batch, 512, (size_t)8192 << 20, L.per_ct_bytes());
    void* ws = nullptr;
    ws_scope_t scope;
    rc = ws_begin(c, L, chunk, nullptr, &ws, &scope);
    if (rc) return rc;
    u64 *S = L.at(ws, chunk, rS), *dig = L.at(ws, chunk, rdig);
    const ks_arg_t Al = make_ks_arg(Lk, level, special ? 1 : 0, polys);  // row bookkeeping of the tail kernels: `level` = ciphertext limbs
    ks_arg_t A = Al;   // inner product: `level` field = number of digits, nw = working limbs
    A.level = need;
    const unsigned gx = (n + 255) / 256;
    rescale_arg_t ra{};
    if (special) special_inv_table(c, Lk, level, ra.qlinv);
    for (int64_t b0 = 0; b0 < batch; b0 += chunk) {
        const int64_t nb = std::min(chunk, batch - b0);
        const u64* cin = ct + (size_t)b0 * polys * level * N;
        u64* cout = out + (size_t)b0 * 2 * level * N;
        rc = launch(c, k_ks_window_digits, dim3((unsigned)(nb * gx)), dim3(256), 0, cin, dig, T, level, window_bits, need, polys, n, gx, nw);
        if (rc) return rc;
        rc = run_ntt(c, false, dig, dig, nb * need * nw, A.w);
        if (rc) return rc;
        const unsigned bsplit = (unsigned)std::max<int64_t>(1, std::min<int64_t>(nb, (4096 + nw * gx - 1) / (nw * gx)));
        rc = launch(c, k_ks_inner<8>, dim3((unsigned)nw * gx * bsplit), dim3(256), 0, evk, dig, S, c->limbs_dev, A, Lk, n, (u32)nb, bsplit, 0u, ks_keys_t{});
        if (rc) return rc;
        // with the special prime, ModulusRaised: c1 = P c + S over [q_0 .. q_{level-1}, P], contracted by modswitch
        // (modulusraising.jl:35-42): out_j = c_j + (T_j - [T_P]) P^-1 with T = INTT(S)  (the tail of the RNS-digit path)
        rc = ks_plain_tail(c, Al, ra, S, cin, cout, nb);
        if (rc) return rc;
    }
    return TFHE_OK;
}

// ---- key switch with grouped RNS digits and several special primes ("hybrid" gadget) ---------------------------------------
// Digit g = the centred representative of c[end] modulo Q_g = prod of the limbs [g group, min((g+1) group, level)) (signedmod.jl:12-19;
// switch(ℛ_W, .) of bfv.jl:202-226 on the group's sub-ring; one limb per group: rlwe_she.jl:326-329), in every working limb
// W = [0 .. level-1] ∪ [key_limbs - n_special .. key_limbs - 1];  S_s = P c_s ⊕ zeros + sum_g key_{g,s} digit_g over W;  out_s =
// modswitch (crt.jl:215-228) applied n_special times, the last special prime first = c_s + the contraction of INTT(sum_g ...).
//   k_ks_group_digits -> run_ntt over W -> ks_inner_launch (A.level = digits, A.w = W) -> run_ntt -> k_ks_group_tail
// workspace: [ region 0: transform scratch | S: [chunk][2][nw][N] | digits: [chunk][d][nw][N] | rotated copy: [chunk][2][level][N] ]
struct ksg_plan_t {
    ks_group_arg_t G;
    ks_arg_t A;          // the key sums: A.level = digits
    ks_arg_t At;         // n_special == 0: the row bookkeeping of ks_plain_tail (level = ciphertext limbs)
    int Lk;
    const conv_tab_t* tabs;
    int64_t chunk;       // of ksg_impl; who carves the regions from a block of its own brings its own (tfhe_mul_relin_grouped)
    size_t N;
    ws_layout_t L;
    ws_region_t S, dig, rot;
};
// one conv_tab_t per digit (source: the group cut at this level, targets: W), built on first use and kept with the context
static int ksg_table(tfhe_ctx* c, int Lk, int level, int k, int group, const conv_tab_t** out) {
    *out = nullptr;
    std::lock_guard<std::mutex> g(c->ksw_mu);
    const std::array<int, 4> key{Lk, level, k, group};
    auto it = c->ksg_tabs.find(key);
    if (it != c->ksg_tabs.end()) { *out = it->second; return TFHE_OK; }
    const limb_sel_t w = working_limbs_k(Lk, level, k);
    std::vector<u64> targets;
    for (int j = 0; j < w.n; j++) targets.push_back(c->q[w.idx[j]]);
    const int d = (level + group - 1) / group;
    std::vector<conv_tab_t> tabs((size_t)d);
    auto up = [&](const void* src, size_t bytes, const void** dev) -> bool {
        void* p = nullptr;
        if (devalloc::malloc_retry(&p, bytes) != hipSuccess) return false;
        c->ksw_allocs.push_back(p);
        if (hipMemcpy(p, src, bytes, hipMemcpyHostToDevice) != hipSuccess) return false;
        *dev = p;
        return true;
    };
    for (int gi = 0; gi < d; gi++) {
        const int lo = gi * group, hi = std::min(lo + group, level);
        conv_host_t H;
        build_conv_host(std::vector<u64>(c->q.begin() + lo, c->q.begin() + hi), targets, &H);
        conv_tab_t T = H.tab;
        if (!up(H.C.data(), H.C.size() * 8, (const void**)&T.C) || !up(H.M.data(), H.M.size() * 8, (const void**)&T.M) ||
            !up(H.Aw.data(), H.Aw.size() * 8, (const void**)&T.Aw)) {
            (void)hipGetLastError();
            return fail(TFHE_E_NOMEM, "allocating the grouped-digit tables failed");
        }
        tabs[(size_t)gi] = T;
    }
    const void* dt = nullptr;
    if (!up(tabs.data(), tabs.size() * sizeof(conv_tab_t), &dt)) {
        (void)hipGetLastError();
        return fail(TFHE_E_NOMEM, "allocating the grouped-digit tables failed");
    }
    c->ksg_tabs[key] = (conv_tab_t*)dt;
    *out = (const conv_tab_t*)dt;
    return TFHE_OK;
}
static int ksg_plan(tfhe_ctx* c, int Lk, int level, int k, int group, int polys, int64_t batch, bool rotate, ksg_plan_t* P) {
    const int d = (level + group - 1) / group, nw = level + k;
    P->Lk = Lk; P->N = (size_t)c->N;
    ks_group_arg_t& G = P->G;
    G = ks_group_arg_t{};
    G.level = level; G.nw = nw; G.k = k; G.polys = polys; G.group = group; G.d = d;
    G.w = working_limbs_k(Lk, level, k);
    // inv[t][j] = p_t^-1 mod working limb j, for the limbs step t still holds (j < level + t)
    for (int t = 0; t < k; t++) {
        const u64 p = c->q[G.w.idx[level + t]];
        for (int j = 0; j < level + t; j++) {
            const u64 qj = c->q[G.w.idx[j]];
            G.inv[t][j] = hostmath::make_tw(hostmath::invmod_prime(p % qj, qj), qj);
        }
    }
    P->A = make_ks_arg_grouped(Lk, level, k, d, polys);
    P->At = make_ks_arg(Lk, level, 0, polys);
    P->L = ws_layout_t(P->N);
    P->L.scratch((size_t)std::max(2, d) * nw);   // the digits' transforms (d nw rows), the key sums' inverse (2 nw)
    P->S = P->L.rows((size_t)2 * nw); P->dig = P->L.rows((size_t)d * nw); P->rot = P->L.rows(rotate ? (size_t)2 * level : 0);
    P->chunk = chunk_of(c, batch, 512, (size_t)8192 << 20, P->L.per_ct_bytes());
    return ksg_table(c, Lk, level, k, group, &P->tabs);
}
// the digits of `batch` ciphertexts, transformed: dig [batch][d][nw][N], NTT domain; v2: two coefficients per thread
static int ksg_digits_fwd(tfhe_ctx* c, const ksg_plan_t& P, const u64* ct, u64* dig, int64_t batch, bool v2) {
    const ks_group_arg_t& G = P.G;
    const u32 n = (u32)c->N;
    const u32 gx = v2 ? (n / 2 + 255) / 256 : (n + 255) / 256;
    const dim3 dgrid((unsigned)(batch * G.d * gx));
    const int rc = dispatch_int<0, 4>(G.group <= 4 ? G.group : 0, [&](auto gc) {
        constexpr int GG = decltype(gc)::value;
        return v2 ? launch(c, k_ks_group_digits<GG, 2>, dgrid, dim3(256), 0, ct, dig, P.tabs, G, n, gx)
                  : launch(c, k_ks_group_digits<GG, 1>, dgrid, dim3(256), 0, ct, dig, P.tabs, G, n, gx);
    });
    if (rc) return rc;
    return run_ntt(c, false, dig, dig, batch * G.d * G.nw, P.A.w);
}
// one chunk of `batch` ciphertexts: `ct` the chunk's input (the rotated copy for a rotation).  The caller hands over the plan and its
// carved regions S and dig, with the plan's region 0 in force, so whoever has sized ONE block for several users (tfhe_mul_relin_grouped)
// runs the chunk without a second allocation.  rs (n_special >= 1, a 3-element input): the modswitch of both components rides on the tail -- out: [batch][2][level - 1][N]
static int ksg_chunk(tfhe_ctx* c, const ksg_plan_t& P, const u64* evk, const u64* ct, u64* out, int64_t batch, u64* S, u64* dig,
                     const ks_group_rescale_t* rs = nullptr) {
    const ks_group_arg_t& G = P.G;
    const u32 n = (u32)c->N;
    // two coefficients per thread (16-byte loads and stores) where the rows allow it
    const bool v2 = n % 2 == 0 && (((uintptr_t)ct | (uintptr_t)out) & 15u) == 0;
    const u32 gx = v2 ? (n / 2 + 255) / 256 : (n + 255) / 256;
    const dim3 tgrid((unsigned)(batch * 2 * gx));
    int rc = ksg_digits_fwd(c, P, ct, dig, batch, v2);
    if (rc) return rc;
    rc = ks_inner_launch(c, P.A, P.Lk, evk, dig, S, batch);
    if (rc) return rc;
    if (G.k == 0) return rs ? fail(TFHE_E_UNSUPPORTED, "internal: no special prime, no tail for the rescale to ride on")
                            : ks_plain_tail(c, P.At, rescale_arg_t{}, S, ct, out, batch);
    rc = run_ntt(c, true, S, S, batch * 2 * G.nw, P.A.w);
    if (rc) return rc;
    if (rs) {
        if (G.polys != 3 || G.level < 2) return fail(TFHE_E_UNSUPPORTED, "internal: the rescaling tail takes a 3-element input of two limbs or more");
        return dispatch_int<1, TFHE_KSG_MAX_SPECIAL>(G.k, [&](auto kc) {
            constexpr int K = decltype(kc)::value;
            return v2 ? launch(c, k_ks_group_tail_rescale<K, 2>, tgrid, dim3(256), 0, (const u64*)S, ct, out, c->limbs_dev, G, *rs, n, gx)
                      : launch(c, k_ks_group_tail_rescale<K, 1>, tgrid, dim3(256), 0, (const u64*)S, ct, out, c->limbs_dev, G, *rs, n, gx);
        });
    }
    const u32 add_s = G.polys == 3 ? 2u : 1u;   // c2 starts from zero for a 2-element input (rlwe_she.jl:324)
    return dispatch_int<1, TFHE_KSG_MAX_SPECIAL>(G.k, [&](auto kc) {
        constexpr int K = decltype(kc)::value;
        return v2 ? launch(c, k_ks_group_tail<K, 2>, tgrid, dim3(256), 0, (const u64*)S, ct, out, c->limbs_dev, G, n, gx, add_s)
                  : launch(c, k_ks_group_tail<K, 1>, tgrid, dim3(256), 0, (const u64*)S, ct, out, c->limbs_dev, G, n, gx, add_s);
    });
}
static int ksg_check(tfhe_ctx* c, int Lk, int level, int k, int group, const void* evk, int n_digits, const void* ct, int polys, const void* out,
                     int64_t batch, bool rotate, u64 galois) {
    char msg[160];
    const int rc = ks_group_check(!c || !evk || !ct || !out, c ? c->L : 0, c ? c->N : 0, Lk, level, k, group, n_digits, polys, batch, rotate, galois,
                                  msg, sizeof msg);
    return rc ? fail(rc, "%s", msg) : TFHE_OK;
}
static int ksg_impl(tfhe_ctx* c, int Lk, int level, int k, int group, const u64* evk, const u64* ct, int polys, u64* out, int64_t batch, u64 galois,
                    bool rotate) {
    if (batch == 0) return TFHE_OK;
    group = std::min(group, level);   // (one digit: every larger group is the whole ciphertext ring)
    ksg_plan_t P;
    int rc = ksg_plan(c, Lk, level, k, group, polys, batch, rotate, &P);
    if (rc) return rc;
    void* ws = nullptr;
    ws_scope_t scope;
    rc = ws_begin(c, P.L, P.chunk, nullptr, &ws, &scope);
    if (rc) return rc;
    u64 *S = P.L.at(ws, P.chunk, P.S), *dig = P.L.at(ws, P.chunk, P.dig), *rot = P.L.at(ws, P.chunk, P.rot);
    const size_t N = P.N;
    for (int64_t b0 = 0; b0 < batch; b0 += P.chunk) {
        const int64_t nb = std::min(P.chunk, batch - b0);
        const u64* cin = ct + (size_t)b0 * polys * level * N;
        if (rotate) {   // KS_ROT_COPY: apply_galois_element into the workspace, then the key switch of the copy
            rc = do_galois(c, cin, rot, galois, nb * polys * level, first_limbs(level));
            if (rc) return rc;
            cin = rot;
        }
        rc = ksg_chunk(c, P, evk, cin, out + (size_t)b0 * 2 * level * N, nb, S, dig);
        if (rc) return rc;
    }
    return TFHE_OK;
}
int tfhe_keyswitch_grouped(tfhe_ctx* c, int key_limbs, int level, int n_special, int group, const uint64_t* evk, int n_digits, const uint64_t* ct,
                           int polys, uint64_t* out, int64_t batch) {
    const int rc = ksg_check(c, key_limbs, level, n_special, group, evk, n_digits, ct, polys, out, batch, false, 0);
    if (rc) return rc;
    return ksg_impl(c, key_limbs, level, n_special, group, evk, ct, polys, out, batch, 0, false);
}
int tfhe_rotate_grouped(tfhe_ctx* c, int key_limbs, int level, int n_special, int group, const uint64_t* evk, int n_digits, uint64_t galois_element,
                        const uint64_t* ct, uint64_t* out, int64_t batch) {
    const int rc = ksg_check(c, key_limbs, level, n_special, group, evk, n_digits, ct, 2, out, batch, true, galois_element);
    if (rc) return rc;
    return ksg_impl(c, key_limbs, level, n_special, group, evk, ct, 2, out, batch, galois_element, true);
}

// ---- hoisted rotations on grouped-digit keys -------------------------------------------------------------------------------------
// out[r] = tfhe_rotate_grouped(key_r, g_r, ct) for every r from ONE digit decomposition: the grouped digit is the centred
// representative modulo the odd Q_g -- no tie, a symmetric range, centred(-x) = -centred(x) -- so it commutes with the signed
// permutation sigma_g in every working limb, and the identity of tfhe_rotate_many carries over: the key sums of the UNROTATED digits
// against the key permuted by g^-1 (tfhe_galois_key_prepare, which does not care what a digit is) are sigma_g^-1 of the sums, and
// sigma_g is applied to INTT(S') BEFORE the K-step contraction, whose floor does not commute with sign changes (k_ks_group_rot_tail).
//   k_ks_group_digits on ct itself -> run_ntt over d nw rows, once -> per tile of up to 64 keys (ks_keys_t, ks_group_rot_t):
//   ks_inner_launch against all the tile's keys -> run_ntt inverse over n_tile 2 nw rows -> k_ks_group_rot_tail, every rotation at once
// d nw forward transforms per ciphertext instead of per rotation, no rotated copies.  Shared with tfhe_matmul_diag_grouped (md_api.inc).
struct ksg_hoist_t {
    ksg_plan_t P;        // G, A, the digit tables (its layout is the single key switch's: unused here)
    int R_tile;          // keys per launch
    size_t dig_rows, S_rows;   // rows (N words) per ciphertext: digits d nw, key sums R_tile 2 nw
};
static int ksg_hoist_plan(tfhe_ctx* c, int Lk, int level, int k, int group, int n_rot, ksg_hoist_t* H) {
    group = std::min(group, level);   // (one digit: every larger group is the whole ciphertext ring)
    const int rc = ksg_plan(c, Lk, level, k, group, 2, 1, false, &H->P);
    if (rc) return rc;
    H->R_tile = std::min(n_rot, TFHE_DOT_MAX);
    H->dig_rows = (size_t)H->P.G.d * H->P.G.nw;
    H->S_rows = (size_t)H->R_tile * 2 * H->P.G.nw;
    return TFHE_OK;
}
// rotations r0 .. r0 + n_tile - 1 of one chunk from its transformed digits: dst[r][b][s][level][N], r local to the tile, rotations
// dst_stride words apart
static int ksg_hoist_tile(tfhe_ctx* c, const ksg_hoist_t& H, const uint64_t* const* evks, const uint64_t* galois, int n_tile, const u64* cin,
                          int64_t nb, const u64* dig, u64* S, u64* dst, size_t dst_stride) {
    const ksg_plan_t& P = H.P;
    int rc = ks_inner_launch(c, P.A, P.Lk, nullptr, dig, S, nb, evks, n_tile);
    if (rc) return rc;
    rc = run_ntt(c, true, S, S, (int64_t)n_tile * nb * 2 * P.G.nw, P.A.w);
    if (rc) return rc;
    ks_group_rot_t R{};
    for (int r = 0; r < n_tile; r++) R.g[r] = galois[r];
    R.out_stride = dst_stride;
    return dispatch_int<0, TFHE_KSG_MAX_SPECIAL>(P.G.k, [&](auto kc) {
        return launch(c, k_ks_group_rot_tail<decltype(kc)::value>, dim3(8 * TFHE_ROT_TAIL_SLOTS), dim3(256), 0, (const u64*)S, cin, dst, c->limbs_dev,
                      P.G, R, (u32)c->N, (u32)nb, (u32)((int64_t)n_tile * nb * 2));
    });
}
static int ksg_many_check(tfhe_ctx* c, bool product, int Lk, int level, int k, int group, const uint64_t* const* evks, int n_digits,
                          const uint64_t* galois, int n_rot, const void* diags, const void* ct, const void* out, int64_t batch, bool* nothing_to_do) {
    char msg[160];
    const int rc = ks_group_many_check(product, !c || !evks || !galois || !ct || !out || (product && !diags), c ? c->L : 0, c ? c->N : 0, Lk, level, k,
                                       group, n_digits, batch, evks, galois, n_rot, (uintptr_t)ct, (uintptr_t)out, (uintptr_t)diags, nothing_to_do, msg,
                                       sizeof msg, TFHE_DOT_MAX);
    return rc ? fail(rc, "%s", msg) : TFHE_OK;
}
// workspace: [ region 0: transform scratch (the larger of the two regions' rows) | digits: [chunk][d][nw][N] | S: [chunk][R_tile][2][nw][N] ]
int tfhe_rotate_many_grouped(tfhe_ctx* c, int key_limbs, int level, int n_special, int group, const uint64_t* const* evks, int n_digits,
                             const uint64_t* galois_elements, int n_rot, const uint64_t* ct, uint64_t* out, int64_t batch) {
    bool nothing = false;
    int rc = ksg_many_check(c, false, key_limbs, level, n_special, group, evks, n_digits, galois_elements, n_rot, nullptr, ct, out, batch, &nothing);
    if (rc || nothing) return rc;
    ksg_hoist_t H;
    rc = ksg_hoist_plan(c, key_limbs, level, n_special, group, n_rot, &H);
    if (rc) return rc;
    const size_t N = (size_t)c->N, ct_words = (size_t)2 * level * N;
    ws_layout_t L(N);
    L.scratch(std::max(H.dig_rows, H.S_rows));
    const ws_region_t rdig = L.rows(H.dig_rows), rS = L.rows(H.S_rows);
    const int64_t chunk = chunk_of(c, batch, 512, (size_t)8192 << 20, L.per_ct_bytes());
    void* ws = nullptr;
    ws_scope_t scope;
    rc = ws_begin(c, L, chunk, nullptr, &ws, &scope);
    if (rc) return rc;
    u64 *const dig = L.at(ws, chunk, rdig), *const S = L.at(ws, chunk, rS);
    for (int64_t b0 = 0; b0 < batch; b0 += chunk) {
        const int64_t nb = std::min(chunk, batch - b0);
        const u64* cin = ct + (size_t)b0 * ct_words;
        rc = ksg_digits_fwd(c, H.P, cin, dig, nb, N % 2 == 0 && ((uintptr_t)cin & 15u) == 0);
        if (rc) return rc;
        for (int r0 = 0; r0 < n_rot; r0 += H.R_tile) {
            const int n_tile = std::min(H.R_tile, n_rot - r0);
            // straight into the caller's array: rotations a whole batch apart, the chunk at its place in each
            rc = ksg_hoist_tile(c, H, evks + r0, galois_elements + r0, n_tile, cin, nb, dig, S, out + ((size_t)r0 * batch + b0) * ct_words,
                                (size_t)batch * ct_words);
            if (rc) return rc;
        }
    }
    return TFHE_OK;
}
