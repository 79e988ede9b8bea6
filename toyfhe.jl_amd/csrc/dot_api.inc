// dot_api.inc -- tfhe_dot_plain: dst_i = (acc_i +) sum_k T_k(a[k]_i) .* b[k]_i over VIEW operands (base + i * stride), T_k the
// forward transform or the identity per term: the accumulation of the diagonal matrix product (infer.jl:140-149) over rotated
// ciphertexts that are still in the coefficient domain, in one call; included by toyfhe_hip.hip.
//
// Routing (dot_plan, decided once per call):
//   N = 2^12 .. 2^14, variant 0, <= 32 limbs : k_dot_plain_fused (dot_core.h), one (item, limb) row per workgroup pass, the transforms
//                                              inside the sum; a ring that mixes the policies runs one launch per policy on the two
//                                              lanes (the size test, the lanes and the launch: toyfhe_hip.hip, "the fused row kernels").
//                                              A pass with fewer rows than the chip has workgroup slots is split over its terms too
//                                              (dot_split: partial sums in the context workspace, added onto dst by k_dot_join)
//   everything else                          : per pass, the coefficient-domain terms are gathered from their views into the context
//                                              workspace (one strided copy each), transformed by ONE batched transform, and
//                                              accumulated by k_dot_view, which reads transformed terms and plaintexts where they lie
// A pass takes at most TFHE_DOT_MAX terms of at most `items` items; later passes of an item range accumulate onto dst (residues are
// canonical, so the partial sums are the words of one pass over all terms).  The composed path's workspace
//       [ transform scratch (N > 2^14) 1 | gathered coefficients 1 | images 1 ]  x terms x items x limbs x N words
// is bounded by chunk_of's byte cap: the terms of a pass are cut first, the items second.  tfhe_ctx_set_chunk bounds both.
// Every path leaves canonical residues: the words are those of tfhe_nntt followed by tfhe_mad term by term.

namespace {

struct dot_plan {
    bool fused;
    int terms;             // of one pass
    int64_t items;         // of one pass
    size_t row;            // words of one item: limbs x N
    size_t scratch_rows;   // composed: workspace slots in front of the gathered coefficients, per (term, item)
    size_t ws_bytes;       // the workspace of one pass: composed, the gathered terms and their images; fused, the partial sums (0: none)
    int64_t fill;          // fused: the workgroups that are co-resident on the chip
};

dot_plan dot_plan_for(const tfhe_ctx* c, int n_terms, int n_coef, int64_t count, int limbs) {
    dot_plan p{};
    p.fused = fused_rows_ok(c, limbs);
    p.row = (size_t)limbs * (size_t)c->N;
    if (p.fused) {
        p.terms = (int)chunk_of(c, n_terms, TFHE_DOT_MAX);
        p.items = chunk_of(c, count, ENC_CHUNK);
        // what launch_fused_rows' grid holds at once: persistent_grid's workgroups per CU for the padded row as LDS image (4 / 2 / 1
        // at 2^12 / 2^13 / 2^14; the kernels' registers admit as many: 128 VGPRs x 4 waves, 242 x 4 waves, 240 x 8 waves per workgroup)
        p.fill = (int64_t)c->num_cus;
        (void)dispatch_int<12, 14>(c->logN, [&](auto lb) {
            constexpr int LOGB = decltype(lb)::value, LOGT = logt_for(LOGB);
            p.fill *= persistent_per_cu((size_t)lds_words<LOGB, LOGT>() * 8, LOGT);
            return TFHE_OK;
        });
        // the partial sums of any pass: splits <= fill / rows, so (splits - 1) x items stays below fill / limbs (a last, smaller range
        // of items has more splits of fewer items); nothing to split below five terms
        p.ws_bytes = std::min(p.terms, n_terms) > 4 ? (size_t)(p.fill / limbs + 1) * p.row * 8 : 0;
        return p;
    }
    p.scratch_rows = c->logN > 14 ? 1 : 0;
    // (the cap: 1 GiB each for the scratch, the coefficients and the images at N > 2^14)
    const size_t slot = n_coef ? (p.scratch_rows + 2) * p.row * 8 : 0, cap = (size_t)3072 << 20;
    const int64_t items0 = chunk_of(c, count, 4096);
    p.terms = (int)chunk_of(c, n_terms, TFHE_DOT_MAX, cap, slot * (size_t)items0);
    p.items = chunk_of(c, count, 4096, cap, slot * (size_t)p.terms);
    p.ws_bytes = slot * (size_t)std::min(p.terms, n_coef) * (size_t)p.items;
    return p;
}

template <class A>
int dot_launch_fused(tfhe_ctx* c, const limb_sel_t& sel, u32 mask, const dot_view_arg_t& D, const u64* acc, size_t acc_stride, u64* dst,
                     size_t dst_stride, u64* part, int64_t ni, int nsplit, int tps) {
    const limb_sel_t pos = limb_subset(sel.n, mask);
    if (pos.n == 0) return TFHE_OK;
    const unsigned items = (unsigned)(ni * nsplit * pos.n);
    int transforms = 0;
    for (int k = 0; k < D.n; k++) transforms += !((D.a_ntt >> k) & 1u);
    auto kern = [&](auto lb) {
        constexpr int LOGB = decltype(lb)::value;
        return k_dot_plain_fused<A, LOGB, logt_for(LOGB)>;
    };
    return launch_fused_rows(c, items, (int64_t)ni * pos.n * transforms, kern, D, acc, (u64)acc_stride, dst, (u64)dst_stride, part, (u32)ni, (u32)tps,
                             c->limbs_dev, sel, pos, items);
}

// the bytes item views [base + i * stride, + row) for i < count span (count >= 1)
size_t view_bytes(size_t stride, int64_t count, size_t row) { return ((size_t)(count - 1) * stride + row) * 8; }

}  // namespace

extern "C" int tfhe_dot_plain(tfhe_ctx* c, const uint64_t* acc, size_t acc_stride, const uint64_t* const* a, const size_t* a_stride,
                              const uint8_t* a_ntt, const uint64_t* const* b, const size_t* b_stride, int n_terms, uint64_t* dst,
                              size_t dst_stride, int64_t count, int limbs, const int32_t* limb_idx) {
    // every check runs on the host before any device use
    if (!a || !a_stride || !a_ntt || !b || !b_stride || !dst) return fail(TFHE_E_BADARG, "null argument");
    if (n_terms < 1) return fail(TFHE_E_BADARG, "tfhe_dot_plain needs at least one term");
    if (count < 0) return fail(TFHE_E_BADARG, "negative count");
    int n_coef = 0;
    for (int k = 0; k < n_terms; k++) {
        if (!a[k] || !b[k]) return fail(TFHE_E_BADARG, "null operand %d", k);
        if (a_ntt[k] > 1) return fail(TFHE_E_BADARG, "a_ntt[%d] is 0 or 1", k);
        if ((const void*)dst == (const void*)a[k] || (const void*)dst == (const void*)b[k]) return fail(TFHE_E_BADARG, "dst overlaps operand %d", k);
        n_coef += a_ntt[k] == 0;
    }
    if (!c) return fail(TFHE_E_BADARG, "null context");
    limb_sel_t sel;
    int rc = make_sel(c, limbs, limb_idx, &sel);
    if (rc) return rc;
    // count x limbs fits the row kernels' item counter, and no view spans more than 2^40 words: nothing below can wrap
    const size_t row = (size_t)limbs * (size_t)c->N, max_stride = ((size_t)1 << 40) / (size_t)std::max<int64_t>(count, 1);
    if (count > 0x7fffffffll / limbs) return fail(TFHE_E_BADARG, "bad polynomial count");
    if (dst_stride < row || dst_stride > max_stride || (acc && (acc_stride < row || acc_stride > max_stride)))
        return fail(TFHE_E_BADARG, "stride of dst / acc below limbs * N = %zu words (or count x stride above 2^40)", row);
    for (int k = 0; k < n_terms; k++)
        if (a_stride[k] < row || a_stride[k] > max_stride || (b_stride[k] != 0 && b_stride[k] < row) || b_stride[k] > max_stride)
            return fail(TFHE_E_BADARG, "stride of operand %d below limbs * N = %zu words (or count x stride above 2^40)", k, row);
    if (count > 0) {
        const size_t dst_bytes = view_bytes(dst_stride, count, row);
        for (int k = 0; k < n_terms; k++)
            if (ranges_overlap(dst, dst_bytes, a[k], view_bytes(a_stride[k], count, row)) ||
                ranges_overlap(dst, dst_bytes, b[k], view_bytes(b_stride[k], count, row)))
                return fail(TFHE_E_BADARG, "dst overlaps operand %d", k);
        if (acc && !((const void*)acc == (const void*)dst && acc_stride == dst_stride) &&
            ranges_overlap(dst, dst_bytes, acc, view_bytes(acc_stride, count, row)))
            return fail(TFHE_E_BADARG, "dst overlaps acc (other than as the same view)");
    }
    if (count == 0) return TFHE_OK;

    const dot_plan plan = dot_plan_for(c, n_terms, n_coef, count, limbs);
    if (!plan.fused && c->logN > 17) return fail(TFHE_E_UNSUPPORTED, "N = 2^%d not supported (max 2^17)", c->logN);
    void* ws = nullptr;
    if (plan.ws_bytes) {
        rc = ensure_ws(c, plan.ws_bytes, &ws);   // once, before any lane fork of the transforms
        if (rc) return rc;
    }
    const policy_split_t ps = policy_split(c, sel);
    for (int64_t i0 = 0; i0 < count; i0 += plan.items) {
        const int64_t ni = std::min(plan.items, count - i0);
        u64* const d = dst + (size_t)i0 * dst_stride;
        const u64* running = acc ? acc + (size_t)i0 * acc_stride : nullptr;
        size_t running_stride = acc_stride;
        for (int k0 = 0; k0 < n_terms; k0 += plan.terms) {   // further passes accumulate onto dst
            dot_view_arg_t D{};
            D.n = std::min(plan.terms, n_terms - k0);
            int coef = 0;
            for (int k = 0; k < D.n; k++) {
                D.a[k] = a[k0 + k] + (size_t)i0 * a_stride[k0 + k];
                D.a_stride[k] = a_stride[k0 + k];
                D.b[k] = b[k0 + k] + (size_t)i0 * b_stride[k0 + k];
                D.b_stride[k] = b_stride[k0 + k];
                if (a_ntt[k0 + k]) D.a_ntt |= 1ull << k;
                else coef++;
            }
            if (plan.fused) {
                int tps;
                const int nsplit = dot_split(plan.fill, ni * limbs, D.n, &tps);
                if ((size_t)(nsplit - 1) * (size_t)ni * plan.row * 8 > plan.ws_bytes) return fail(TFHE_E_HIP, "internal: the plan's workspace is too small");
                rc = both_policies(c, ps.all & ~ps.fpmask, ps.fpmask, [&](auto pol, u32 mask) {
                    return dot_launch_fused<decltype(pol)>(c, sel, mask, D, running, running_stride, d, dst_stride, (u64*)ws, ni, nsplit, tps);
                });
                if (rc) return rc;
                if (nsplit > 1) {   // (both lanes have joined)
                    rc = launch(c, k_dot_join, row_grid((unsigned)(ni * limbs), (size_t)c->N), dim3(256), 0, d, (u64)dst_stride, (const u64*)ws, (u32)ni,
                                (u32)nsplit, c->limbs_dev, sel, (u32)c->N);
                    if (rc) return rc;
                }
            } else {
                if (coef) {
                    // slot s of the pass: the s-th coefficient-domain term, [ni][limbs][N] dense
                    const size_t slot = (size_t)ni * plan.row;
                    u64* const S = (u64*)ws + (size_t)coef * slot * plan.scratch_rows;
                    u64* const G = S + (size_t)coef * slot;
                    for (int k = 0, s = 0; k < D.n; k++) {
                        if ((D.a_ntt >> k) & 1u) continue;
                        HIP_TRY(hipMemcpy2DAsync(S + (size_t)s * slot, plan.row * 8, D.a[k], (size_t)D.a_stride[k] * 8, plan.row * 8, (size_t)ni,
                                                 hipMemcpyDeviceToDevice, c->stream));
                        D.a[k] = G + (size_t)s * slot;
                        D.a_stride[k] = plan.row;
                        s++;
                    }
                    rc = run_ntt(c, false, S, G, (int64_t)coef * ni * limbs, sel);
                    if (rc) return rc;
                    if (c->ws != ws) return fail(TFHE_E_HIP, "internal: a transform moved the workspace");
                    D.a_ntt = ~0ull;
                }
                rc = launch(c, k_dot_view, row_grid((unsigned)(ni * limbs), (size_t)c->N), dim3(256), 0, D, running, (u64)running_stride, d,
                            (u64)dst_stride, c->limbs_dev, sel, (u32)c->N);
                if (rc) return rc;
            }
            running = d;
            running_stride = dst_stride;
        }
    }
    return TFHE_OK;
}
