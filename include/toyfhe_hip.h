/*
 * toyfhe_hip.h -- C ABI of libtoyfhe_hip.so, the MI355X (gfx950) engine for the power-of-two
 * cyclotomic RNS polynomial path of JuliaCrypto/ToyFHE.jl.
 *
 * The reference has no FFI: its extension seam is Julia dispatch on the storage type of
 * RingElement{ℛ,Field,Storage} (src/pow2_cyc_rings.jl:93-96), exactly how src/crt.jl:247-275 plugs
 * the RNS NTT in.  Each entry point below names the reference method(s) a Julia shim binds it to
 * (see INTEGRATION.md for the ccall side).  All citations are relative to /root/reference/src/.
 *
 * Conventions
 *   - every function returns 0 (TFHE_OK) or a negative tfhe_status; tfhe_last_error() gives text.
 *     Nothing aborts or throws across the ABI.
 *   - residues are uint64_t in [0, q_l); q_l < 2^62, odd primes with 2N | q_l - 1.
 *   - polynomial data is device memory, layout [count][limbs][N] (limb-major SoA = the StructArray
 *     field arrays of src/crt.jl:150-156); a ciphertext batch is [batch][polys][limbs][N].
 *   - limb j of a buffer uses context modulus limb_idx[j] (crtselect, src/crt.jl:185-211);
 *     limb_idx == NULL means 0..limbs-1.  limb_idx is a HOST array.
 *   - domain (coefficient "primal" / NTT "dual", src/pow2_cyc_rings.jl:93-145) is tracked by the
 *     caller; NTT-domain data is in natural order: â[k] = a(ψ^(2k+1)) (src/pow2_cyc_rings.jl:278-294).
 *   - all work is enqueued on the context's stream (tfhe_ctx_set_stream); calls are asynchronous
 *     unless stated.  No host pointer is retained after a call returns.
 *   - threading: a tfhe_ctx (and a tfhe_bfv_plan) carries per-call scratch (transform workspaces, the prepared key rows
 *     of the fused key switch) that is recycled in stream order, so ONE host thread drives a given context at a time;
 *     different contexts / plans are independent and may be driven from different threads (no global mutable state
 *     besides the thread-local error text).  Share read-only inputs (evaluation keys, ciphertexts) freely.
 *     A tfhe_plain_plan runs on its context's stream and uses that context's workspace: it is driven by the thread that
 *     drives its context.
 *     tfhe_free, tfhe_ctx_destroy, tfhe_bfv_plan_destroy, tfhe_plain_plan_destroy and tfhe_comm_destroy may be called from ANY thread (a garbage
 *     collector's finalizer thread): tfhe_free takes the allocator's lock and parks the block behind events recorded on every
 *     live context's stream -- it never waits and never touches a context's scratch; the destroy calls synchronise the
 *     object's own stream first and must only not race with a call that is still USING that object.
 *     tfhe_ctx_destroy DRAINS the context's streams (main and side lane) BEFORE the allocator forgets them: a tfhe_free that arrives
 *     from another thread while the destroy runs still parks its block behind the context's queued work.  tfhe_bfv_plan_destroy
 *     drains the main stream and the side lane of both of its contexts, and tfhe_plain_plan_destroy its context's stream: a plan is
 *     destroyed BEFORE the contexts it was made on.  (The Python binding sees to it when finalizers run in another order: a Context
 *     closed while plans on it are open is destroyed by the last plan's close -- tests/test_native_lifetime_cpu.py.)
 *     Held by: contexts / plans on different threads, first use at once, the thread-local error text --
 *     tests/test_gpu_threads.py test_four_rings_on_four_threads_first_use_at_once_and_error_text_per_thread; tfhe_free from any
 *     thread -- test_frees_from_a_finaliser_thread_while_the_producer_keeps_enqueuing; a freed block is not handed out while
 *     queued work of another stream can touch it -- test_hand_out_waits_for_work_queued_on_another_stream and (the next user a borrowed workspace)
 *     test_workspace_borrower_takes_the_parked_block_behind_a_stream_wait; destroy drains first --
 *     test_destroy_drains_before_the_allocator_forgets_the_stream; the allocator's lock, events and stream waits on threads, on
 *     the CPU under sanitizers -- tests/test_alloc_model_cpu.py.
 *   - a BFV plan over two contexts runs the extension-basis work on ℛbig's stream and the key switch on ℛ's stream and
 *     orders the two with events; it never re-points a context's stream.  Results are ordered on ℛ's stream
 *     (tfhe_ctx_sync(small) waits for them).
 */
#ifndef TOYFHE_HIP_H
#define TOYFHE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    TFHE_OK = 0,
    TFHE_E_BADARG = -1,          /* @assert-class failures (pow2_cyc_rings.jl:31,61,116; rlwe_she.jl:318) */
    TFHE_E_DOMAIN = -2,
    TFHE_E_LEVEL_MISMATCH = -3,
    TFHE_E_PARAMS_MISMATCH = -4, /* UsageError (rlwe_she.jl:223-225,233-235,248-250) */
    TFHE_E_NOMEM = -5,
    TFHE_E_HIP = -6,
    TFHE_E_UNSUPPORTED = -7      /* error("... only implemented for ...") (crt.jl:270,274) */
} tfhe_status;

typedef struct tfhe_ctx tfhe_ctx;       /* a ring: NegacyclicRing{CRTEncoded{L,...},N} */
typedef struct tfhe_bfv_plan tfhe_bfv_plan; /* (ℛ, ℛbig, t) of a BFVParams */
typedef struct tfhe_comm tfhe_comm;     /* the ranks of a multi-GPU job (one process per GPU) */
typedef struct tfhe_plain_plan tfhe_plain_plan; /* (ring limbs, t) of a BFVParams / BGVParams: the plaintext codec */

const char *tfhe_last_error(void);      /* thread-local text of the last failure */
int tfhe_device_count(int *n);
int tfhe_set_device(int dev);

/* ---- ring context ---------------------------------------------------------------------------
 * NegacyclicRing{BaseRing,N}(ψ) (pow2_cyc_rings.jl:27-65) / NegacyclicRing(N, logqs) (crt.jl:282-295).
 * psi[l] == 0 (or psi == NULL) derives GaloisFields.minimal_primitive_root(𝔽q, 2N) (pow2_cyc_rings.jl:40,
 * crt.jl:142-144); a non-zero psi[l] must satisfy psi^(2N) == 1 (pow2_cyc_rings.jl:31) else TFHE_E_BADARG. */
int tfhe_ctx_create(int64_t N, int L, const uint64_t *q, const uint64_t *psi, tfhe_ctx **out);
int tfhe_ctx_destroy(tfhe_ctx *ctx);
int tfhe_ctx_psi(const tfhe_ctx *ctx, uint64_t *psi_out /* [L] */);
int tfhe_ctx_set_stream(tfhe_ctx *ctx, void *hip_stream /* hipStream_t, NULL = library-owned */);
int tfhe_ctx_sync(tfhe_ctx *ctx);
/* Device-side ordering between two contexts (each has its own stream): work submitted to `ctx` after this call starts after
 * everything submitted to `producer` before it.  No host wait.  (The reference is single-threaded and synchronous, so it has
 * no counterpart; the host mirrors use it where a ciphertext of one ring context meets a key of another, rlwe_she.jl:315.) */
int tfhe_ctx_wait_for(tfhe_ctx *ctx, tfhe_ctx *producer);
/* choose the NTT kernel family: 0 = auto (register-blocked LDS kernel; exact-integer fp64 butterflies
 * when every selected modulus is < 2^50 + 2^40, u64 Shoup butterflies otherwise), 1 = force the generic
 * radix-2 kernel, 2 = force the u64 register-blocked kernel, 3 = fp64 kernels one operation per launch: no fused
 * BFV core / key-switch kernels, no next-row overlap (LDS-DMA staging in the inverse, register prefetch in the
 * forward), no read-once digit lift -- 1, 2 and 3 are cross-check paths for tests */
int tfhe_ctx_set_ntt_variant(tfhe_ctx *ctx, int variant);
/* upper bound on the ciphertexts (polynomials, for the samplers and codecs) per internal chunk of every chunked entry point
 * driven through this context; 0 = default.  Same words for every value -- a cross-check knob for tests. */
int tfhe_ctx_set_chunk(tfhe_ctx *ctx, int chunk);
/* the context's current long-lived workspace (device pointer and size; NULL / 0 before the first call that needs one).  Reports
 * state and never allocates -- a diagnostic for tests, which fill the block between calls (tfhe_memset) to show that no entry
 * point's words depend on what its scratch held.  The block moves when a later call needs a larger one. */
int tfhe_ctx_workspace(const tfhe_ctx *ctx, void **ptr, size_t *bytes);

/* ---- device memory helpers (for callers without a GPU array package) -------------------------
 * tfhe_malloc / tfhe_free are a size-bucketed recycling allocator (csrc/dev_alloc.h): the reference allocates a fresh array
 * per ring operation (e.g. broadcast results, pow2_cyc_rings.jl:167,200-214), so the mirror frees and allocates thousands of
 * equally sized buffers per circuit.  tfhe_free never synchronises: the block is parked behind events recorded on every
 * live context's stream and is handed out again only once they have completed.  TFHE_ALLOC_CACHE=0 selects plain
 * hipMalloc / hipFree.  tfhe_alloc_trim returns the cached blocks to the driver (drains the device). */
int tfhe_malloc(size_t bytes, void **dptr);
int tfhe_free(void *dptr);
int tfhe_alloc_stats(uint64_t *live_bytes, uint64_t *cached_bytes, uint64_t *hip_mallocs, uint64_t *reuses);
int tfhe_alloc_trim(void);
int tfhe_memcpy_h2d(void *dst, const void *src, size_t bytes);  /* synchronous */
int tfhe_memcpy_d2h(void *dst, const void *src, size_t bytes);  /* synchronous */
int tfhe_memcpy_d2d(tfhe_ctx *ctx, void *dst, const void *src, size_t bytes); /* on the ctx stream */
int tfhe_memset(tfhe_ctx *ctx, void *dst, int byte, size_t bytes);
/* ciphertext staging: the reference keeps a ciphertext as a tuple of ring elements (CipherText.cs, rlwe_she.jl:131-136),
 * the fused entry points take [batch][polys][limbs][N].  Component p of a packed batch [count][polys][words]
 * <- / -> a batch of single polynomials [count][words] (words = limbs * N), one strided copy on the ctx stream. */
int tfhe_pack_poly(tfhe_ctx *ctx, uint64_t *packed, const uint64_t *src, int polys, int p, size_t words, int64_t count);
int tfhe_unpack_poly(tfhe_ctx *ctx, uint64_t *dst, const uint64_t *packed, int polys, int p, size_t words, int64_t count);
/* dst [count][words] <- src [words] repeated: one ring element (a plaintext operand, a key) against a batch of ciphertexts
 * (the `Ref(c)` / scalar-broadcast patterns of rlwe_she.jl:143 and ckksencoding.jl:99-124). */
int tfhe_broadcast_poly(tfhe_ctx *ctx, uint64_t *dst, const uint64_t *src, size_t words, int64_t count);

/* ---- K1/K2: nntt / inntt --------------------------------------------------------------------
 * NTT.nntt / NTT.inntt on RingCoeffs (pow2_cyc_rings.jl:295-318), per limb as crt.jl:247-267.
 * count = number of polynomials ([count][limbs][N]); src == dst allowed. */
int tfhe_nntt(tfhe_ctx *ctx, const uint64_t *src, uint64_t *dst, int64_t count, int limbs, const int32_t *limb_idx);
int tfhe_inntt(tfhe_ctx *ctx, const uint64_t *src, uint64_t *dst, int64_t count, int limbs, const int32_t *limb_idx);

/* ---- K3/K4: limb-wise arithmetic (crt.jl:120-134; pow2_cyc_rings.jl:167,177-219) -------------- */
int tfhe_add(tfhe_ctx *ctx, const uint64_t *a, const uint64_t *b, uint64_t *dst, int64_t count, int limbs, const int32_t *limb_idx);
int tfhe_sub(tfhe_ctx *ctx, const uint64_t *a, const uint64_t *b, uint64_t *dst, int64_t count, int limbs, const int32_t *limb_idx);
int tfhe_neg(tfhe_ctx *ctx, const uint64_t *a, uint64_t *dst, int64_t count, int limbs, const int32_t *limb_idx);
int tfhe_mul(tfhe_ctx *ctx, const uint64_t *a, const uint64_t *b, uint64_t *dst, int64_t count, int limbs, const int32_t *limb_idx);
/* dst = acc + a*b (the `c += x*y` pattern of rlwe_she.jl:257,342-343) */
int tfhe_mad(tfhe_ctx *ctx, const uint64_t *acc, const uint64_t *a, const uint64_t *b, uint64_t *dst, int64_t count, int limbs, const int32_t *limb_idx);
/* dst = (acc +) sum_{k < n_terms} a[k] .* b[k], every operand [count][limbs][N] (acc may be NULL; dst may alias acc): the
 * accumulation loop `result += rotated_k * diagonal_k` of the diagonal matrix-vector product (examples/encrypted_mnist/
 * infer.jl:140-149 -- there one ring multiplication and one ring addition per term, pow2_cyc_rings.jl:167,200-214) in one pass.
 * a, b: host arrays of n_terms device pointers.  Exact: the same canonical residues as tfhe_mad term by term. */
int tfhe_dot(tfhe_ctx *ctx, const uint64_t *acc, const uint64_t *const *a, const uint64_t *const *b, int n_terms, uint64_t *dst,
             int64_t count, int limbs, const int32_t *limb_idx);
/* dst = sum_{k < n_terms} scalars[k] * a[k], every a[k] and dst [count][limbs][N], either domain: the scalar-weighted sum of ring
 * elements (per term one scalar_mul, pow2_cyc_rings.jl:177-185, and one +, :200-214) -- e.g. a convolution with plaintext
 * scalar weights over encrypted inputs, examples/encrypted_mnist/infer.jl:127-129 (49 terms per channel and component) -- in
 * one pass.  scalars: HOST array [n_terms][limbs] of residues (scalars[k][j] < modulus of limb j); a: host array of n_terms
 * device pointers; n_terms <= 64.  Exact: the canonical residues of the term-by-term sum. */
int tfhe_lincomb(tfhe_ctx *ctx, const uint64_t *scalars, const uint64_t *const *a, int n_terms, uint64_t *dst, int64_t count, int limbs,
                 const int32_t *limb_idx);
/* n_out such sums of the SAME operands in one pass over them -- the output channels of a convolution layer, infer.jl:127-131 (each of
 * the 4 channels weighs the same 49 encrypted inputs): dst[o] = sum_k scalars[o][k] * a[k].  scalars: HOST array
 * [n_out][n_terms][limbs] of residues; dst: host array of n_out device pointers ([count][limbs][N] each, distinct from the
 * operands); n_terms <= 64.  Same words as n_out calls of tfhe_lincomb. */
int tfhe_lincomb_many(tfhe_ctx *ctx, const uint64_t *scalars, const uint64_t *const *a, int n_terms, uint64_t *const *dst, int n_out,
                      int64_t count, int limbs, const int32_t *limb_idx);
/* scalar_mul (pow2_cyc_rings.jl:177-185): scalar given as residues scal[j] mod q_{limb_idx[j]} (host array) */
int tfhe_scalar_mul(tfhe_ctx *ctx, const uint64_t *scal, const uint64_t *a, uint64_t *dst, int64_t count, int limbs, const int32_t *limb_idx);

/* ---- K5: tensor of two 2-element ciphertexts in the NTT domain (rlwe_she.jl:255-258) ----------
 * a, b: [batch][2][limbs][N]; out: [batch][3][limbs][N] = (a0 b0, a0 b1 + a1 b0, a1 b1). */
int tfhe_tensor(tfhe_ctx *ctx, const uint64_t *a, const uint64_t *b, uint64_t *out, int64_t batch, int limbs, const int32_t *limb_idx);

/* ---- K6/K7: level operations ------------------------------------------------------------------
 * modswitch(::RingElement) (crt.jl:226-228 with :215-220): coefficient domain,
 * src [count][limbs][N] -> dst [count][limbs-1][N]; c_last taken as its unsigned representative. */
int tfhe_rescale(tfhe_ctx *ctx, const uint64_t *src, uint64_t *dst, int64_t count, int limbs, const int32_t *limb_idx);
/* crtselect / drop_last / modswitch_drop (crt.jl:185-213,222-236): gather limbs `which` (positions in
 * the source buffer) of each polynomial: src [count][src_limbs][N] -> dst [count][n_which][N]. */
int tfhe_select_limbs(tfhe_ctx *ctx, const uint64_t *src, uint64_t *dst, int64_t count, int src_limbs, const int32_t *which, int n_which);

/* ---- K8: apply_galois_element (pow2_cyc_rings.jl:321-329), coefficient domain; src != dst. */
int tfhe_galois(tfhe_ctx *ctx, const uint64_t *src, uint64_t *dst, uint64_t galois_element, int64_t count, int limbs, const int32_t *limb_idx);

/* ---- K9-K11 (+K6): keyswitch (rlwe_she.jl:315-347) with RNS digits (relin_window == 0, :326-329) --
 * The KEY ring is the first key_limbs (= Lk) moduli of ctx (ctx may hold further moduli, e.g. a BFV
 * extension basis).  The ciphertext lives on key limbs 0..level-1.
 *   special != 0: ModulusRaised (modulusraising.jl:35-49): key modulus Lk-1 is the special prime;
 *                 expand = *P and append a zero limb, contract = modswitch by P; level <= Lk-1.
 *   evk: [n_digits][2][Lk][N], component 0 = mask, 1 = masked (rlwe_she.jl:297), NTT domain, full key
 *        basis; digits 0..level-1 are consumed (rlwe_she.jl:340), n_digits >= level.
 *   ct:  [batch][polys][level][N], polys in {2,3} (rlwe_she.jl:318), coefficient domain.
 *   out: [batch][2][level][N], coefficient domain. */
int tfhe_keyswitch(tfhe_ctx *ctx, int key_limbs, int level, int special, const uint64_t *evk, int n_digits, const uint64_t *ct, int polys, uint64_t *out, int64_t batch);
/* rotate(gk, c) = keyswitch(gk, apply_galois_element(c, g)) (rlwe_she.jl:355-359) */
int tfhe_rotate(tfhe_ctx *ctx, int key_limbs, int level, int special, const uint64_t *evk, int n_digits, uint64_t galois_element, const uint64_t *ct, uint64_t *out, int64_t batch);
/* the same with the key already prepared by tfhe_galois_key_prepare for this galois_element (below): a caller that rotates by one
 * Galois element again and again (infer.jl:140-149: 63 chained rotate(gk, rotated) per matrix product, ONE key) prepares the key
 * once instead of once per call.  Bit-identical to tfhe_rotate on the plain key. */
int tfhe_rotate_prepared(tfhe_ctx *ctx, int key_limbs, int level, int special, const uint64_t *evk_prepared, int n_digits, uint64_t galois_element,
                         const uint64_t *ct, uint64_t *out, int64_t batch);

/* Hoisted rotations: out[r] = rotate(gk_r, c) for r < n_rot from one digit decomposition of c (the RNS digits commute with
 * the automorphism; in the NTT domain it is an index permutation), bit-identical to n_rot calls of tfhe_rotate at
 * level * (level [+1]) forward transforms in total instead of per rotation -- the shape of a diagonal-method matrix product
 * (ckks_matmul.jl:33-41, infer.jl:140-149) when every rotation starts from the same ciphertext.
 *   evks: HOST array of n_rot device pointers (one Galois key each, layout as tfhe_keyswitch; prepared != 0: the outputs of
 *   tfhe_galois_key_prepare); galois: HOST array [n_rot];
 *   ct: [batch][2][level][N]; out: [n_rot][batch][2][level][N]. */
int tfhe_rotate_many(tfhe_ctx *ctx, int key_limbs, int level, int special, const uint64_t *const *evks, int n_digits, int prepared,
                     const uint64_t *galois_elements, int n_rot, const uint64_t *ct, uint64_t *out, int64_t batch);
/* Diagonal matrix-vector product in one call (examples/encrypted_mnist/infer.jl:140-149, test/ckks_matmul.jl:33-41):
 *     out = diag[0] .* c + sum_{r < n_rot} diag[r+1] .* rotate(gk_r, c)
 * with the rotations hoisted as in tfhe_rotate_many and every step run over all rotations at once; bit-identical to
 * tfhe_rotate_many -> tfhe_nntt -> tfhe_dot.  evks: HOST array of n_rot device pointers to PREPARED Galois keys
 * (tfhe_galois_key_prepare); galois_elements: HOST array [n_rot]; n_rot <= 64;
 *   diags: device [n_rot + 1][level][N], the plaintext diagonals in the NTT domain at the ciphertext's level, shared by the batch;
 *   ct: [batch][2][level][N] coefficient domain; out: [batch][2][level][N] NTT domain (the product's scale is the caller's business). */
int tfhe_matmul_diag(tfhe_ctx *ctx, int key_limbs, int level, int special, const uint64_t *const *evks, int n_digits,
                     const uint64_t *galois_elements, int n_rot, const uint64_t *diags, const uint64_t *ct, uint64_t *out, int64_t batch);
/* The same product by baby and giant steps, in one call.  With the rotation index written k = j n1 + i,
 *     sum_k d_k .* rho^k(x) = sum_j rho^(j n1)( sum_i rho^(-j n1)(d_k) .* rho^i(x) ):
 * n_baby + n_giant Galois keys and key sums instead of one per diagonal (a 64 x 64 layer with n1 = 8: 7 + 7 instead of 63).
 *     inner_j = sum_{i = 0 .. n_baby} diags[j][i] .* NTT(r_i(ct))      (r_0 = identity, r_i = rotate(baby key i - 1, .)),  j = 0 .. n_giant
 *     out     = INTT(inner_0) + sum_{j = 1 .. n_giant} rotate(giant key j - 1, INTT(inner_j))
 *   baby_evks / giant_evks: HOST arrays of n_baby / n_giant device pointers to PREPARED Galois keys (tfhe_galois_key_prepare), as for
 *   tfhe_matmul_diag; baby_galois / giant_galois: HOST arrays of their Galois elements; n_baby, n_giant in [0, 64];
 *   diags: device [n_giant + 1][n_baby + 1][level][N], NTT domain, shared by the batch -- pre-rotating them (rho^(-j n1)) is the
 *   caller's business;  ct, out: [batch][2][level][N], coefficient domain, as for tfhe_rotate.
 * The result equals, word for word, tfhe_rotate_many over the baby keys -> tfhe_nntt -> tfhe_dot per giant step -> tfhe_inntt ->
 * tfhe_rotate_prepared per giant step j >= 1 -> tfhe_add: every step is exact arithmetic on canonical residues, so every path
 * (evaluation-domain or coefficient tail, every route of the nested key switch) and every tfhe_ctx_set_chunk gives the same bits.
 * Checked on the host before any device use, in this order: null arrays or a null key among the first n_baby / n_giant, n_baby /
 * n_giant outside [0, 64], an even Galois element, out starting where ct or diags start (all TFHE_E_BADARG); then the context;
 * then the level / key-limb rules of tfhe_keyswitch, Galois elements not below 2N and out overlapping ct or diags anywhere
 * (TFHE_E_BADARG).  batch == 0 does nothing, but still needs a context. */
int tfhe_matmul_bsgs(tfhe_ctx *ctx, int key_limbs, int level, int special,
                     const uint64_t *const *baby_evks, const uint64_t *baby_galois, int n_baby,
                     const uint64_t *const *giant_evks, const uint64_t *giant_galois, int n_giant,
                     int n_digits, const uint64_t *diags, const uint64_t *ct, uint64_t *out, int64_t batch);
/* The block-row product by baby and giant steps, in one call: n_in ciphertext inputs, each with its own diagonals, over ONE key set
 * (examples/encrypted_mnist/infer.jl:158-163: a 64 x 256 matrix applied to four ciphertexts, .+ b).  The rotation is linear, so the
 * inner sums of all inputs are added before they are rotated: n_giant giant key switches instead of n_in n_giant.
 *     inner_j = sum_{m < n_in} sum_{i = 0 .. n_baby} diags[m][j][i] .* NTT(r_i(cts[m]))      j = 0 .. n_giant
 *     out     = INTT(inner_0) + sum_{j = 1 .. n_giant} rotate(giant key j - 1, INTT(inner_j))   (+ bias on component 0)
 *   baby_evks / giant_evks, baby_galois / giant_galois, n_baby, n_giant in [0, 64], n_digits: as for tfhe_matmul_bsgs (PREPARED keys,
 *   HOST arrays);
 *   diags: HOST array of n_in device pointers, each [n_giant + 1][n_baby + 1][level][N], NTT domain, shared by the batch (the layout
 *   tfhe_matmul_bsgs takes, one per input);  cts: HOST array of n_in device pointers, each [batch][2][level][N], coefficient domain
 *   (the same pointer may appear more than once);  n_in in [1, 64];
 *   bias: NULL, or device [level][N], coefficient domain, canonical residues, shared by the batch: added limb-wise to component 0 of
 *   every output ciphertext;  out: [batch][2][level][N], coefficient domain.
 * The result equals, word for word, per input tfhe_rotate_many over the baby keys -> tfhe_nntt; per giant step ONE sum over all
 * n_in (n_baby + 1) terms, tfhe_dot (chained through its acc above 64 terms); -> tfhe_inntt -> tfhe_rotate_prepared per giant step
 * j >= 1 -> tfhe_add -> tfhe_add of the bias onto component 0: exact arithmetic on canonical residues, so every path
 * (evaluation-domain or coefficient tail, every route of the nested key switch) and every tfhe_ctx_set_chunk gives the same bits.
 * It is NOT the sum of n_in calls of tfhe_matmul_bsgs: the contraction by the special prime rounds, and here it rounds
 * once per giant step, not once per input and giant step.  With n_in = 1 and bias = NULL the words are those of tfhe_matmul_bsgs.
 * Checked on the host before any device use, in this order: null arrays, a null key among the first n_baby / n_giant, a null
 * diags[m] or cts[m] among the first n_in; n_baby / n_giant outside [0, 64], n_in outside [1, 64]; an even Galois element; out
 * starting where any cts[m], diags[m] or bias starts (all TFHE_E_BADARG); then the context; then the level / key-limb rules of
 * tfhe_keyswitch, Galois elements not below 2N and out overlapping any operand anywhere (TFHE_E_BADARG).  batch == 0 does nothing,
 * but still needs a context. */
int tfhe_matmul_bsgs_blocks(tfhe_ctx *ctx, int key_limbs, int level, int special,
                            const uint64_t *const *baby_evks, const uint64_t *baby_galois, int n_baby,
                            const uint64_t *const *giant_evks, const uint64_t *giant_galois, int n_giant, int n_digits,
                            const uint64_t *const *diags, const uint64_t *const *cts, int n_in,
                            const uint64_t *bias, uint64_t *out, int64_t batch);
/* Rotate and sum, in one call: the sum of a ciphertext with rotations of itself, step by step ("sum of slots"; the fold that closes
 * the product of a rectangular matrix, below).
 *     F_0 = ct;   F_{t+1} = F_t + sum_{u < group_sizes[t]} rotate(key_{t,u}, F_t);   out = F_{n_groups}
 *   evks / galois_elements: HOST arrays over all groups back to back (group 0's keys first): device pointers to PREPARED Galois keys
 *   (tfhe_galois_key_prepare) and their Galois elements;  group_sizes: HOST array [n_groups], every entry >= 1, their sum <= 64;
 *   n_groups in [0, 64] (0: out = ct);  ct, out: [batch][2][level][N], coefficient domain; out overlaps nothing.
 * The result equals, word for word, per group tfhe_rotate_many (prepared) over the group's keys on F_t -> tfhe_add of every result
 * onto F_t: exact arithmetic on canonical residues, so every path (with a special prime the rotations are summed in the evaluation
 * domain and inverse-transformed once per group; without one they are summed in the coefficient domain) and every
 * tfhe_ctx_set_chunk gives the same bits.
 * Checked on the host before any device use, in this order: null arrays (evks, galois_elements, group_sizes, ct, out); n_groups
 * outside [0, 64]; a group size below 1; more than 64 keys in all; a null key; an even Galois element; out starting where ct starts
 * (all TFHE_E_BADARG); then the context; then the level / key-limb rules of tfhe_keyswitch, Galois elements not below 2N and out
 * overlapping ct anywhere (TFHE_E_BADARG).  batch == 0 does nothing, but still needs a context. */
int tfhe_rotate_sum(tfhe_ctx *ctx, int key_limbs, int level, int special, const uint64_t *const *evks, const uint64_t *galois_elements,
                    const int *group_sizes, int n_groups, int n_digits, const uint64_t *ct, uint64_t *out, int64_t batch);
/* The product of a rectangular matrix, in one call: tfhe_matmul_bsgs_blocks without its bias -> the fold of tfhe_rotate_sum -> the
 * bias onto component 0.  For an m x n matrix with m | n (m a power of two) the diagonals are the m EXTENDED ones,
 * e_i[r] = W[r mod m][(r - i) mod n], and log2(n / m) fold steps add the n / m partial sums: m diagonals and log2(n / m) fold keys
 * instead of n diagonals of the matrix padded to n x n.  Afterwards every row r holds out[r mod m].
 *   baby_evks .. n_in: as for tfhe_matmul_bsgs_blocks;
 *   fold_evks / fold_galois / fold_group_sizes / n_fold_groups: as evks / galois_elements / group_sizes / n_groups of tfhe_rotate_sum;
 *   bias: NULL, or device [level][N], coefficient domain: added to component 0 AFTER the fold (before it, the fold would multiply it);
 *   out: [batch][2][level][N], coefficient domain.
 * The result equals, word for word, tfhe_matmul_bsgs_blocks (bias = NULL) -> tfhe_rotate_sum -> tfhe_add of the bias onto component 0,
 * on every path and for every tfhe_ctx_set_chunk; with n_fold_groups = 0 the words are those of tfhe_matmul_bsgs_blocks.
 * Checked on the host before any device use, in this order: null arrays (the fold's three among them), a null key among the first
 * n_baby / n_giant, a null diags[m] or cts[m] among the first n_in; n_baby / n_giant outside [0, 64], n_in outside [1, 64];
 * n_fold_groups outside [0, 64], a fold group size below 1, more than 64 fold keys in all, a null fold key; an even Galois element
 * (baby, giant, fold); out starting where any cts[m], diags[m] or bias starts (all TFHE_E_BADARG); then the context; then the
 * level / key-limb rules of tfhe_keyswitch, Galois elements not below 2N and out overlapping any operand anywhere (TFHE_E_BADARG).
 * batch == 0 does nothing, but still needs a context. */
int tfhe_matmul_bsgs_fold(tfhe_ctx *ctx, int key_limbs, int level, int special,
                          const uint64_t *const *baby_evks, const uint64_t *baby_galois, int n_baby,
                          const uint64_t *const *giant_evks, const uint64_t *giant_galois, int n_giant, int n_digits,
                          const uint64_t *const *diags, const uint64_t *const *cts, int n_in,
                          const uint64_t *const *fold_evks, const uint64_t *fold_galois, const int *fold_group_sizes, int n_fold_groups,
                          const uint64_t *bias, uint64_t *out, int64_t batch);
/* the one-time key preparation of the hoisted rotations: evk_out = the Galois key of x -> x^g (layout of tfhe_keyswitch,
 * n_digits components over key_limbs moduli) with every NTT-domain row permuted by g^-1, so that the key products run on the
 * transformed digits of the unrotated ciphertext.  prepared = 0 above takes plain keys and prepares them per call. */
int tfhe_galois_key_prepare(tfhe_ctx *ctx, int key_limbs, int n_digits, uint64_t galois_element, const uint64_t *evk, uint64_t *evk_out);

/* ---- K14: keyswitch with base-2^w digits (relin_window = w != 0, rlwe_she.jl:330-338; the default for
 * single-modulus rings, rlwe_she.jl:271) -------------------------------------------------------------
 * The ciphertext ring is limbs 0..level-1 of ctx, the key ring limbs 0..key_limbs-1 (as tfhe_keyswitch).  Digit i of a
 * coefficient is digit i of convert(Integer, x) in [0, Q_level) -- reconstructed exactly from the residues when
 * level > 1 -- embedded in every working limb; out_s = c_s + sum_i key_i,s * digit_i.
 *   special != 0: ModulusRaised (modulusraising.jl:35-49) -- limb key_limbs-1 is the special prime P, the working limbs
 *        are [0..level-1, key_limbs-1], c is raised to P c and the sums are contracted by floor(./P) (crt.jl:215-220).
 *   evk: [n_windows][2][key_limbs][N], component 0 = mask, 1 = masked, NTT domain; n_windows >= ndigits(Q_level, base = 2^w)
 *        = ceil(bitlength(Q_level) / w) (rlwe_she.jl:282,333; a key of a larger ring has more components, the first
 *        ndigits(Q_level) are used, rlwe_she.jl:340), else TFHE_E_PARAMS_MISMATCH.
 *   window_bits: 1..32 with 2^w below every modulus.   ct / out as tfhe_keyswitch. */
int tfhe_keyswitch_window(tfhe_ctx *ctx, int key_limbs, int level, int special, int window_bits, const uint64_t *evk, int n_windows,
                          const uint64_t *ct, int polys, uint64_t *out, int64_t batch);

/* ---- keyswitch with grouped RNS digits and several special primes (the "hybrid" gadget) ---------------------------------------
 * tfhe_keyswitch takes one digit per ciphertext limb and at most one special prime: level * (level + 1) forward transforms and
 * `level` key components of 2 (level + 1) rows.  Here a digit covers `group` limbs and the key ring ends in n_special = k special
 * primes whose product P should be at least every group modulus: with d = ceil(level / group) digits, d * (level + k) forward
 * transforms and d key components of 2 (level + k) rows.  Every step is exact arithmetic on canonical residues.
 *   Key ring: limbs 0..key_limbs-1 of ctx, the last k of them the special primes.  Ciphertext ring: limbs 0..level-1,
 *   level <= key_limbs - k.  Working limbs W = [0..level-1] + [key_limbs-k..key_limbs-1], nw = level + k.
 *   Digit g covers limbs G_g = [g group, min((g + 1) group, level)), g < d: the last group may be ragged, and at a level below
 *   the key's a group is cut at `level`.
 *   1. digit_g = the centred representative of c[end] modulo Q_g = prod_{i in G_g} q_i -- the exact CRT value with the tie rule of
 *      signedmod.jl:12-19 (n > Q_g ÷ 2 => n - Q_g) -- reduced into every limb of W: switch(ℛ_W, .) of bfv.jl:202-226 applied to
 *      the sub-ring of the group; with group = 1 the digit of rlwe_she.jl:326-329.
 *   2. S_s = P c_s (+ k zero limbs) + sum_g key_{g,s} * digit_g over W; s = 0 uses masked, s = 1 uses mask (rlwe_she.jl:340-344);
 *      c_2 starts from zero for a 2-element input (rlwe_she.jl:324).
 *   3. out_s = modswitch (crt.jl:215-228, unsigned c_last) applied k times to S_s, the last special prime first
 *      = c_s + the k-step contraction of INTT(sum_g ...), which is what is computed.
 *   evk: [n_digits][2][key_limbs][N], component 0 = mask, 1 = masked, NTT domain; n_digits >= d, the first d components are used.
 *        Gadget row g holds P mod q_j at the limbs j of group g at the key's own top level and zero elsewhere (the special primes'
 *        columns are zero): tfhe_evalkey_gen takes it as a table.
 *   ct: [batch][polys][level][N], polys in {2,3};  out: [batch][2][level][N];  both in the coefficient domain, as for tfhe_keyswitch.
 * (n_special, group) = (1, 1) gives the words of tfhe_keyswitch(special = 1), (0, 1) those of tfhe_keyswitch(special = 0).
 * tfhe_rotate_grouped is apply_galois_element (pow2_cyc_rings.jl:321-329) into the workspace followed by the key switch of the copy
 * (rlwe_she.jl:355-359), ct: [batch][2][level][N].
 * Checked on the host before any device use, in this order: a null argument; polys outside {2,3}; key_limbs outside [1, L];
 * n_special outside [0, min(4, key_limbs - 1)]; group < 1 (all TFHE_E_BADARG); level outside [1, key_limbs - n_special]
 * (TFHE_E_LEVEL_MISMATCH); n_digits < ceil(level / group) (TFHE_E_PARAMS_MISMATCH); level + n_special > 40 (TFHE_E_UNSUPPORTED);
 * a negative batch (TFHE_E_BADARG); a Galois element that is even or not below 2N (TFHE_E_BADARG).  `out` against `ct` and `evk`:
 * the rule of tfhe_keyswitch -- none is checked.  batch == 0 does nothing. */
int tfhe_keyswitch_grouped(tfhe_ctx *ctx, int key_limbs, int level, int n_special, int group, const uint64_t *evk, int n_digits,
                           const uint64_t *ct, int polys, uint64_t *out, int64_t batch);
int tfhe_rotate_grouped(tfhe_ctx *ctx, int key_limbs, int level, int n_special, int group, const uint64_t *evk, int n_digits,
                        uint64_t galois_element, const uint64_t *ct, uint64_t *out, int64_t batch);
/* Hoisted rotations and the diagonal product on grouped-digit keys.  The grouped digit is the centred representative modulo the odd
 * Q_g (no tie, centred(-x) = -centred(x)), so it commutes with the automorphism in every working limb and the identity of
 * tfhe_rotate_many carries over: the digits of c are decomposed and transformed ONCE -- d (level + k) forward transforms instead of
 * that per rotation -- and each rotation costs one key sum against its PREPARED key, one inverse transform and one tail, in which
 * the automorphism is applied to INTT(S') BEFORE the k-step contraction (the floor does not commute with sign changes).
 *   evks: HOST array of n_rot device pointers to prepared grouped Galois keys: tfhe_galois_key_prepare(key_limbs, the key's own
 *         component count, g_r) of the key tfhe_rotate_grouped takes.  There is no unprepared mode.  A key may appear more than once.
 *   galois_elements: HOST array [n_rot].
 * tfhe_rotate_many_grouped:  ct [batch][2][level][N], out [n_rot][batch][2][level][N], both in the coefficient domain; out[r] equals,
 *   word for word, tfhe_rotate_grouped(the unprepared key r, galois_elements[r], ct).  n_rot is not limited: the keys are taken in
 *   tiles of 64.
 * tfhe_matmul_diag_grouped:  out = diags[0] .* NTT(c) + sum_{r < n_rot} diags[r+1] .* NTT(rotate_grouped(gk_r, c));
 *   diags: device [n_rot + 1][level][N], NTT domain, shared by the batch; ct: [batch][2][level][N] coefficient domain; out:
 *   [batch][2][level][N] NTT domain; n_rot <= 64 -- the contract of tfhe_matmul_diag.  Word for word tfhe_rotate_many_grouped ->
 *   tfhe_nntt -> tfhe_dot.  With n_special >= 1 and n_rot >= 1 the rotations are finished in the evaluation domain: the k-step
 *   contraction of a limb is affine in its word, so only the n_special special limbs of every key sum are inverse-transformed (after
 *   the permutation pi_g) and their lift costs `level` forward transforms; TFHE_MD_COEFF=1 (read once per process) keeps the
 *   coefficient-domain tail, which also serves n_special == 0.  Both routes give the same words.
 * Checked on the host before any device use, in this order: a null ctx, evks, galois_elements, ct, out (diags for the product) or
 * n_rot < 0 (TFHE_E_BADARG); n_rot > 64, the product only (TFHE_E_UNSUPPORTED); for r = 0, 1, .. in turn the checks of
 * tfhe_rotate_grouped on (evks[r], galois_elements[r]) in that entry point's order, a null evks[r] being its null argument; `out`
 * overlapping `ct` (or `diags`) anywhere (TFHE_E_BADARG: the tail scatters into out while it reads ct).  tfhe_rotate_many_grouped with
 * n_rot == 0 returns TFHE_OK right after the null checks, as tfhe_rotate_many; tfhe_matmul_diag_grouped with n_rot == 0 runs the shape
 * checks of tfhe_keyswitch_grouped once and computes diags[0] .* NTT(c).  batch == 0 does nothing after the checks.  The result does
 * not depend on the chunk (tfhe_ctx_set_chunk) or the tile.
 * Workspace: tfhe_rotate_many_grouped takes its block -- digits and key sums of a chunk, up to 8 GiB, and as much again for the transforms
 * above N = 2^14 -- from the context's long-lived workspace, where it STAYS after the call (as tfhe_rotate_many's does) until a larger
 * request or tfhe_ctx_destroy; tfhe_ctx_set_chunk bounds it.  tfhe_matmul_diag_grouped borrows its block for the call, as tfhe_matmul_diag:
 * per ciphertext of a chunk d nw + R 2 nw + R 2 level + 2 level + R 2 n_special rows of N words (digits, key sums, lifts or rotated
 * ciphertexts, the ciphertext's transform, the permuted special limbs), and above N = 2^14 the largest transform's rows once more.
 * Still refused on grouped keys: the per-limb entry points tfhe_matmul_bsgs*, tfhe_matmul_bsgs_fold and tfhe_rotate_sum (on grouped keys
 * the product by baby and giant steps is tfhe_matmul_bsgs_grouped, the fold tfhe_rotate_sum_grouped and the rectangular product
 * tfhe_matmul_bsgs_fold_grouped, all below) and the
 * fused N <= 2^14 key switch; tfhe_mul_relin takes per-limb keys only -- the product on grouped keys is tfhe_mul_relin_grouped, below. */
int tfhe_rotate_many_grouped(tfhe_ctx *ctx, int key_limbs, int level, int n_special, int group, const uint64_t *const *evks, int n_digits,
                             const uint64_t *galois_elements, int n_rot, const uint64_t *ct, uint64_t *out, int64_t batch);
int tfhe_matmul_diag_grouped(tfhe_ctx *ctx, int key_limbs, int level, int n_special, int group, const uint64_t *const *evks, int n_digits,
                             const uint64_t *galois_elements, int n_rot, const uint64_t *diags, const uint64_t *ct, uint64_t *out, int64_t batch);
/* The block-row product by baby and giant steps on grouped-digit keys, in one call: the contract of tfhe_matmul_bsgs_blocks (n_in = 1,
 * bias = NULL: of tfhe_matmul_bsgs) with every rotation a tfhe_rotate_grouped.
 *     inner_j = sum_{m < n_in} sum_{i = 0 .. n_baby} diags[m][j][i] .* NTT(r_i(cts[m]))      j = 0 .. n_giant,  r_0 = identity
 *     out     = INTT(inner_0) + sum_{j = 1 .. n_giant} rotate_grouped(giant key j - 1, INTT(inner_j))   (+ bias on component 0)
 *   key_limbs, level, n_special, group, n_digits: as tfhe_rotate_many_grouped;  baby_evks / giant_evks: HOST arrays of device pointers
 *   to PREPARED grouped Galois keys (tfhe_galois_key_prepare), as for tfhe_rotate_many_grouped -- there is no unprepared mode, a key may
 *   appear more than once;  baby_galois / giant_galois: HOST arrays;  n_baby, n_giant in [0, 64];  diags, cts, n_in in [1, 64], bias,
 *   out: the layouts of tfhe_matmul_bsgs_blocks.
 * The result equals, word for word, per input tfhe_rotate_many_grouped over the baby keys -> tfhe_nntt; per giant step ONE tfhe_dot over
 * all n_in (n_baby + 1) terms; -> tfhe_inntt -> tfhe_rotate_grouped per giant step j >= 1 -> tfhe_add -> tfhe_add of the bias onto
 * component 0, on either route of the baby phase (evaluation-domain or TFHE_MD_COEFF=1, see tfhe_matmul_diag_grouped) and for every
 * tfhe_ctx_set_chunk.  (n_special, group) = (1, 1) and (0, 1) give the words of tfhe_matmul_bsgs_blocks with special = 1 and 0;
 * n_giant = 0 gives tfhe_inntt of tfhe_matmul_diag_grouped.  The giant steps are hoisted rotations with a tile of one key, finished in
 * the coefficient domain.
 * Checked on the host before any device use, in this order: a null ctx, baby_evks, baby_galois, giant_evks, giant_galois, diags, cts
 * or out; a null key among the first n_baby / n_giant, a null diags[m] or cts[m] among the first n_in; n_baby / n_giant outside
 * [0, 64], n_in outside [1, 64] (all TFHE_E_BADARG); for the baby keys, then the giant keys, in turn the shape checks of
 * tfhe_rotate_grouped on galois[r] in that entry point's order (without any key: those of tfhe_keyswitch_grouped, once); `out`
 * starting where, or overlapping anywhere, bias, any cts[m] or any diags[m] (TFHE_E_BADARG).  `out` is untouched on every refusal.
 * batch == 0 does nothing after the checks.  The call borrows its workspace block, as tfhe_matmul_bsgs_blocks: the rows of
 * tfhe_matmul_diag_grouped with R = n_baby (at least one key sum when there are giant steps) plus (2 n_giant + 1) 2 level rows per
 * ciphertext; the giant rotations run in the baby phase's digit and key-sum regions. */
int tfhe_matmul_bsgs_grouped(tfhe_ctx *ctx, int key_limbs, int level, int n_special, int group,
                             const uint64_t *const *baby_evks, const uint64_t *baby_galois, int n_baby,
                             const uint64_t *const *giant_evks, const uint64_t *giant_galois, int n_giant, int n_digits,
                             const uint64_t *const *diags, const uint64_t *const *cts, int n_in,
                             const uint64_t *bias, uint64_t *out, int64_t batch);
/* Rotate and sum, and the product of a rectangular matrix, on grouped-digit keys: the contracts of tfhe_rotate_sum and
 * tfhe_matmul_bsgs_fold with every rotation a tfhe_rotate_grouped.  (`group` is the number of limbs per digit, as everywhere on these
 * keys; the key lists of the fold are called fold steps here.)
 *     F_0 = ct;   F_{t+1} = F_t + sum_{u < group_sizes[t]} rotate_grouped(key_{t,u}, F_t);   out = F_{n_groups}
 *   key_limbs, level, n_special, group, n_digits: as tfhe_rotate_many_grouped;  evks / galois_elements (fold_evks / fold_galois): HOST
 *   arrays over all fold steps back to back: device pointers to PREPARED grouped Galois keys (tfhe_galois_key_prepare) and their Galois
 *   elements -- there is no unprepared mode, a key may appear more than once;  group_sizes (fold_group_sizes): HOST array [n_groups], the
 *   number of keys of every fold step, each >= 1, their sum <= 64;  n_groups in [0, 64];  the other operands of
 *   tfhe_matmul_bsgs_fold_grouped: as for tfhe_matmul_bsgs_grouped;  ct, out: [batch][2][level][N], coefficient domain.
 * tfhe_rotate_sum_grouped equals, word for word, per fold step tfhe_rotate_many_grouped over the step's keys on F_t -> tfhe_add of every
 * result onto F_t;  tfhe_matmul_bsgs_fold_grouped equals, word for word, tfhe_matmul_bsgs_grouped (bias = NULL) ->
 * tfhe_rotate_sum_grouped -> tfhe_add of the bias onto component 0.  (n_special, group) = (1, 1) and (0, 1) give the words of
 * tfhe_rotate_sum / tfhe_matmul_bsgs_fold with special = 1 and 0.  n_groups = 0 gives out = ct for the fold and the words of
 * tfhe_matmul_bsgs_grouped for the product.  The result depends neither on tfhe_ctx_set_chunk nor on the route of a fold step:
 *   evaluation route (n_special >= 1): X = NTT(F_t) and the key sums V_r as in tfhe_matmul_diag_grouped, E = X + sum_r V_r o pi_r, ONE
 *     inverse transform of E, and the lifts of the n_special special limbs of every key sum taken off in the coefficient domain --
 *     they never enter the evaluation domain: per ciphertext and step d nw + 2 level forward and R 2 n_special + 2 level inverse rows;
 *   coefficient route (n_special == 0, or TFHE_MD_COEFF=1): the hoisted rotations of tfhe_rotate_many_grouped into the workspace and
 *     one sum: d nw forward and R 2 nw inverse rows.
 *   The coefficient route is the default: measured, the evaluation route is ahead in steps of three keys and behind in steps of one
 *   (README, profiles/LOG.md), so it did not win everywhere.  TFHE_MDG_FOLD_EVAL=1 (read once per process) asks for the evaluation
 *   route; TFHE_MD_COEFF=1 wins over it.
 * Checked on the host before any device use, in this order: a null ctx or array (evks, galois_elements, group_sizes, ct, out; for the
 * product baby_evks, baby_galois, giant_evks, giant_galois, diags, cts, fold_evks, fold_galois, fold_group_sizes, out); the fold's host
 * rules, as tfhe_rotate_sum: n_groups outside [0, 64], a fold step size below 1, more than 64 fold keys in all, a null fold key; for the
 * product the null-key and count rules of tfhe_matmul_bsgs_grouped: a null key among the first n_baby / n_giant, a null diags[m] or
 * cts[m] among the first n_in, n_baby / n_giant outside [0, 64], n_in outside [1, 64] (all TFHE_E_BADARG); for the baby keys, then the
 * giant keys, then the fold keys, in turn the shape checks of tfhe_rotate_grouped on galois[r] in that entry point's order (without any
 * key: those of tfhe_keyswitch_grouped, once); `out` starting where, or overlapping anywhere, ct / bias, any cts[m] or any diags[m]
 * (TFHE_E_BADARG).  `out` is untouched on every refusal.  batch == 0 does nothing after the checks.
 * Workspace: one borrowed block, as tfhe_matmul_bsgs_grouped.  Per ciphertext of a chunk, with step(R) = d nw + R 2 nw + R 2 level +
 * 2 level + R 2 n_special rows of N words (the rows of tfhe_matmul_diag_grouped; E lives in the R 2 level rows):
 *   tfhe_rotate_sum_grouped        step(largest fold step) + 2 * 2 level (two ciphertext buffers F)
 *   tfhe_matmul_bsgs_fold_grouped  max(step(n_baby, at least one key sum with giant steps), step(largest fold step)) + (2 n_giant + 1) 2 level
 *                                  (+ 2 * 2 level with fold steps)
 * and above N = 2^14 the largest stand-alone transform's rows once more (region 0).  No nested request. */
int tfhe_rotate_sum_grouped(tfhe_ctx *ctx, int key_limbs, int level, int n_special, int group,
                            const uint64_t *const *evks, const uint64_t *galois_elements, const int *group_sizes, int n_groups,
                            int n_digits, const uint64_t *ct, uint64_t *out, int64_t batch);
int tfhe_matmul_bsgs_fold_grouped(tfhe_ctx *ctx, int key_limbs, int level, int n_special, int group,
                                  const uint64_t *const *baby_evks, const uint64_t *baby_galois, int n_baby,
                                  const uint64_t *const *giant_evks, const uint64_t *giant_galois, int n_giant, int n_digits,
                                  const uint64_t *const *diags, const uint64_t *const *cts, int n_in,
                                  const uint64_t *const *fold_evks, const uint64_t *fold_galois, const int *fold_group_sizes, int n_fold_groups,
                                  const uint64_t *bias, uint64_t *out, int64_t batch);
/* The ciphertext product, relinearised on a grouped-digit key and optionally rescaled, in one call: tfhe_mul_relin on the keys of
 * tfhe_keyswitch_grouped (a grouped-digit key is first of all a relinearisation key: ceil(level / group) components instead of level).
 *   c1, c2: [batch][2][level][N]; ntt_in = 0: coefficient domain, 1: NTT domain (natural order).  c1 == c2 (squaring) allowed.
 *   evk, key_limbs, level, n_special, group, n_digits: as tfhe_keyswitch_grouped; the key comes from tfhe_evalkey_gen unchanged.
 *   rescale = 0: out [batch][2][level][N];  rescale = 1 (level >= 2): out [batch][2][level-1][N].  Coefficient domain.
 * The words are those of tfhe_nntt x2 (skipped with ntt_in) -> tfhe_tensor -> tfhe_inntt -> tfhe_keyswitch_grouped(polys = 3)
 * [-> tfhe_rescale] on the same packed buffers, bit for bit, every word canonical; they do not depend on the chunk
 * (tfhe_ctx_set_chunk).  (n_special, group) = (1, 1) gives the words of tfhe_mul_relin(special = 1), (0, 1) those of
 * tfhe_mul_relin(special = 0); group above level is clamped to level (one digit).
 * The product stage is tfhe_mul_relin's (fused cores at N = 2^12 .. 2^14, batched kernels elsewhere); the intermediates live in the
 * context workspace, sized once before the first launch.  With n_special >= 1 and rescale = 1 the modswitch rides on the key
 * switch's tail: it is one more step of the tail's own form, so the key switch's result is never written out and read back and the
 * rescaled words go straight into `out`.  With n_special == 0 there is no tail to ride on: the inverse transform with the addends
 * and tfhe_rescale's kernel are composed through the workspace.  rescale = 0 runs the tail of tfhe_keyswitch_grouped.
 * Checked on the host before any device use, in this order: a null argument (TFHE_E_BADARG); a negative batch (TFHE_E_BADARG);
 * ntt_in or rescale not 0 or 1 (TFHE_E_BADARG); rescale with level < 2 (TFHE_E_LEVEL_MISMATCH); out == c1 or out == c2
 * (TFHE_E_BADARG); the checks of tfhe_keyswitch_grouped with polys = 3, in that entry point's order; `out` overlapping c1 or c2 as
 * byte ranges (TFHE_E_BADARG); batch == 0 returns TFHE_OK and does nothing; (batch * 4 * level) << max(0, log2 N - 14) above 2^31 - 1
 * (TFHE_E_BADARG, the row-count bound of tfhe_mul_relin). */
int tfhe_mul_relin_grouped(tfhe_ctx *ctx, int key_limbs, int level, int n_special, int group, const uint64_t *evk, int n_digits,
                           const uint64_t *c1, const uint64_t *c2, int ntt_in, int rescale, uint64_t *out, int64_t batch);

/* ---- CKKS encode / decode (float; ckksencoding.jl:56-97, FixedRational ckks.jl:35-59) -- SURVEY §8(f) ----
 * The ring is limbs 0..level-1 of ctx.  scale = scale_mant * 2^scale_exp2 (2^40 = (1, 40); any positive scale to
 * 2^-63 relative).  slots: [batch][N/2] complex doubles (re, im interleaved), device memory.
 *   encode: slots -> ifft over the (Z/2N)^* orbit + psi-twist -> n_k = round(x_k * scale) (exact product, ties to even,
 *           ckks.jl:42) -> residues [batch][level][N], coefficient domain.
 *   decode: residues -> centred integer (exact CRT) -> Float64(n / scale) -> conj twist -> fft -> slots.
 * Float path: transform summation order differs from FFTW, so results agree with the reference to rounding.  Against the
 * exact coefficients X_k and slots (psi exact; tests/test_gpu_ckks_exact.py), with eps = 2^-53, cm the scattered slot vector
 * of length N and v = n / scale:
 *   encode: |n_k - scale X_k| <= 1/2 + scale c eps log2(N) ||cm||_2 / N -- the integer is rint(scale X_k) unless scale X_k
 *           lies that close to a half-integer, or scale times the error of the double x_k exceeds 1/2 (large scale |x_k|);
 *   decode: |err| <= c eps log2(N) ||v||_2  (||v||_2 <= max|slot|, so 8 log2(N) eps max|slot| holds with room);
 * measured on the MI355X for N = 4 .. 2^17: c <= 1.2 for random and one-hot inputs, up to 3.9 for alternating slots at
 * N = 2^13, whose energy lands in four coefficients (profiles/LOG.md). */
int tfhe_ckks_encode(tfhe_ctx *ctx, int level, uint64_t scale_mant, int scale_exp2, const double *slots, uint64_t *out, int64_t batch);
int tfhe_ckks_decode(tfhe_ctx *ctx, int level, uint64_t scale_mant, int scale_exp2, const uint64_t *in, double *slots, int64_t batch);

/* ---- device-side samplers for RingSampler (poly.jl:7-23; RNS crt.jl:277-279) -- SURVEY §8(f) -------------------
 * The ring is limbs 0..level-1 of ctx; out: [count][level][N], coefficient domain.  The random stream is Philox4x32-10
 * keyed by `seed`, counter = (coefficient index, polynomial index first_poly + p < 2^32, attempt/limb, stream) -- defined in
 * csrc/sample_kernels.h and restated in oracle/spec.py (Julia's generator cannot be matched).
 *   uniform : independent exactly-uniform residues per limb (rejection sampling).
 *   gaussian: multiplier * round(N(0, sigma^2)) (Box-Muller, ties to even), the same integer in every limb
 *             (multiplier = 1 for BFV/CKKS noise and secrets, = t for BGV, bgv.jl:27-34). */
int tfhe_sample_uniform(tfhe_ctx *ctx, int level, uint64_t seed, uint32_t stream, uint64_t first_poly, uint64_t *out, int64_t count);
int tfhe_sample_gaussian(tfhe_ctx *ctx, int level, double sigma, uint64_t multiplier, uint64_t seed, uint32_t stream, uint64_t first_poly, uint64_t *out, int64_t count);

/* ---- K12/K13: BFV multiplication (rlwe_she.jl:247-262 with bfv.jl:34-40,172-226) ---------------
 * plan = (ℛ = small ctx limbs idx_s, ℛbig = big ctx limbs idx_b, t).  Supported basis relations:
 * ℛbig ⊇ ℛ as sets of primes, or disjoint (test/bfv_crt.jl); anything else TFHE_E_UNSUPPORTED.
 * c1, c2: [batch][2][ns][N]; out: [batch][3][ns][N]; coefficient domain. Exact (bit-identical to
 * the BigInt path). */
int tfhe_bfv_plan_create(tfhe_ctx *small, const int32_t *idx_s, int ns, tfhe_ctx *big, const int32_t *idx_b, int nb, uint64_t t, tfhe_bfv_plan **out);
int tfhe_bfv_plan_destroy(tfhe_bfv_plan *plan);
int tfhe_bfv_mul(tfhe_bfv_plan *plan, const uint64_t *c1, const uint64_t *c2, uint64_t *out, int64_t batch);
/* mul_expand (bfv.jl:34, switch :222-226) and mul_contract (bfv.jl:35-40) exposed on their own */
int tfhe_bfv_expand(tfhe_bfv_plan *plan, const uint64_t *src, uint64_t *dst, int64_t count);   /* [count][ns][N] -> [count][nb][N] */
int tfhe_bfv_contract(tfhe_bfv_plan *plan, const uint64_t *src, uint64_t *dst, int64_t count); /* [count][nb][N] -> [count][ns][N] */
/* c1*c2 followed by keyswitch(evk, ·) on the small ring (the BASELINE.json "ciphertext-mul +
 * relinearize" unit): out [batch][2][ns][N].  The key ring is ℛ itself (special == 0), which must be
 * limbs 0..ns-1 of the small ctx; evk: [n_digits][2][ns][N]. */
int tfhe_bfv_mul_relin(tfhe_bfv_plan *plan, const uint64_t *evk, int n_digits, const uint64_t *c1, const uint64_t *c2, uint64_t *out, int64_t batch);
/* expand/contract kernel family: 0 = auto (register-resident constant-folded kernels when ℛbig ⊇ ℛ and the
 * limb counts are instantiated, else the general kernels), 1 = force the general kernels (cross-check). */
int tfhe_bfv_plan_set_variant(tfhe_bfv_plan *plan, int variant);
/* ciphertexts processed per internal chunk (workspace = chunk * (7 nb + 3 ns) * N * 8 bytes); 0 = default (256) */
int tfhe_bfv_plan_set_chunk(tfhe_bfv_plan *plan, int chunk);
/* the plan's own workspace, as tfhe_ctx_workspace (the transforms inside a BFV call also use the two contexts' workspaces) */
int tfhe_bfv_plan_workspace(const tfhe_bfv_plan *plan, void **ptr, size_t *bytes);

/* ---- CKKS / BGV: ciphertext product + relinearisation (+ modswitch) in one call ------------------------------------
 * c1*c2 (rlwe_she.jl:247-262, mul_expand/mul_contract = identity) -> keyswitch(evk, .) (rlwe_she.jl:315-347; ModulusRaised
 * modulusraising.jl:35-49) -> optionally modswitch of both components (crt.jl:215-228; ckksencoding.jl:127-130).
 *   c1, c2: [batch][2][level][N]; ntt_in = 0: coefficient domain, 1: NTT domain (natural order).  c1 == c2 (squaring) allowed.
 *   evk, key_limbs, level, special, n_digits: as tfhe_keyswitch (RNS digits).
 *   rescale = 0: out [batch][2][level][N];  rescale = 1 (level >= 2): out [batch][2][level-1][N].  Coefficient domain.
 * The words are those of tfhe_nntt x2 -> tfhe_tensor -> tfhe_inntt -> tfhe_keyswitch(polys = 3) -> tfhe_rescale on the same
 * packed buffers, bit for bit; the intermediates live in the context workspace (no pack / unpack copies).
 * The product (transforms + tensor) of a ring whose limbs are all of fp64 size (q < 2^50 + 2^40) at N = 2^12 .. 2^14 runs in one
 * fused kernel per chunk (4 rows read + 3 written per limb; 2 read when squaring); rings with a larger limb, N < 2^12,
 * N >= 2^15 and tfhe_ctx_set_ntt_variant != 0 run the batched transform / tensor kernels on the packed layout.
 * Checks (host, before any device use): as tfhe_keyswitch; rescale with level < 2 is TFHE_E_LEVEL_MISMATCH; `out` overlapping
 * c1 or c2 as address ranges is TFHE_E_BADARG; batch == 0 does nothing.  The BFV product is tfhe_bfv_mul_relin. */
int tfhe_mul_relin(tfhe_ctx *ctx, int key_limbs, int level, int special, const uint64_t *evk, int n_digits,
                   const uint64_t *c1, const uint64_t *c2, int ntt_in, int rescale, uint64_t *out, int64_t batch);

/* ---- public-key encryption and the decryption phase of a batch, one call each (rlwe_she.jl:176-216) ------------------
 * The ring is limbs 0..level-1 of ctx, 1 <= level <= key_limbs <= the context's limbs; level < key_limbs is the ModulusRaised
 * case (modulusraising.jl:23-26): everything here is limb-wise, so "encrypt over the key ring, then drop the last limb" gives
 * the words of never computing that limb.
 * tfhe_encrypt (rlwe_she.jl:176-195):
 *   pk  : [2][key_limbs][N], (mask, masked) as in the evaluation-key layout, NTT domain, natural order.
 *   out : [batch][2][level][N], coefficient domain, canonical residues:
 *           component 0 = masked u + e1 (+ msg),  component 1 = mask u + e2.
 *   msg : NULL encrypts zero; else [batch][level][N], coefficient domain (tfhe_plain_encode / tfhe_ckks_encode output).
 *   rand == NULL: the Gaussian stream of tfhe_sample_gaussian (Philox; counter convention): u_b is polynomial first_poly + b
 *           with sigma_u and multiplier 1, e1_b is polynomial first_poly + batch + b and e2_b polynomial first_poly + 2 batch + b,
 *           both with sigma_e and multiplier mult_e (1 for BFV / CKKS, t for BGV, bgv.jl:27-34) -- exactly the words of three
 *           tfhe_sample_gaussian(.., stream, first_poly + k batch, .., batch) calls.  first_poly + 3 batch must not exceed 2^32.
 *   rand != NULL: device int32 [batch][3][N] holding u, e1, e2 as signed integers (a host CSPRNG's draws); e is still
 *           multiplied by mult_e; seed, stream, first_poly and the sigmas are ignored.
 * tfhe_decrypt_phase (rlwe_she.jl:199-212): out = c1 + s c2 (+ s^2 c3).
 *   secret : [key_limbs][N], NTT domain; its first `level` rows are used.
 *   ct     : [batch][polys][level][N]; ntt_in = 0: coefficient domain, 1: NTT domain.  polys is 2 or 3, anything else is
 *            TFHE_E_UNSUPPORTED.
 *   out    : [batch][level][N], coefficient domain, canonical: the input of tfhe_plain_decode / tfhe_bfv_noise_max /
 *            tfhe_ckks_decode.
 * N = 2^12 .. 2^14 (tfhe_ctx_set_ntt_variant 0, level <= 32) runs as one fused kernel per arithmetic policy: per
 * (ciphertext, limb) one message row read and two ciphertext rows written (encrypt), polys rows read and one written (decrypt);
 * a ring that mixes 60-bit and fp64-size moduli runs its two launches side by side.  N < 2^12, N >= 2^15 and variant != 0 run
 * the batched transforms on the packed layout with streaming kernels around them.  Same words on every path.
 * Checks (host, before any device use, in this order): a null pk / secret / ct / out is TFHE_E_BADARG; negative batch
 * TFHE_E_BADARG; level outside [1, key_limbs] or key_limbs above the context's TFHE_E_LEVEL_MISMATCH; counter overflow
 * TFHE_E_BADARG; `out` overlapping pk, msg, rand, ct or secret as address ranges TFHE_E_BADARG; batch == 0 does nothing, but
 * still needs a context. */
int tfhe_encrypt(tfhe_ctx *ctx, int key_limbs, int level, const uint64_t *pk, double sigma_u, double sigma_e, uint64_t mult_e,
                 uint64_t seed, uint32_t stream, uint64_t first_poly, const int32_t *rand, const uint64_t *msg, uint64_t *out, int64_t batch);
int tfhe_decrypt_phase(tfhe_ctx *ctx, int key_limbs, int level, const uint64_t *secret, const uint64_t *ct, int polys, int ntt_in,
                       uint64_t *out, int64_t batch);

/* ---- key generation: public, relinearisation and Galois keys of a parameter set, one call (rlwe_she.jl:155-166, 273-304) ----
 * The key ring is limbs 0..key_limbs-1 of ctx.  Component m = k n_digits + i (key k < n_keys, digit i < n_digits) has at limb j
 *     evks[k][i][0][j] = NTT_j(a_m)                                                         (mask)
 *     evks[k][i][1][j] = gadget[i][j] old_k[j] - ( NTT_j(a_m) secret[j] + NTT_j(mult_e e_m) )   (masked)
 *   evks   : HOST array of n_keys device pointers, each [n_digits][2][key_limbs][N], NTT domain, natural order, canonical
 *            residues: the layout tfhe_keyswitch, tfhe_keyswitch_window, tfhe_galois_key_prepare and (n_digits = 1) tfhe_encrypt's pk
 *            consume.  Every word is written exactly once.
 *   secret : device [key_limbs][N], NTT domain.
 *   gadget : HOST [n_digits][key_limbs] canonical residues (a residue >= q_j is TFHE_E_BADARG).  RNS digits (rlwe_she.jl:287,
 *            crt.jl:64-77): gadget[i][j] = (i == j); ModulusRaised (modulusraising.jl:28-32): (i == j) P mod q_j, the row and the
 *            column of the special prime P zero; relin_window = w: (2^(i w) mod Q) mod q_j, under ModulusRaised P 2^(i w) mod Q P.
 *            Where gadget[i][j] == 0 the old term is skipped.  gadget == NULL: all zero, the PUBLIC-KEY form -(a s + e)
 *            (rlwe_she.jl:155-166); old and galois_elements are then ignored.
 *   old    : device [n_keys][key_limbs][N], NTT domain: row k is old_k.  old == NULL: galois_elements (HOST [n_keys]) names it:
 *            0 is secret . secret (the relinearisation key, rlwe_she.jl:299), an odd g < 2N is secret under x -> x^g (a Galois key,
 *            rlwe_she.jl:301-304; an index permutation of the NTT-domain row); any other value is TFHE_E_BADARG.
 *   mask_rand == noise_rand == NULL: a_m is polynomial mask_poly + m poly_stride of tfhe_sample_uniform's stream stream_mask over
 *            key_limbs limbs, e_m polynomial noise_poly + m poly_stride of tfhe_sample_gaussian's stream stream_noise with sigma_e
 *            and multiplier mult_e (1 for BFV / CKKS, t for BGV) -- exactly the words 2 n_keys n_digits sampler calls of count 1
 *            would have written, regenerated inside the kernels.  No counter may reach 2^32: mask_poly + (n_keys n_digits - 1)
 *            poly_stride < 2^32 and the same for noise_poly.  key_limbs <= 256 (the limb byte of the uniform counter).
 *   both non-NULL: a host CSPRNG's draws.  mask_rand device [n_keys][n_digits][key_limbs][N] canonical residues, coefficient
 *            domain; noise_rand device int32 [n_keys][n_digits][N] signed integers, still multiplied by mult_e; seed, the streams,
 *            the counters and sigma_e are ignored.  Exactly one of the two NULL is TFHE_E_BADARG.
 * N = 2^12 .. 2^14 (tfhe_ctx_set_ntt_variant 0, key_limbs <= 32) runs as one fused kernel per arithmetic policy: per (component,
 * limb) one secret row read and two key rows written; a ring that mixes 60-bit and fp64-size moduli runs its two launches side by
 * side.  Every other size fills rows 0 and 1 of the output itself, transforms them in place and finishes row 1.  Same words on
 * every path, and for every tfhe_ctx_set_chunk (the chunk counts components (k, i)).
 * Checks (host, before any device use, in this order): a null secret / evks is TFHE_E_BADARG; n_keys < 0 or n_digits < 1
 * TFHE_E_BADARG; key_limbs < 1 TFHE_E_LEVEL_MISMATCH; exactly one of mask_rand / noise_rand TFHE_E_BADARG; with device randomness
 * sigma_e out of range, a counter reaching 2^32 and key_limbs > 256 TFHE_E_BADARG; a null galois_elements where it is needed or a
 * null evks[k] TFHE_E_BADARG; an output starting where secret, old, mask_rand, noise_rand or another output starts TFHE_E_BADARG;
 * a null context TFHE_E_BADARG; key_limbs above the context's limbs TFHE_E_LEVEL_MISMATCH; a Galois element that is neither 0 nor
 * odd and below 2N, then a gadget residue out of range, TFHE_E_BADARG; any output overlapping secret, old, mask_rand, noise_rand or
 * another output as address ranges TFHE_E_BADARG; n_keys == 0 does nothing, but still needs a context. */
int tfhe_evalkey_gen(tfhe_ctx *ctx, int key_limbs, const uint64_t *secret, const uint64_t *old, const uint64_t *galois_elements,
                     int n_keys, const uint64_t *gadget, int n_digits, double sigma_e, uint64_t mult_e, uint64_t seed,
                     uint32_t stream_mask, uint32_t stream_noise, uint64_t mask_poly, uint64_t noise_poly, uint64_t poly_stride,
                     const uint64_t *mask_rand, const int32_t *noise_rand, uint64_t *const *evks);

/* ---- ciphertext x plaintext sums with the forward transforms inside, one call (infer.jl:140-149) -------------------------------
 *     dst_i = (acc_i +) sum_{k < n_terms} T_k(a[k]_i) .* b[k]_i        for items i < count, limb-wise
 *   T_k = NTT (tfhe_nntt, pow2_cyc_rings.jl:295-318) if a_ntt[k] == 0, the identity if a_ntt[k] == 1: the accumulation
 *   `result += rotated_k * diagonal_k` of the diagonal matrix product over rotated ciphertexts that are still in the coefficient
 *   domain.  The words are the canonical residues of tfhe_nntt followed by tfhe_mad term by term.
 * Every operand is a VIEW, a base pointer and an item stride in words: item i is [limbs][N] words at base + i * stride.
 *   a[k], acc, dst : stride >= limbs * N.  A ring element is the view (base, limbs * N); component p of a packed
 *                    [count][P][limbs][N] ciphertext is the view (base + p * limbs * N, P * limbs * N), an operand where it lies.
 *   b[k]           : NTT domain; stride 0 = one plaintext shared by the whole batch, else >= limbs * N.
 *   dst            : NTT domain.  acc is NULL or NTT domain and may be the SAME view as dst (same base, same stride); dst may
 *                    overlap no other operand and acc in no other way.
 *   a, a_stride, a_ntt, b, b_stride : HOST arrays of n_terms entries.  n_terms >= 1 with no upper limit: more than 64 terms
 *                    accumulate over further passes onto dst, as tfhe_dot does.
 * N = 2^12 .. 2^14 (tfhe_ctx_set_ntt_variant 0, limbs <= 32) runs as one fused kernel per arithmetic policy: per (item, limb) the
 * running sum stays in registers, a coefficient-domain term is transformed through the workgroup's LDS and multiplied by its
 * plaintext row as it comes out, so every source row and plaintext row is read once and the sum written once; a ring that mixes
 * 60-bit and fp64-size moduli runs its two launches side by side.  N < 2^12, N >= 2^15, variant != 0 and more than 32 limbs gather
 * the coefficient-domain terms into the context workspace, transform them in one batch and accumulate with a strided tfhe_dot.
 * Same words on every path, and for every tfhe_ctx_set_chunk (the chunk bounds the items and the terms of one pass).
 * Checks (host, before any device use, in this order): a null a / a_stride / a_ntt / b / b_stride / dst is TFHE_E_BADARG;
 * n_terms < 1 TFHE_E_BADARG; negative count TFHE_E_BADARG; a null a[k] / b[k], an a_ntt[k] outside {0, 1} and dst starting where an
 * a[k] / b[k] starts TFHE_E_BADARG; a null context TFHE_E_BADARG; limbs / limb_idx as every limb-wise entry point (TFHE_E_BADARG /
 * TFHE_E_LEVEL_MISMATCH); count * limbs above 2^31 - 1 TFHE_E_BADARG; a stride below limbs * N (other than a b stride of 0), or
 * with count * stride above 2^40 words, TFHE_E_BADARG; dst overlapping an a[k] / b[k] as strided address ranges (first item to the end of the last), or acc
 * other than as the same view, TFHE_E_BADARG and nothing is written; count == 0 does nothing, but still needs a context. */
int tfhe_dot_plain(tfhe_ctx *ctx, const uint64_t *acc, size_t acc_stride, const uint64_t *const *a, const size_t *a_stride,
                   const uint8_t *a_ntt, const uint64_t *const *b, const size_t *b_stride, int n_terms, uint64_t *dst,
                   size_t dst_stride, int64_t count, int limbs, const int32_t *limb_idx);

/* ---- BFV / BGV plaintext codecs on the device (π⁻¹ / π, bfv.jl:21-29, bgv.jl:21-25; noise, bfv.jl:137-166) ---------
 * plan = (ring = ctx limbs limb_idx, t).  t in [2, 2^62) and t < Q (Q = product of the selected moduli); limb_idx entries
 * in range and distinct; else TFHE_E_BADARG (checked on the host before any device use).  Exact: bit-identical to the
 * BigInt path of the reference.  Work runs on the ctx's stream; count == 0 does nothing.
 *   scheme         : TFHE_PLAIN_BFV or TFHE_PLAIN_BGV.
 *   encode         : m [count][N] plaintext words (any uint64; reduced mod t first: a negative plaintext arrives as its
 *                    residue mod t) -> out [count][limbs][N] coefficient domain.
 *                    BFV: (m mod t)(Δ mod q_l) mod q_l, Δ = Q ÷ t (bfv.jl:21-24).  BGV: (m mod t) mod q_l (bgv.jl:21-25).
 *   decode         : in [count][limbs][N] coefficient domain -> out [count][N] in [0, t).
 *                    BFV: mod(SignedMod(div(centred(x), Δ, RoundNearestTiesAway)), t) (bfv.jl:26-29).
 *                    BGV: mod(centred(x), t) (bgv.jl:21-25).  centred(x) = x - Q if x > Q÷2 else x (signedmod.jl:12-19).
 *   bfv_noise_max  : in [count][limbs][N] (the decryption b = c_1 + s c_2 + ...) -> out_words [count][delta_words], the exact
 *                    max over the N coefficients of birem(x) = min(x mod Δ, Δ - x mod Δ) (r <= Δ÷2 keeps r; x unsigned),
 *                    little-endian 64-bit words, delta_words = number of 64-bit words of Δ = Q ÷ t.  The host applies
 *                    log2(Q) - log2(t) - 1 - log2(max) (bfv.jl:137-166).
 * m / in / out / out_words are device memory; limb_idx is a host array (NULL = 0..limbs-1). */
typedef enum { TFHE_PLAIN_BFV = 0, TFHE_PLAIN_BGV = 1 } tfhe_plain_scheme;
int tfhe_plain_plan_create(tfhe_ctx *ctx, const int32_t *limb_idx, int limbs, uint64_t t, tfhe_plain_plan **out);
int tfhe_plain_plan_destroy(tfhe_plain_plan *plan);
int tfhe_plain_encode(tfhe_plain_plan *plan, int scheme, const uint64_t *m, uint64_t *out, int64_t count);
int tfhe_plain_decode(tfhe_plain_plan *plan, int scheme, const uint64_t *in, uint64_t *out, int64_t count);
int tfhe_bfv_noise_max(tfhe_plain_plan *plan, const uint64_t *in, uint64_t *out_words, int64_t count);

/* ---- multi-GPU: the final gather (the reference is single-process) ---------------------------------------
 * A batch of independent ciphertexts shards by ciphertext over one process per GPU (contexts and keys replicated, tens of
 * MiB); nothing is exchanged while computing.  The one optional collective is the gather of per-rank results: an all-gather
 * over RCCL (xGMI), enqueued on the context's stream.  RCCL is bound at run time (dlopen; TFHE_RCCL_LIB overrides the
 * library path), so single-GPU use has no RCCL dependency.
 *   tfhe_comm_id     : rank 0 creates the 128-byte rendezvous id; the host side (MPI.jl / Distributed / torch.distributed)
 *                      hands it to every rank.
 *   tfhe_comm_create : collective over the ranks (after tfhe_set_device on each).  The rendezvous has a deadline
 *                      (TFHE_COMM_TIMEOUT_S, default 180 s): a rank that never joins is a TFHE_E_HIP with the story in
 *                      tfhe_last_error, not a hung job.
 *   tfhe_gather      : dst [nranks][words_per_rank] <- every rank's src [words_per_rank]; equal shard sizes (pad the last). */
int tfhe_comm_id(void *id_out /* 128 bytes */);
int tfhe_comm_create(const void *id, int nranks, int rank, tfhe_comm **out);
int tfhe_comm_destroy(tfhe_comm *comm);
int tfhe_gather(tfhe_comm *comm, tfhe_ctx *ctx, const uint64_t *src, uint64_t *dst, size_t words_per_rank);

/* ---- measurement hooks (bench.py): HIP events on the ctx stream --------------------------------
 * While enabled, every NTT kernel launch is bracketed by a pair of events; read returns the number of
 * launches, the number of limb-polynomials transformed and the summed kernel time, then resets. */
int tfhe_prof_enable(tfhe_ctx *ctx, int on);
int tfhe_prof_read(tfhe_ctx *ctx, int64_t *launches, int64_t *limb_polys, double *total_ms);
int tfhe_event_create(void **ev);
int tfhe_event_destroy(void *ev);
int tfhe_event_record(tfhe_ctx *ctx, void *ev);
int tfhe_event_elapsed_ms(void *start, void *stop, float *ms); /* synchronises on `stop` */

#ifdef __cplusplus
}
#endif
#endif /* TOYFHE_HIP_H */
