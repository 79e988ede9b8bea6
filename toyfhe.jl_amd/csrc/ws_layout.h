// ws_layout.h -- how one call lays out the context workspace, and who may take the transform scratch at its start.  Host only, no HIP:
// tests/ws_layout_emul compiles it with the host compiler.
//
// The block of one call, for chunks of `chunk` ciphertexts:
//     [ region 0 | row region 0: [chunk][rows_0][N] | row region 1 | ... | tail 0: bytes | tail 1 | ... ]
// Region 0 is the start of the block.  The stand-alone transforms above N = 2^14 take their intermediate there, the mixed lifts of
// ks_digits_fwd and md_lift_fwd do, and so does a nested user (a key switch inside a product) that is handed region 0 as its span and
// lays out its own block in it.  It holds the larger of chunk x scratch_rows rows (above N = 2^14 only) and the nested user's bytes,
// rounded up to 256 bytes; it is empty when nothing asks for it.  Every region is declared once, in the order it lies in memory; the
// size of the block and every pointer into it come from that one list.
#pragma once
#include <algorithm>
#include <cassert>
#include <cstddef>
#include <cstdint>
#include <functional>

struct ws_region_t { int i; };   // a declared region of a ws_layout_t
struct ws_span_t { void* ptr; size_t bytes; };   // what a nested user is handed instead of the context's block: its caller's region 0

struct ws_layout_t {
    static constexpr int MAX_REGIONS = 12;
    static constexpr size_t SCRATCH_ABOVE_N = (size_t)1 << 14;   // transforms up to this size run in one kernel: no intermediate
    size_t N = 0;
    size_t scratch_rows = 0;                    // rows per ciphertext of the largest stand-alone transform
    std::function<size_t(int64_t)> nested;      // bytes a nested user asks of its span for `chunk` ciphertexts
    int n_rows = 0, n_tails = 0;
    size_t rows_of[MAX_REGIONS] = {};           // row regions: rows (N words) per ciphertext
    size_t bytes_of[MAX_REGIONS] = {};          // tail regions: bytes, whatever the chunk

    ws_layout_t() = default;
    explicit ws_layout_t(size_t n) : N(n) {}
    // declared first, if at all
    void scratch(size_t rows_per_ct, std::function<size_t(int64_t)> nested_bytes = nullptr) {
        assert(n_rows == 0 && n_tails == 0);
        scratch_rows = rows_per_ct;
        nested = std::move(nested_bytes);
    }
    ws_region_t rows(size_t rows_per_ct) {
        assert(n_tails == 0 && n_rows < MAX_REGIONS);
        rows_of[n_rows] = rows_per_ct;
        return ws_region_t{n_rows++};
    }
    ws_region_t tail(size_t bytes) {
        assert(n_tails < MAX_REGIONS);
        bytes_of[n_tails] = bytes;
        return ws_region_t{MAX_REGIONS + n_tails++};
    }

    size_t rows_per_ct() const { return rows_before(n_rows); }
    size_t per_ct_bytes() const { return rows_per_ct() * N * 8; }   // the chunked rows of one ciphertext (what chunk_of divides by)
    size_t region0(int64_t chunk) const {
        size_t r0 = N > SCRATCH_ABOVE_N ? (size_t)chunk * scratch_rows * N * 8 : 0;
        if (nested) r0 = std::max(r0, nested(chunk));
        return (r0 + 255) & ~(size_t)255;
    }
    size_t offset(int64_t chunk, ws_region_t h) const {
        if (h.i < MAX_REGIONS) return region0(chunk) + (size_t)chunk * rows_before(h.i) * N * 8;
        size_t off = region0(chunk) + (size_t)chunk * per_ct_bytes();
        for (int t = 0; t < h.i - MAX_REGIONS; t++) off += bytes_of[t];
        return off;
    }
    size_t bytes(int64_t chunk) const { return offset(chunk, ws_region_t{MAX_REGIONS + n_tails}); }   // the end of the last tail
    uint64_t* at(void* ws, int64_t chunk, ws_region_t h) const { return (uint64_t*)((char*)ws + offset(chunk, h)); }

private:
    size_t rows_before(int i) const {
        size_t r = 0;
        for (int k = 0; k < i; k++) r += rows_of[k];
        return r;
    }
};

// ---- the transform scratch -----------------------------------------------------------------------------------------------------------
// Whoever needs the intermediate of a transform asks the one accessor (ws_scratch, toyfhe_hip.hip), which decides here.  No layout in
// force (a bare tfhe_nntt, the single-user entry points): the context's block grows to the request, as it always did.  A layout in
// force: the block is laid out and must not move, the request is served from region 0 or refused -- a reservation one term short is an
// error, not scratch over the caller's key sums.
struct ws_scratch_state_t { bool in_force = false; size_t region0 = 0; };
enum ws_scratch_t { WS_SCRATCH_GROW, WS_SCRATCH_FITS, WS_SCRATCH_REFUSED };
inline ws_scratch_t ws_scratch_decide(const ws_scratch_state_t& s, size_t bytes) {
    if (!s.in_force) return WS_SCRATCH_GROW;
    return bytes <= s.region0 ? WS_SCRATCH_FITS : WS_SCRATCH_REFUSED;
}
// A layout is in force from the call's one allocation to its return, on every path; a nested user's tighter region 0 while it runs.
struct ws_scope_t {
    ws_scratch_state_t* s = nullptr;
    ws_scratch_state_t prev;
    ws_scope_t() = default;
    ws_scope_t(ws_scratch_state_t& st, size_t region0) { set(st, region0); }
    ws_scope_t(const ws_scope_t&) = delete;
    ws_scope_t& operator=(const ws_scope_t&) = delete;
    void set(ws_scratch_state_t& st, size_t region0) {
        assert(!s);
        s = &st;
        prev = st;
        st = ws_scratch_state_t{true, region0};
    }
    ~ws_scope_t() { if (s) *s = prev; }
};
