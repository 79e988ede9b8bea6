// The workspace layout type and the transform-scratch decision of csrc/ws_layout.h on the host: C entry points for
// tests/test_ws_layout_cpu.py, which restates the arithmetic in Python, and -- with -DWS_LAYOUT_EMUL_MAIN -- a stand-alone program
// that runs the same table against the layout's own invariants (built with -fsanitize=address,undefined by the test).
#include <cstdio>

#include "../../toyfhe.jl_amd/csrc/ws_layout.h"

namespace {

// the table: every combination of ring size, chunk, scratch rows, nested user, row regions and tails below
const uint64_t T_N[] = {2, 16, (uint64_t)1 << 15};                  // 8 N is no multiple of 256 for the first two
const int64_t T_CHUNK[] = {1, 512};
const uint64_t T_SCRATCH[] = {0, 7};
const uint64_t T_NESTED[][3] = {{0, 0, 0}, {1, 1000, 24}, {1, 0, 1 << 20}};   // present, fixed bytes, bytes per ciphertext
const uint64_t T_ROWS[][5] = {{0}, {1, 3}, {4, 8, 20, 0, 6}};        // count, rows per ciphertext ...
const uint64_t T_TAILS[][3] = {{0}, {1, 40}, {2, 8 * 100, 24}};      // count, bytes ...
template <class T, size_t K> constexpr int len(const T (&)[K]) { return (int)K; }
const int N_CASES = len(T_N) * len(T_CHUNK) * len(T_SCRATCH) * len(T_NESTED) * len(T_ROWS) * len(T_TAILS);

}  // namespace

extern "C" {

int ws_layout_emul_cases() { return N_CASES; }
// in: N, chunk, scratch rows, nested present / fixed / per ciphertext, n_rows, rows[4], n_tails, tails[2]  (14 words)
void ws_layout_emul_case(int i, uint64_t* in) {
    auto pick = [&](int n) { const int k = i % n; i /= n; return k; };
    const uint64_t* tl = T_TAILS[pick(len(T_TAILS))];
    const uint64_t* rw = T_ROWS[pick(len(T_ROWS))];
    const uint64_t* ne = T_NESTED[pick(len(T_NESTED))];
    in[2] = T_SCRATCH[pick(len(T_SCRATCH))];
    in[1] = (uint64_t)T_CHUNK[pick(len(T_CHUNK))];
    in[0] = T_N[pick(len(T_N))];
    for (int k = 0; k < 3; k++) in[3 + k] = ne[k];
    in[6] = rw[0];
    for (int k = 0; k < 4; k++) in[7 + k] = k < (int)rw[0] ? rw[1 + k] : 0;
    in[11] = tl[0];
    for (int k = 0; k < 2; k++) in[12 + k] = k < (int)tl[0] ? tl[1 + k] : 0;
}
// out: region 0, per_ct_bytes, bytes(chunk), then the offset of every row region and every tail in declaration order -- as at() gives
// them from a base pointer
void ws_layout_emul(const uint64_t* in, uint64_t* out) {
    ws_layout_t L((size_t)in[0]);
    const int64_t chunk = (int64_t)in[1];
    const uint64_t fixed = in[4], per = in[5];
    if (in[3]) L.scratch((size_t)in[2], [=](int64_t ch) { return (size_t)(fixed + (uint64_t)ch * per); });
    else if (in[2]) L.scratch((size_t)in[2]);
    ws_region_t h[6];
    int n = 0;
    for (int k = 0; k < (int)in[6]; k++) h[n++] = L.rows((size_t)in[7 + k]);
    for (int k = 0; k < (int)in[11]; k++) h[n++] = L.tail((size_t)in[12 + k]);
    static char base[1];
    out[0] = L.region0(chunk);
    out[1] = L.per_ct_bytes();
    out[2] = L.bytes(chunk);
    for (int k = 0; k < n; k++) out[3 + k] = (uint64_t)((char*)L.at(base, chunk, h[k]) - base);
}
// the accessor's decision for a request of `bytes`: 0 grow, 1 fits region 0, 2 refused
int ws_scratch_emul(int in_force, uint64_t region0, uint64_t bytes) {
    ws_scratch_state_t st;
    if (!in_force) return (int)ws_scratch_decide(st, (size_t)bytes);
    const ws_scope_t scope(st, (size_t)region0);
    return (int)ws_scratch_decide(st, (size_t)bytes);
}
// an outer layout, a nested user's tighter one, and the returns: the decisions for `bytes` inside the inner scope, back in the
// outer one, and after both, as d_inner + 4 d_outer + 16 d_after
int ws_scope_emul(uint64_t outer, uint64_t inner, uint64_t bytes) {
    ws_scratch_state_t st;
    int d = 0;
    {
        const ws_scope_t a(st, (size_t)outer);
        {
            const ws_scope_t b(st, (size_t)inner);
            d += (int)ws_scratch_decide(st, (size_t)bytes);
        }
        d += 4 * (int)ws_scratch_decide(st, (size_t)bytes);
    }
    return d + 16 * (int)ws_scratch_decide(st, (size_t)bytes);
}

}  // extern "C"

#ifdef WS_LAYOUT_EMUL_MAIN
int main() {
    int bad = 0;
    for (int i = 0; i < ws_layout_emul_cases(); i++) {
        uint64_t in[14], out[9];
        ws_layout_emul_case(i, in);
        ws_layout_emul(in, out);
        const uint64_t chunk = in[1], N = in[0];
        const int nr = (int)in[6], nt = (int)in[11];
        bool ok = out[0] % 256 == 0;
        if (!in[3] && (N <= ((uint64_t)1 << 14) || !in[2])) ok = ok && out[0] == 0;
        uint64_t end = out[0];                                   // regions in declaration order, each starting where the last ended
        for (int k = 0; k < nr + nt; k++) {
            ok = ok && out[3 + k] == end;
            end += k < nr ? chunk * in[7 + k] * N * 8 : in[12 + k - nr];
        }
        ok = ok && out[2] == end;
        ok = ok && ws_scratch_emul(1, out[0], out[0]) == 1 && ws_scratch_emul(1, out[0], out[0] + 1) == 2 && ws_scratch_emul(0, out[0], out[0] + 1) == 0;
        if (!ok) { std::printf("case %d fails\n", i); bad++; }
    }
    if (ws_scope_emul(1024, 256, 512) != 2 + 4 * 1 + 16 * 0) { std::printf("scope nesting fails\n"); bad++; }
    std::printf("%d cases, %d bad\n", ws_layout_emul_cases(), bad);
    return bad != 0;
}
#endif
