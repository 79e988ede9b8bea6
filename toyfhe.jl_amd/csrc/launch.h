// launch.h -- the one place where kernels are launched; included by toyfhe_hip.hip after tfhe_ctx, fail() and HIP_TRY.
// Everything a launch site used to write out by hand lives here: raising the dynamic-LDS limit of a kernel once, the launch,
// the error check, the profiling bracket, the grid rules that recur, and the run-time integer -> template argument dispatch.
#pragma once

namespace {

// ---- dynamic LDS --------------------------------------------------------------------------------------------------------
// A kernel that asks for dynamic LDS has hipFuncAttributeMaxDynamicSharedMemorySize raised to what it asks for before its first
// launch.  The record is keyed by (device, kernel pointer): the ROCm headers say nothing about the scope of the attribute (only
// that AMD devices may ignore such hints), a process may drive several devices (tfhe_set_device, dev_alloc.h), and the runtime
// resolves a host function per device -- so it is raised again on every device a kernel runs on, which is right under either
// reading.  The pointer is a run-time value at many sites (`cond ? k<A> : k<B>`), hence a map and not a template parameter.
// Contexts may be used from different threads (include/toyfhe_hip.h): the map is behind a mutex.  A kernel whose LDS size
// depends on the ring (k_ntt_*_generic, k_galois_lds, the general BFV conversions) is raised again when a call needs more than
// any before it.  One uncontended lock and one lookup per LDS launch; nothing is allocated once a kernel has been seen.
inline int lds_ensure(const void* kern, size_t bytes) {
    static std::mutex mu;
    static std::map<std::pair<int, const void*>, size_t> raised;
    const std::pair<int, const void*> key(devalloc::current_device(), kern);
    std::lock_guard<std::mutex> g(mu);
    auto it = raised.find(key);
    if (it != raised.end() && it->second >= bytes) return TFHE_OK;
    HIP_TRY(hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    if (it != raised.end()) it->second = bytes; else raised.emplace(key, bytes);
    return TFHE_OK;
}

// ---- the launch ---------------------------------------------------------------------------------------------------------
// on the context's current stream (main or side lane, lanes_t); the BFV / plain plans launch through their context
template <class K, class... Args>
int launch(tfhe_ctx* c, K kern, dim3 grid, dim3 block, size_t lds, const Args&... args) {
    if (lds) {
        const int rc = lds_ensure(reinterpret_cast<const void*>(kern), lds);
        if (rc) return rc;
    }
    hipLaunchKernelGGL(kern, grid, block, lds, c->stream, args...);
    HIP_TRY(hipGetLastError());
    return TFHE_OK;
}

// ---- profiling bracket ----------------------------------------------------------------------------------------------------
// One event pair around the launches made while the scope lives, counted by tfhe_prof_read as one launch of `limb_polys` limb
// transforms (0: recorded, not counted).  Launches outside any scope record nothing.
struct prof_scope {
    tfhe_ctx* c;
    prof_scope(tfhe_ctx* ctx, int64_t limb_polys) : c(ctx) {
        if (!c->prof) return;
        prof_pair p;
        hipEventCreate(&p.a);
        hipEventCreate(&p.b);
        p.limb_polys = limb_polys;
        hipEventRecord(p.a, c->stream);
        c->prof_pairs.push_back(p);
    }
    ~prof_scope() {
        if (c->prof) hipEventRecord(c->prof_pairs.back().b, c->stream);
    }
    prof_scope(const prof_scope&) = delete;
    prof_scope& operator=(const prof_scope&) = delete;
};
template <class K, class... Args>
int launch_prof(tfhe_ctx* c, int64_t limb_polys, K kern, dim3 grid, dim3 block, size_t lds, const Args&... args) {
    prof_scope p(c, limb_polys);
    return launch(c, kern, grid, block, lds, args...);
}

// ---- grids ----------------------------------------------------------------------------------------------------------------
// grid of the row-wise kernels (one limb row per blockIdx.x): few rows -- a single ciphertext at N = 2^16 is 14 -- are
// split over blockIdx.y so that the launch still covers the chip (about 2048 workgroups, at least 1024 coefficients each)
inline dim3 row_grid(unsigned rows, size_t n) {
    const unsigned want = rows ? (2048u + rows - 1) / rows : 1u;
    const unsigned cap = (unsigned)std::max<size_t>(1, n / 1024);
    return dim3(rows, std::max(1u, std::min(want, cap)));
}
// persistent workgroups of 2^logt threads, LDS-limited: as many as are co-resident, each loops over items
inline unsigned persistent_per_cu(size_t lds, int logt) {
    return (unsigned)std::max<size_t>(1, std::min<size_t>({(size_t)8, (size_t)(160 * 1024) / lds, (size_t)2048 >> logt}));
}
inline unsigned persistent_grid(const tfhe_ctx* c, unsigned items, size_t lds, int logt) {
    return std::min(items, (unsigned)c->num_cus * persistent_per_cu(lds, logt));
}
// one workgroup per CU (`per_cu`: where two fit), each loops over items
inline unsigned cu_grid(const tfhe_ctx* c, unsigned items, unsigned per_cu = 1u) { return std::min(items, per_cu * (unsigned)c->num_cus); }

// ---- run-time integer -> template argument ----------------------------------------------------------------------------------
// f(std::integral_constant<int, V>{}) for the V in [LO, HI] that equals v; the range is the set of instantiations, per call site
template <int LO, int HI, class F>
int dispatch_int(int v, F&& f) {
    if constexpr (LO > HI) {
        return fail(TFHE_E_UNSUPPORTED, "internal: %d has no instantiated kernel here", v);
    } else {
        if (v == LO) return f(std::integral_constant<int, LO>{});
        return dispatch_int<LO + 1, HI>(v, f);
    }
}

}  // namespace
