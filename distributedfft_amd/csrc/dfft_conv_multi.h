// dfft_conv_multi.h -- the K-output X stage of the multi-output real-field spectral-filter plans, dfft_plan_create_conv_real_multi
// (dfft_conv_multi.hip): forward transform along X once, multiply by the plan's one filter copy once, then per output k the separable
// factors a_k[x] . b_k[row] . c_k[col] and the inverse transform along X into slab k.  Internal header (the C-ABI is include/dfft.h).
#pragma once
#include <hip/hip_runtime.h>

#include "dfft_conv.h"

namespace dfft {

constexpr int CONV_MAX_OUTPUTS = 8;  // DFFT_CONV_MAX_OUTPUTS of include/dfft.h

// The K slabs and the factor tables, passed to the kernels BY VALUE (one kernel argument; no table of pointers in memory).
// Every slab has the layout of ConvLaunch (plain rows: real-field plans never rotate); out[0] may be the input slab.
// ax[k]: N0 complex elements of the dtype; by[k]: `rows` elements (the plan's own part of the caller's vector, from y0);
// cz[k]: `ncols` elements, zeros behind N2/2 + 1, on a 16-byte boundary (fp32 reads it as column pairs).  Never NULL: a factor nobody
// set points at a table of ones.
struct ConvMultiArgs {
    void*       out[CONV_MAX_OUTPUTS];
    const void* ax[CONV_MAX_OUTPUTS];
    const void* by[CONV_MAX_OUTPUTS];
    const void* cz[CONV_MAX_OUTPUTS];
};

// Fused form (xconv_multi_cols_kernel; the fused lengths and tile geometry of dfft_conv.hip): reads L.in and L.filt, writes M.out[0 .. K).
// L.out and L.rot are not used (rot must be 0).  Whether it applies: conv_fused_applies(L).
hipError_t launch_conv_multi_fused(const ConvLaunch& L, const ConvMultiArgs& M, int K, hipStream_t stream);
// Multi route, output k: dst[i] = src[i] . ax[x] . by[row] . cz[col] over the whole slab of L's layout (16-byte accesses; columns
// ncols .. pitch - 1 receive zeros); dst == src is allowed.
hipError_t launch_conv_factor_mul(const ConvLaunch& L, const void* src, void* dst, const void* ax, const void* by, const void* cz,
                                  hipStream_t stream);

}  // namespace dfft

#ifdef DFFT_CONV_MULTI_DEVICE
// The traits of dfft_conv.hip the K-output kernel needs, restated (they live inside that unit, which stays as it is): the plan of a
// length, the tile geometry, and the filter element per data type and filter kind.
#include "dfft_fft_impl.h"
#include "dfft_plans.h"

namespace dfft {

constexpr bool xm_fused_n(int n) { return n == 64 || n == 128 || n == 256 || n == 384 || n == 512 || n == 768 || n == 1024; }

template <int N> struct XmPlanFor;
#define DFFT_DECL_XM_PLAN(N, GRP, E, ...) \
    template <> struct XmPlanFor<N> { using type = Plan<N, E, __VA_ARGS__>; };
DFFT_PLAN_TABLE(DFFT_DECL_XM_PLAN)
#undef DFFT_DECL_XM_PLAN

// full-line tiles of 8 elements of 16 bytes, at most 512 threads per workgroup (XcGeom)
template <class V, class P> struct XmGeom {
    static constexpr int CB = cols_per_tile<V, P>();
    static_assert(CB * (int)sizeof(V) == 128 && CB * P::T <= 512, "fused conv lengths use full-line tiles of at most 512 threads");
    static constexpr int G = ConstMax1<256 / (CB * P::T)>::value;
    using KG = KernelGeom<V, P, CB, G, TuneDefault>;
    static_assert(KG::PH == 1, "single-phase tiles only");
};

// filter element as it lies in memory (XcFilter)
template <class V, bool REAL> struct XmFilter;
template <> struct XmFilter<double2, false> {
    using T = double2;
    static __device__ __forceinline__ double2 mul(double2 a, T h) { return double2{a.x * h.x - a.y * h.y, a.x * h.y + a.y * h.x}; }
};
template <> struct XmFilter<double2, true> {
    using T = double;
    static __device__ __forceinline__ double2 mul(double2 a, T h) { return double2{a.x * h, a.y * h}; }
};
template <> struct XmFilter<cpair, false> {
    using T = f32x4;  // (re0, im0, re1, im1) of two adjacent columns
    static __device__ __forceinline__ cpair mul(cpair a, T g) {
        const cpair h = VecTraits<cpair>::from_g(g);
        return cpair{a.x * h.x - a.y * h.y, a.x * h.y + a.y * h.x};
    }
};
template <> struct XmFilter<cpair, true> {
    using T = f32x2;  // the two columns' reals
    static __device__ __forceinline__ cpair mul(cpair a, T h) { return cpair{a.x * h, a.y * h}; }
};
template <class V> __device__ __forceinline__ V xm_conj(V a) { return V{a.x, -a.y}; }

}  // namespace dfft
#endif
