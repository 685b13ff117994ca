// dfft_conv_impl.h -- what the fused X-stage kernels of the spectral-filter plans share (xconv_cols_kernel, dfft_conv.hip;
// xconv_multi_cols_kernel, dfft_conv_multi.hip): the fused lengths, the tile geometry, the filter element per data type and filter kind,
// where the filter is read, and the host side of the tiling.  Device-only header: the kernel units include it, nothing else does.
#pragma once
#include <algorithm>

#include "dfft_fft_impl.h"
#include "dfft_plans.h"
#include "dfft_conv.h"

namespace dfft {

constexpr bool conv_fused_n(int n) { return n == 64 || n == 128 || n == 256 || n == 384 || n == 512 || n == 768 || n == 1024; }

// Geometry: full-line tiles (the C2C column kernel's cols_per_tile: 8 elements of 16 bytes for every fused length -- the 1024-point tile
// is 128 KiB of the CU's 160 KiB LDS), at most 512 threads per workgroup so that a thread may use 256 registers: it keeps its E points
// live across two transforms while up to E filter elements are in flight.
template <class V, class P> struct XcGeom {
    static constexpr int CB = cols_per_tile<V, P>();
    static_assert(CB * (int)sizeof(V) == 128 && CB * P::T <= 512, "fused conv lengths use full-line tiles of at most 512 threads");
    static constexpr int G = ConstMax1<256 / (CB * P::T)>::value;
    using KG = KernelGeom<V, P, CB, G, TuneDefault>;
    static_assert(KG::PH == 1, "single-phase tiles only");
};

// filter element as it lies in memory, per data type V and filter kind
template <class V, bool REAL> struct XcFilter;
template <> struct XcFilter<double2, false> {
    using T = double2;
    static __device__ __forceinline__ double2 mul(double2 a, T h) { return double2{a.x * h.x - a.y * h.y, a.x * h.y + a.y * h.x}; }
};
template <> struct XcFilter<double2, true> {
    using T = double;
    static __device__ __forceinline__ double2 mul(double2 a, T h) { return double2{a.x * h, a.y * h}; }
};
template <> struct XcFilter<cpair, false> {
    using T = f32x4;  // (re0, im0, re1, im1) of two adjacent columns
    static __device__ __forceinline__ cpair mul(cpair a, T g) {
        const cpair h = VecTraits<cpair>::from_g(g);
        return cpair{a.x * h.x - a.y * h.y, a.x * h.y + a.y * h.x};
    }
};
template <> struct XcFilter<cpair, true> {
    using T = f32x2;  // the two columns' reals
    static __device__ __forceinline__ cpair mul(cpair a, T h) { return cpair{a.x * h, a.y * h}; }
};

// The filter loads are issued right behind the data loads wherever data and filter fit the thread's registers together: always in
// workgroups of at most 256 threads (one wave per SIMD may use 512 registers: 384 points, 96 + 96), and in 512-thread workgroups (256
// registers) up to 12 points.  16 points of 16 bytes with a complex filter (1024 points: 64 + 64 registers, next to 16 offsets and the
// butterflies' temporaries) do not fit -- that form kept 92-124 bytes per lane in scratch -- and read the filter between the two
// transforms instead.
template <class V, class P, bool REAL> constexpr bool conv_filter_early() {
    return REAL || P::E * (int)sizeof(V) / 4 < 64 || XcGeom<V, P>::KG::THREADS <= 256;
}

// Host side of the tiling: the slab in units of one V (fp32: pairs of columns), tiles of CB columns of one row.
template <class V, class P> struct ConvTiles {
    long long ncols, plane, pitch, per_row, tiles;
    explicit ConvTiles(const ConvLaunch& L) {
        constexpr int LANES = VecTraits<V>::LANES, CB = XcGeom<V, P>::CB;
        ncols = L.ncols / LANES, plane = L.plane / LANES, pitch = L.pitch / LANES;
        per_row = (ncols + CB - 1) / CB, tiles = L.rows * per_row;
    }
    // 32-bit offsets inside a row's columns, 32-bit tile counts: the largest element offset is below (n0 - 1) * plane + pitch
    bool fits32(const ConvLaunch& L) const { return tiles >= 1 && tiles < (1ll << 31) && (long long)L.n0 * plane + pitch < (1ll << 32); }
};

// grid of the elementwise kernels of the multi routes (multiply, re-layout, factor multiply): 256 threads per element group
inline unsigned xc_grid(long long total) { return (unsigned)std::max(1ll, std::min((total + 255) / 256, (long long)device_info().cus * 16)); }

}  // namespace dfft
