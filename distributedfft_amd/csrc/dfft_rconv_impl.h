// dfft_rconv_impl.h -- device-side types shared by the fused kernels of the 1-D real FFT convolution: rconv_rows_kernel (dfft_rconv.hip,
// one padded row per thread group) and osconv_blocks_kernel (dfft_osconv.hip, one overlap-save block per thread group).  Both load
// m = 2 M reals as the M complex values z[j] = x[2j] + i x[2j+1], run the forward M-point stages, pair / multiply / merge, run the
// stages again and store Re / -Im of the result; they differ in where the reals come from and go to.  Internal header.
#pragma once
#include "dfft_fft_impl.h"

namespace dfft {

// Geometry: RealGeom of dfft_real.hip (one M-point FFT per thread group, about 256 threads per workgroup, twiddles where KernelGeom
// puts them; the tile of a group holds the M bins of the pairing step in natural order).
template <class V, class P> struct RconvGeom {
    static constexpr int G = ConstMax1<256 / P::T>::value;
    using KG = KernelGeom<V, P, 1, G, TuneDefault>;
    static constexpr int M = P::N;
    static constexpr int SPLIT = (KG::PAD ? M + M / 8 : M) + 1;
    static constexpr int EXR = ((KG::LDS_ELEMS > SPLIT ? KG::LDS_ELEMS : SPLIT) + 1) / 2 * 2;
    static constexpr size_t LDS_BYTES = (size_t)EXR * G * sizeof(V) + KG::TW_BYTES;
    // the pairing twiddles W^k of a thread's E bins do not depend on the row: kept in registers where they are few
    static constexpr bool TWH_REG = P::E * (int)sizeof(V) / 4 <= 32;
};

// filter element times 1 / (2 m) (the halves of Xe, Xo are folded in), and its product with a bin
template <class V, bool HREAL> struct RconvFilter;
template <class V> struct RconvFilter<V, false> {
    using T = V;
    using RT = typename real_of<V>::type;
    static __device__ __forceinline__ V mul(V a, V h, RT sc) { return cmul(a, V{h.x * sc, h.y * sc}); }
};
template <class V> struct RconvFilter<V, true> {
    using RT = typename real_of<V>::type;
    using T = RT;
    static __device__ __forceinline__ V mul(V a, RT h, RT sc) {
        const RT s = h * sc;
        return V{a.x * s, a.y * s};
    }
};

// The row at `ip` (n reals, zeros beyond; nothing is read of a row that is not `valid`) as the M complex values of a thread group
template <class V, class P, bool VEC>
__device__ __forceinline__ void rrow_load(V (&v)[P::E], const typename real_of<V>::type* ip, bool valid, int n, int j) {
    using RT = typename real_of<V>::type;
    constexpr int E = P::E, T = P::T;
    if constexpr (VEC) {  // n even: a two-real value lies wholly inside the row or wholly in the padding
        const V* vp = reinterpret_cast<const V*>(ip);
#pragma unroll
        for (int k = 0; k < E; ++k) {
            const int kk = j + T * k;
            v[k] = (valid && 2 * kk < n) ? vp[kk] : V{0, 0};
        }
    } else {
#pragma unroll
        for (int k = 0; k < E; ++k) {
            const int kk = j + T * k;
            v[k] = V{(valid && 2 * kk < n) ? ip[2 * kk] : (RT)0, (valid && 2 * kk + 1 < n) ? ip[2 * kk + 1] : (RT)0};
        }
    }
}

// v: a row's (frame's) M complex values -> 2 X[k] of the thread's bins k = j + T * (0 ... E-1); returns 2 X[M] in the thread of bin 0.
// Ends behind a group barrier: every partner is read before the next transform's exchanges reuse the tile.  (The cross-spectrum
// kernels of dfft_xspec.hip and dfft_csd.hip.)
template <class V, class P, class RG>
__device__ __forceinline__ typename real_of<V>::type rrow_bins(V (&v)[P::E], const typename VecTraits<V>::W* twr, V* lds,
                                                                const typename VecTraits<V>::W (&wh)[RG::TWH_REG ? P::E : 1],
                                                                const typename VecTraits<V>::W* __restrict__ twh, int j) {
    using KG = typename RG::KG;
    using W = typename VecTraits<V>::W;
    using RT = typename real_of<V>::type;
    constexpr int  E = P::E, T = P::T, M = P::N;
    constexpr bool TWPOW = KG::TWMODE == TW_REG;
    run_stages<V, P, 0, +1, 1, KG::PAD, KG::WAVE_LOCAL, KG::TWMODE, TWPOW, 1, 1, KG::NW, KG::LOCALX>(v, twr, lds, j, 0);
    group_sync<KG::WAVE_LOCAL>();
#pragma unroll
    for (int k = 0; k < E; ++k) lds[lds_index<1, KG::PAD>(j + T * k, 0)] = v[k];
    group_sync<KG::WAVE_LOCAL>();
    RT nyq = (RT)0;
#pragma unroll
    for (int k = 0; k < E; ++k) {
        const int kk = j + T * k;
        const V   zm = lds[lds_index<1, KG::PAD>(kk == 0 ? 0 : M - kk, 0)];
        const W   w = RG::TWH_REG ? wh[RG::TWH_REG ? k : 0] : twh[kk];
        const V   xe{v[k].x + zm.x, v[k].y - zm.y};  // 2 Xe[k]
        const V   xo{v[k].y + zm.y, zm.x - v[k].x};  // 2 Xo[k]
        const V   t = cmul(xo, w);
        if (kk == 0) nyq = xe.x - xo.x;              // 2 X[M] = 2 (Re Z[0] - Im Z[0])
        v[k] = V{xe.x + t.x, xe.y + t.y};
    }
    group_sync<KG::WAVE_LOCAL>();
    return nyq;
}

}  // namespace dfft
