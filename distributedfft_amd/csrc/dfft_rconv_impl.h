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

}  // namespace dfft
