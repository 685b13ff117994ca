// dfft_conv.hip -- the X stage of the spectral-filter plans (dfft_plan_create_conv): y = ifft_x( fft_x(data) . H ) along the slow axis of the
// slab [x][row][z] that the forward YZ stage (P > 1: the forward exchange) leaves and the inverse YZ stage (the backward exchange) picks up.
//
// Fused form, xconv_cols_kernel (N0 = 64, 128, 256, 384, 512, 768, 1024): one launch, in place.  A thread group owns a tile of CB adjacent
// columns (CB * sizeof(V) = 128 bytes: 8 fp64 columns, or 8 PAIRS of fp32 columns), loads the N0 points of every column, issues the loads
// of the same tile of the filter copy behind them (the copy has the data's physical layout, so one offset serves both operands), runs the
// tuned forward stages of the C2C kernels (run_stages, dfft_fft_impl.h) -- which leave bin j + T k where point j + T k was loaded --,
// multiplies, runs the inverse as conj . forward . conj (one set of forward twiddles serves both halves; the form the Bluestein column
// kernel uses) and stores where it loaded.  Three volume-sized streams (data in, filter, data out; two and a half with a real filter)
// instead of the seven of forward X pass + multiply + inverse X pass, and no transpose in either direction.  1 / (N0 N1 N2) and the plan's
// scale are folded into the filter copy.
//
// Multi route (every other single-pass length, fp32 slabs that cannot be read as column pairs, DFFT_CONV_FUSED=0): the C2C column kernels
// in place along X (launch_fft), xconv_mul_kernel, the inverse column kernels -- same filter copy.
//
// Compiled once per instantiation group (-DDFFT_INST_GROUP=g: the fused kernels of the lengths of group g) and once with
// -DDFFT_INST_GROUP=DFFT_NUM_INST_GROUPS (the dispatcher, the multiply and the re-layout kernel).
#include "dfft_conv_impl.h"
#include "dfft_internal.h"

#include <atomic>

#ifndef DFFT_INST_GROUP
#error "compile with -DDFFT_INST_GROUP=<g>"
#endif

namespace dfft {

// entry point of length N: defined (and explicitly instantiated) in the translation unit of N's group only
template <bool ON, int N> struct XcInst {};
template <int N> struct XcInst<true, N> {
    static hipError_t run(const ConvLaunch& L, hipStream_t stream);
};

#if DFFT_INST_GROUP < DFFT_NUM_INST_GROUPS

// One launch per X stage.  Thread group g of a workgroup owns tile r0 + g = (row r, column block b): columns [b CB, b CB + CB) of row r
// in every plane x.  All strides in units of one V (fp32: pairs of columns).  in == out is the normal case: a tile reads all its points
// before its first exchange and writes them after the last one, and no two tiles share an element.
template <class V, class P, bool REAL, bool ROT>
__global__ void __attribute__((amdgpu_flat_work_group_size(1, XcGeom<V, P>::KG::THREADS)))
xconv_cols_kernel(const typename VecTraits<V>::G* in, typename VecTraits<V>::G* out, const typename XcFilter<V, REAL>::T* __restrict__ filt,
                  const typename VecTraits<V>::W* __restrict__ tw, unsigned plane, long long pitch, unsigned tiles, unsigned tiles_per_row,
                  int ncols, int rot, int mask, int forward_only, double scale) {
    using XG = XcGeom<V, P>;
    using KG = typename XG::KG;
    using VT = VecTraits<V>;
    using W = typename VT::W;
    using RT = typename real_of<W>::type;
    using F = XcFilter<V, REAL>;
    constexpr int  E = P::E, T = P::T, G = XG::G, GT = KG::GT, CB = XG::CB;
    constexpr bool TWPOW = KG::TWMODE == TW_REG;
    constexpr bool EARLY = conv_filter_early<V, P, REAL>();
    extern __shared__ __attribute__((aligned(16))) char dfft_smem[];
    const int g = threadIdx.x / GT;
    const int tid = (int)threadIdx.x - g * GT;
    const int c = tid % CB;
    const int j = tile_j<CB, KG::NW>(tid);
    V*        lds = reinterpret_cast<V*>(dfft_smem + KG::TW_BYTES) + g * KG::LDS_ELEMS;
    W         twreg[KG::TWMODE == TW_REG && KG::TWN > 0 ? KG::TWN : 1];
    const W*  twr = stage_twiddles<V, P, +1, KG>(twreg, reinterpret_cast<W*>(dfft_smem), tw, j);
    // rotated rows: point k of this thread lies in plane j + T k, whose rows are rotated by rot * (j + T k) mod the row length
    const int rot_j = ROT ? (rot * j) & mask : 0, rot_t = ROT ? (rot * T) & mask : 0;
    const RT  sc = (RT)scale;
    for (unsigned r0 = blockIdx.x * G; r0 < tiles; r0 += gridDim.x * G) {
        const unsigned t = r0 + g;
        bool           valid = t < tiles;
        const unsigned r = valid ? t / tiles_per_row : 0u;
        const int      col = (int)((valid ? t - r * tiles_per_row : 0u) * CB) + c;
        valid = valid && col < ncols;
        const long long base = (long long)r * pitch;
        unsigned        off[E];
#pragma unroll
        for (int k = 0; k < E; ++k) {
            const unsigned x = (unsigned)(j + T * k);
            off[k] = x * plane + (unsigned)(ROT ? ((col + rot_j + k * rot_t) & mask) : col);
        }
        V                    v[E];
        typename F::T        h[EARLY ? E : 1];
        if (valid) {
#pragma unroll
            for (int k = 0; k < E; ++k) v[k] = VT::from_g(in[base + off[k]]);
            if (EARLY && !forward_only) {  // behind the data loads, so that they fly under the forward stages
#pragma unroll
                for (int k = 0; k < E; ++k) h[EARLY ? k : 0] = filt[base + off[k]];
            }
        } else {
#pragma unroll
            for (int k = 0; k < E; ++k) {
                v[k] = VT::zero();
                h[EARLY ? k : 0] = typename F::T{};
            }
        }
        run_stages<V, P, 0, +1, CB, KG::PAD, KG::WAVE_LOCAL, KG::TWMODE, TWPOW, KG::PH, 1, KG::NW, KG::LOCALX>(v, twr, lds, j, c);
        if (forward_only) {  // (uniform over the launch) the filter copy of dfft_conv_set_kernel: the scaled spectrum, same layout
            if (valid) {
#pragma unroll
                for (int k = 0; k < E; ++k) out[base + off[k]] = VT::to_g(cscale(v[k], sc));
            }
            group_sync<KG::WAVE_LOCAL>();  // the next tile's exchanges reuse the tile
            continue;
        }
        // (A . H) conjugated: the inverse transform is conj(FFT(conj(A . H))); 1 / N is in H
#pragma unroll
        for (int k = 0; k < E; ++k) {
            if constexpr (EARLY) v[k] = cconj(F::mul(v[k], h[k]));
            else v[k] = valid ? cconj(F::mul(v[k], filt[base + off[k]])) : VT::zero();
        }
        group_sync<KG::WAVE_LOCAL>();  // the second transform's exchanges reuse the tile
        run_stages<V, P, 0, +1, CB, KG::PAD, KG::WAVE_LOCAL, KG::TWMODE, TWPOW, KG::PH, 1, KG::NW, KG::LOCALX>(v, twr, lds, j, c);
        if (valid) {
#pragma unroll
            for (int k = 0; k < E; ++k) out[base + off[k]] = VT::to_g(cconj(v[k]));
        }
        group_sync<KG::WAVE_LOCAL>();  // the next tile's exchanges reuse the tile
    }
}

template <class V, class P, bool REAL, bool ROT> hipError_t launch_xconv(const ConvLaunch& L, hipStream_t stream) {
    using XG = XcGeom<V, P>;
    using KG = typename XG::KG;
    using VT = VecTraits<V>;
    constexpr int           LANES = VT::LANES;
    static std::atomic<int> occ_cache[kMaxDevices];
    const ConvTiles<V, P>   t(L);
    if (!t.fits32(L)) return hipErrorInvalidValue;
    if (ROT != (L.rot > 0) || (ROT && ((t.ncols & (t.ncols - 1)) != 0 || L.rot % LANES != 0))) return hipErrorInvalidValue;
    (void)hipGetLastError();
    auto       kern = xconv_cols_kernel<V, P, REAL, ROT>;
    hipError_t e;
    const int  occ = resident_blocks_per_cu(reinterpret_cast<const void*>(kern), KG::THREADS, KG::LDS_BYTES, occ_cache, &e);
    if (occ == 0) return e;
    const long long grid = persistent_grid(device_info().cus, occ, (t.tiles + XG::G - 1) / XG::G);
    hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(KG::THREADS), KG::LDS_BYTES, stream, (const typename VT::G*)L.in, (typename VT::G*)L.out,
                       (const typename XcFilter<V, REAL>::T*)L.filt, (const typename VT::W*)L.tw, (unsigned)t.plane, t.pitch, (unsigned)t.tiles,
                       (unsigned)t.per_row, (int)t.ncols, L.rot / LANES, (int)t.ncols - 1, L.forward_only, L.scale);
    return hipGetLastError();
}

template <class V, class P> hipError_t launch_xconv_vp(const ConvLaunch& L, hipStream_t stream) {
    if (L.filter_real) return L.rot > 0 ? launch_xconv<V, P, true, true>(L, stream) : launch_xconv<V, P, true, false>(L, stream);
    return L.rot > 0 ? launch_xconv<V, P, false, true>(L, stream) : launch_xconv<V, P, false, false>(L, stream);
}

template <int N> hipError_t XcInst<true, N>::run(const ConvLaunch& L, hipStream_t stream) {
    if (L.dtype == F64) return launch_xconv_vp<double2, typename PlanFor<N>::type>(L, stream);
    if (L.dtype == F32) return launch_xconv_vp<cpair, typename PlanFor<N>::type>(L, stream);
    return hipErrorInvalidValue;
}
#define DFFT_XC_INST(N, GRP, E, ...) template struct XcInst<(GRP == DFFT_INST_GROUP && conv_fused_n(N)), N>;
DFFT_PLAN_TABLE(DFFT_XC_INST)
#undef DFFT_XC_INST

#else  // the dispatcher, the multiply of the multi route and the filter re-layout

namespace {

// data[i] *= filt[i]: D = 16 bytes of data (one fp64 element, two fp32 elements), H the filter elements that go with them
template <class D, class H> __device__ __forceinline__ D xc_mul16(D d, H h);
template <> __device__ __forceinline__ double2 xc_mul16(double2 d, double2 h) { return double2{d.x * h.x - d.y * h.y, d.x * h.y + d.y * h.x}; }
template <> __device__ __forceinline__ double2 xc_mul16(double2 d, double h) { return double2{d.x * h, d.y * h}; }
template <> __device__ __forceinline__ f32x4 xc_mul16(f32x4 d, f32x4 h) {
    return f32x4{d.x * h.x - d.y * h.y, d.x * h.y + d.y * h.x, d.z * h.z - d.w * h.w, d.z * h.w + d.w * h.z};
}
template <> __device__ __forceinline__ f32x4 xc_mul16(f32x4 d, f32x2 h) { return f32x4{d.x * h.x, d.y * h.x, d.z * h.y, d.w * h.y}; }

template <class D, class H>
__global__ void __launch_bounds__(256) xconv_mul_kernel(D* __restrict__ data, const H* __restrict__ filt, long long n16) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n16; i += (long long)gridDim.x * 256) data[i] = xc_mul16(data[i], filt[i]);
}
// the odd last element of an fp32 buffer
__global__ void xconv_mul_tail_kernel(float2* data, const float* filt, long long i, int real) {
    const float2 d = data[i];
    if (real) data[i] = float2{d.x * filt[i], d.y * filt[i]};
    else data[i] = float2{d.x * filt[2 * i] - d.y * filt[2 * i + 1], d.x * filt[2 * i + 1] + d.y * filt[2 * i]};
}

// dst[layout(kx, r, z)] = scale * h[(r * ncols + z) * n0 + kx], COMPS scalars per element (2: complex, 1: real); e runs over the source
template <class S, int COMPS>
__global__ void __launch_bounds__(256) xconv_relayout_kernel(const S* __restrict__ h, S* __restrict__ dst, long long n0, long long ncols,
                                                             long long plane, long long pitch, int rot, long long total, double scale) {
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
        const long long rz = e / n0, kx = e - rz * n0;
        const long long r = rz / ncols, z = rz - r * ncols;
        const long long zz = rot > 0 ? ((z + (long long)rot * kx) & (ncols - 1)) : z;
        const long long o = kx * plane + r * pitch + zz;
#pragma unroll
        for (int i = 0; i < COMPS; ++i) dst[o * COMPS + i] = (S)((double)h[e * COMPS + i] * scale);
    }
}

template <int N> hipError_t xc_run(const ConvLaunch& L, hipStream_t stream) {
    if constexpr (conv_fused_n(N)) return XcInst<true, N>::run(L, stream);
    else return hipErrorInvalidValue;
}

}  // namespace

bool conv_fused_length(int n0) { return conv_fused_n(n0); }

bool conv_fused_applies(const ConvLaunch& L) {
    if (!conv_fused_n(L.n0) || L.rows < 1 || L.ncols < 1) return false;
    if (L.rot > 0 && (L.ncols & (L.ncols - 1)) != 0) return false;
    if (L.dtype == F32 && ((L.ncols | L.plane | L.pitch | (long long)L.rot) & 1)) return false;  // fp32 runs on column pairs
    // ... with 16-byte accesses on both sides: a caller's buffer that is only 8-byte aligned (the P = 1 natural layout stores into `out`)
    // takes the multi route, whose column launches fall back per base (make_pair_launch)
    if (L.dtype == F32 && (((uintptr_t)L.in | (uintptr_t)L.out) & 15)) return false;
    const long long lanes = L.dtype == F32 ? 2 : 1;
    return (long long)L.n0 * (L.plane / lanes) + L.pitch / lanes < (1ll << 32) && L.rows * ((L.ncols / lanes + 7) / 8) < (1ll << 31);
}

hipError_t launch_conv_fused(const ConvLaunch& L, hipStream_t stream) {
    if (!conv_fused_applies(L)) return hipErrorInvalidValue;
    switch (L.n0) {
#define DFFT_XC_CASE(N, GRP, E, ...) \
    case N: return xc_run<N>(L, stream);
        DFFT_PLAN_TABLE(DFFT_XC_CASE)
#undef DFFT_XC_CASE
        default: return hipErrorInvalidValue;
    }
}

hipError_t launch_conv_mul(int dtype, int filter_real, void* data, const void* filt, long long count, hipStream_t stream) {
    if (count <= 0) return hipSuccess;
    (void)hipGetLastError();
    if (dtype == F64) {
        if (filter_real) hipLaunchKernelGGL((xconv_mul_kernel<double2, double>), dim3(xc_grid(count)), dim3(256), 0, stream, (double2*)data, (const double*)filt, count);
        else hipLaunchKernelGGL((xconv_mul_kernel<double2, double2>), dim3(xc_grid(count)), dim3(256), 0, stream, (double2*)data, (const double2*)filt, count);
        return hipGetLastError();
    }
    if (dtype != F32) return hipErrorInvalidValue;
    const long long n16 = count / 2;
    if (n16 > 0) {
        if (filter_real) hipLaunchKernelGGL((xconv_mul_kernel<f32x4, f32x2>), dim3(xc_grid(n16)), dim3(256), 0, stream, (f32x4*)data, (const f32x2*)filt, n16);
        else hipLaunchKernelGGL((xconv_mul_kernel<f32x4, f32x4>), dim3(xc_grid(n16)), dim3(256), 0, stream, (f32x4*)data, (const f32x4*)filt, n16);
    }
    if (count & 1) hipLaunchKernelGGL(xconv_mul_tail_kernel, dim3(1), dim3(1), 0, stream, (float2*)data, (const float*)filt, count - 1, filter_real);
    return hipGetLastError();
}

hipError_t launch_conv_relayout(const ConvLaunch& L, const void* h, void* dst, hipStream_t stream) {
    const long long total = L.rows * L.ncols * (long long)L.n0;
    if (total <= 0) return hipSuccess;
    if (L.rot > 0 && (L.ncols & (L.ncols - 1)) != 0) return hipErrorInvalidValue;
    (void)hipGetLastError();
    const dim3 grid(xc_grid(total)), block(256);
    if (L.dtype == F64 && L.filter_real)
        hipLaunchKernelGGL((xconv_relayout_kernel<double, 1>), grid, block, 0, stream, (const double*)h, (double*)dst, (long long)L.n0, L.ncols, L.plane, L.pitch, L.rot, total, L.scale);
    else if (L.dtype == F64)
        hipLaunchKernelGGL((xconv_relayout_kernel<double, 2>), grid, block, 0, stream, (const double*)h, (double*)dst, (long long)L.n0, L.ncols, L.plane, L.pitch, L.rot, total, L.scale);
    else if (L.dtype == F32 && L.filter_real)
        hipLaunchKernelGGL((xconv_relayout_kernel<float, 1>), grid, block, 0, stream, (const float*)h, (float*)dst, (long long)L.n0, L.ncols, L.plane, L.pitch, L.rot, total, L.scale);
    else if (L.dtype == F32)
        hipLaunchKernelGGL((xconv_relayout_kernel<float, 2>), grid, block, 0, stream, (const float*)h, (float*)dst, (long long)L.n0, L.ncols, L.plane, L.pitch, L.rot, total, L.scale);
    else
        return hipErrorInvalidValue;
    return hipGetLastError();
}

#endif

}  // namespace dfft
