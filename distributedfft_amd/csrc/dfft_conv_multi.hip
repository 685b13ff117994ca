// dfft_conv_multi.hip -- the X stage of the multi-output real-field spectral-filter plans (dfft_plan_create_conv_real_multi):
//     y_k = ifft_x( fft_x(data) . H . a_k[x] . b_k[row] . c_k[col] ),   k = 0 .. K-1,
// on the half-spectrum slab [x][row][col] the forward YZ stage (P > 1: the forward exchange) leaves, into K slabs of the same layout.
//
// Fused form, xconv_multi_cols_kernel (N0 = 64, 128, 256, 384, 512, 768, 1024; the tile geometry of xconv_cols_kernel, dfft_conv.hip):
// a thread group owns a tile of CB adjacent 16-byte columns, loads the N0 points of every column, runs the forward stages ONCE and
// multiplies ONCE by the filter copy: B.  Per output k it forms conj(B . a_k[x] . s_k) -- s_k = b_k[row] . c_k[col] is one value per thread,
// tile and output (fp32: one per column of the pair) --, runs the inverse as conj . forward . conj on the same twiddles and stores to
// slab k at the offsets the tile was loaded from.  The K . N0 elements of a stay hot in cache (they cannot go to LDS: the 1024-point tile
// fills it).  Outputs are produced in the order 1 .. K-1, 0: slab 0 may be the input slab, and a tile reads everything before it writes.
//
// Where B lives.  Next to the E working points it doubles the live data.  Workgroups of at most 256 threads (one wave per SIMD, 512
// registers) and the short plans of 512-thread workgroups keep B in registers.  The 16-point plans of 512-thread workgroups (1024 points:
// 64 + 64 registers of data under a budget of 256, next to the butterflies' temporaries) cannot -- so they PARK B in slab 0: the tile
// owns those elements, every thread re-reads exactly what it wrote itself (program order, no fence), the lines are in L2 from the store,
// and output 0 is produced last, over them.  No instantiation uses scratch (profiles/r14/kernel_resources.txt).
//
// Multi route (every other single-pass length, DFFT_CONV_FUSED=0): forward column kernels in place, launch_conv_mul by the filter copy
// in place (dfft_conv.hip), then per output xconv_factor_mul_kernel out of place into slab k and the inverse column kernels there;
// output 0 last, in place (dfft_plan.cpp, conv_multi_x_stage).
//
// Compiled once per instantiation group (-DDFFT_INST_GROUP=g: the fused kernels of the lengths of group g) and once with
// -DDFFT_INST_GROUP=DFFT_NUM_INST_GROUPS (the dispatcher and the factor multiply).
#include "dfft_conv_impl.h"
#include "dfft_conv_multi.h"
#include "dfft_internal.h"

#include <atomic>

#ifndef DFFT_INST_GROUP
#error "compile with -DDFFT_INST_GROUP=<g>"
#endif

namespace dfft {

// entry point of length N: defined (and explicitly instantiated) in the translation unit of N's group only
template <bool ON, int N> struct XmInst {};
template <int N> struct XmInst<true, N> {
    static hipError_t run(const ConvLaunch& L, const ConvMultiArgs& M, int K, hipStream_t stream);
};

#if DFFT_INST_GROUP < DFFT_NUM_INST_GROUPS

// B is parked in slab 0 instead of registers: 64 registers of points per thread in workgroups of more than 256 threads
template <class V, class P> constexpr bool xm_park() { return P::E * (int)sizeof(V) / 4 >= 64 && XcGeom<V, P>::KG::THREADS > 256; }

// One launch per X stage.  Thread group g of a workgroup owns tile r0 + g = (row r, column block b): columns [b CB, b CB + CB) of row r in
// every plane x.  All strides in units of one V (fp32: pairs of columns).
template <class V, class P, bool REAL>
__global__ void __attribute__((amdgpu_flat_work_group_size(1, XcGeom<V, P>::KG::THREADS)))
xconv_multi_cols_kernel(const typename VecTraits<V>::G* in, const typename XcFilter<V, REAL>::T* __restrict__ filt,
                        const typename VecTraits<V>::W* __restrict__ tw, ConvMultiArgs M, int K, unsigned plane, long long pitch, unsigned tiles,
                        unsigned tiles_per_row, int ncols) {
    using XG = XcGeom<V, P>;
    using KG = typename XG::KG;
    using VT = VecTraits<V>;
    using GV = typename VT::G;
    using W = typename VT::W;
    using F = XcFilter<V, REAL>;
    constexpr int  E = P::E, T = P::T, G = XG::G, GT = KG::GT, CB = XG::CB;
    constexpr bool TWPOW = KG::TWMODE == TW_REG;
    constexpr bool PARK = xm_park<V, P>();
    constexpr bool EARLY = conv_filter_early<V, P, REAL>();
    extern __shared__ __attribute__((aligned(16))) char dfft_smem[];
    const int g = threadIdx.x / GT;
    const int tid = (int)threadIdx.x - g * GT;
    const int c = tid % CB;
    const int j = tile_j<CB, KG::NW>(tid);
    V*        lds = reinterpret_cast<V*>(dfft_smem + KG::TW_BYTES) + g * KG::LDS_ELEMS;
    W         twreg[KG::TWMODE == TW_REG && KG::TWN > 0 ? KG::TWN : 1];
    const W*  twr = stage_twiddles<V, P, +1, KG>(twreg, reinterpret_cast<W*>(dfft_smem), tw, j);
    GV* const out0 = (GV*)M.out[0];
    for (unsigned r0 = blockIdx.x * G; r0 < tiles; r0 += gridDim.x * G) {
        const unsigned t = r0 + g;
        bool           valid = t < tiles;
        const unsigned r = valid ? t / tiles_per_row : 0u;
        const int      col = (int)((valid ? t - r * tiles_per_row : 0u) * CB) + c;
        valid = valid && col < ncols;
        const long long base = (long long)r * pitch;
        // (parked kernels: the plane offsets are formed per tile -- as loop invariants the E of them, next to the tile's LDS addresses,
        // are what did not fit the registers)
        unsigned pl = plane;
        if constexpr (PARK) asm volatile("" : "+s"(pl));
        unsigned off[E];
#pragma unroll
        for (int k = 0; k < E; ++k) off[k] = (unsigned)(j + T * k) * pl + (unsigned)col;
        V             v[E];
        typename F::T h[EARLY ? E : 1];
        if (valid) {
#pragma unroll
            for (int k = 0; k < E; ++k) v[k] = VT::from_g(in[base + off[k]]);
            if constexpr (EARLY) {
#pragma unroll
                for (int k = 0; k < E; ++k) h[k] = filt[base + off[k]];
            }
        } else {
#pragma unroll
            for (int k = 0; k < E; ++k) {
                v[k] = VT::zero();
                h[EARLY ? k : 0] = typename F::T{};
            }
        }
        run_stages<V, P, 0, +1, CB, KG::PAD, KG::WAVE_LOCAL, KG::TWMODE, TWPOW, KG::PH, 1, KG::NW, KG::LOCALX>(v, twr, lds, j, c);
        // B = A . H (1 / N is in H); a parked B goes to slab 0, where this thread alone reads and writes these elements
        V B[PARK ? 1 : E];
#pragma unroll
        for (int k = 0; k < E; ++k) {
            if constexpr (EARLY) v[k] = F::mul(v[k], h[k]);
            else v[k] = valid ? F::mul(v[k], filt[base + off[k]]) : VT::zero();
            if constexpr (!PARK) B[k] = v[k];
            // the late filter reads four at a time: all E in flight next to the E points do not fit the registers
            if constexpr (!EARLY) {
                if (k % 4 == 3) __builtin_amdgcn_sched_barrier(0);
            }
        }
        if constexpr (PARK) {
            if (valid && K > 1) {
#pragma unroll
                for (int k = 0; k < E; ++k) out0[base + off[k]] = VT::to_g(v[k]);
            }
        }
        for (int oi = 0; oi < K; ++oi) {
            const int o = oi + 1 < K ? oi + 1 : 0;  // 1 .. K-1, then 0
            // s = b[row] . c[col]: one value per thread, tile and output (fp32: per column of the pair)
            V s = VT::zero();
            if (valid) s = cmul(VT::from_g(((const GV*)M.cz[o])[col]), ((const W*)M.by[o])[r]);
            const W* __restrict__ a = (const W*)M.ax[o];
            if constexpr (PARK) {
                if (oi > 0) {
#pragma unroll
                    for (int k = 0; k < E; ++k) v[k] = valid ? VT::from_g(out0[base + off[k]]) : VT::zero();
                }
            }
            // (B . a[x] . s) conjugated: the inverse transform is conj(FFT(conj(.)))
#pragma unroll
            for (int k = 0; k < E; ++k) {
                const V b = PARK ? v[k] : B[PARK ? 0 : k];
                v[k] = cconj(cmul(b, cmul(s, a[j + T * k])));
                if constexpr (PARK) {  // the factor reads four at a time, like the late filter reads
                    if (k % 4 == 3) __builtin_amdgcn_sched_barrier(0);
                }
            }
            group_sync<KG::WAVE_LOCAL>();  // this transform's exchanges reuse the tile
            run_stages<V, P, 0, +1, CB, KG::PAD, KG::WAVE_LOCAL, KG::TWMODE, TWPOW, KG::PH, 1, KG::NW, KG::LOCALX>(v, twr, lds, j, c);
            if (valid) {
                GV* const dst = (GV*)M.out[o];
#pragma unroll
                for (int k = 0; k < E; ++k) dst[base + off[k]] = VT::to_g(cconj(v[k]));
            }
        }
        group_sync<KG::WAVE_LOCAL>();  // the next tile's exchanges reuse the tile
    }
}

template <class V, class P, bool REAL> hipError_t launch_xmulti(const ConvLaunch& L, const ConvMultiArgs& M, int K, hipStream_t stream) {
    using XG = XcGeom<V, P>;
    using KG = typename XG::KG;
    using VT = VecTraits<V>;
    static std::atomic<int> occ_cache[kMaxDevices];
    const ConvTiles<V, P>   t(L);
    if (!t.fits32(L)) return hipErrorInvalidValue;
    (void)hipGetLastError();
    auto       kern = xconv_multi_cols_kernel<V, P, REAL>;
    hipError_t e;
    const int  occ = resident_blocks_per_cu(reinterpret_cast<const void*>(kern), KG::THREADS, KG::LDS_BYTES, occ_cache, &e);
    if (occ == 0) return e;
    const long long grid = persistent_grid(device_info().cus, occ, (t.tiles + XG::G - 1) / XG::G);
    hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(KG::THREADS), KG::LDS_BYTES, stream, (const typename VT::G*)L.in,
                       (const typename XcFilter<V, REAL>::T*)L.filt, (const typename VT::W*)L.tw, M, K, (unsigned)t.plane, t.pitch, (unsigned)t.tiles,
                       (unsigned)t.per_row, (int)t.ncols);
    return hipGetLastError();
}

template <int N> hipError_t XmInst<true, N>::run(const ConvLaunch& L, const ConvMultiArgs& M, int K, hipStream_t stream) {
    using P = typename PlanFor<N>::type;
    if (L.dtype == F64) return L.filter_real ? launch_xmulti<double2, P, true>(L, M, K, stream) : launch_xmulti<double2, P, false>(L, M, K, stream);
    if (L.dtype == F32) return L.filter_real ? launch_xmulti<cpair, P, true>(L, M, K, stream) : launch_xmulti<cpair, P, false>(L, M, K, stream);
    return hipErrorInvalidValue;
}
#define DFFT_XM_INST(N, GRP, E, ...) template struct XmInst<(GRP == DFFT_INST_GROUP && conv_fused_n(N)), N>;
DFFT_PLAN_TABLE(DFFT_XM_INST)
#undef DFFT_XM_INST

#else  // the dispatcher and the factor multiply of the multi route

namespace {

// 16 bytes of the slab times the factor f0 (fp32: f0 / f1 for the two elements)
template <class D, class W> __device__ __forceinline__ D xm_mul16(D d, W f0, W f1);
template <> __device__ __forceinline__ double2 xm_mul16(double2 d, double2 f, double2) { return double2{d.x * f.x - d.y * f.y, d.x * f.y + d.y * f.x}; }
template <> __device__ __forceinline__ f32x4 xm_mul16(f32x4 d, float2 f0, float2 f1) {
    return f32x4{d.x * f0.x - d.y * f0.y, d.x * f0.y + d.y * f0.x, d.z * f1.x - d.w * f1.y, d.z * f1.y + d.w * f1.x};
}

// dst[i] = src[i] . a[x] . b[row] . c[col], i over the n16 16-byte units of the slab; LANES elements per unit (plane, pitch and ncols
// are multiples of LANES, so a unit never straddles a row); columns >= ncols receive zeros
template <class D, class W, int LANES>
__global__ void __launch_bounds__(256) xconv_factor_mul_kernel(const D* src, D* dst, const W* __restrict__ a, const W* __restrict__ b,
                                                               const W* __restrict__ cz, long long plane, long long pitch, long long ncols,
                                                               long long n16) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n16; i += (long long)gridDim.x * 256) {
        const long long e = i * LANES, x = e / plane, rem = e - x * plane, r = rem / pitch, z = rem - r * pitch;
        if (z >= ncols) {
            dst[i] = D{};
            continue;
        }
        const W ab = cmul(a[x], b[r]);
        dst[i] = xm_mul16<D, W>(src[i], cmul(ab, cz[z]), cmul(ab, cz[z + LANES - 1]));
    }
}

template <int N> hipError_t xm_run(const ConvLaunch& L, const ConvMultiArgs& M, int K, hipStream_t stream) {
    if constexpr (conv_fused_n(N)) return XmInst<true, N>::run(L, M, K, stream);
    else return hipErrorInvalidValue;
}

}  // namespace

hipError_t launch_conv_multi_fused(const ConvLaunch& L, const ConvMultiArgs& M, int K, hipStream_t stream) {
    if (!conv_fused_applies(L) || L.rot != 0 || K < 1 || K > CONV_MAX_OUTPUTS) return hipErrorInvalidValue;
    for (int k = 0; k < K; ++k)
        if (!M.out[k] || !M.ax[k] || !M.by[k] || !M.cz[k]) return hipErrorInvalidValue;
    // fp32 stores column pairs: every slab on a 16-byte boundary, like L.in (conv_fused_applies).  The slabs are the plan's own
    // allocations today; a caller's 8-byte-aligned buffer here must fail loudly instead of taking 16-byte stores
    if (L.dtype == F32)
        for (int k = 0; k < K; ++k)
            if ((uintptr_t)M.out[k] & 15) return hipErrorInvalidValue;
    switch (L.n0) {
#define DFFT_XM_CASE(N, GRP, E, ...) \
    case N: return xm_run<N>(L, M, K, stream);
        DFFT_PLAN_TABLE(DFFT_XM_CASE)
#undef DFFT_XM_CASE
        default: return hipErrorInvalidValue;
    }
}

hipError_t launch_conv_factor_mul(const ConvLaunch& L, const void* src, void* dst, const void* ax, const void* by, const void* cz,
                                  hipStream_t stream) {
    const long long total = (long long)L.n0 * L.plane;
    if (total <= 0) return hipSuccess;
    if (!src || !dst || !ax || !by || !cz || L.rot != 0 || L.ncols > L.pitch || L.plane != L.rows * L.pitch) return hipErrorInvalidValue;
    (void)hipGetLastError();
    if (L.dtype == F64) {
        hipLaunchKernelGGL((xconv_factor_mul_kernel<double2, double2, 1>), dim3(xc_grid(total)), dim3(256), 0, stream, (const double2*)src, (double2*)dst,
                           (const double2*)ax, (const double2*)by, (const double2*)cz, L.plane, L.pitch, L.ncols, total);
        return hipGetLastError();
    }
    if (L.dtype != F32 || ((L.ncols | L.pitch) & 1)) return hipErrorInvalidValue;  // pairs of elements: even rows
    const long long n16 = total / 2;
    hipLaunchKernelGGL((xconv_factor_mul_kernel<f32x4, float2, 2>), dim3(xc_grid(n16)), dim3(256), 0, stream, (const f32x4*)src, (f32x4*)dst,
                       (const float2*)ax, (const float2*)by, (const float2*)cz, L.plane, L.pitch, L.ncols, n16);
    return hipGetLastError();
}

#endif

}  // namespace dfft
