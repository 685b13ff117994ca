// dfft_real.hip -- the Z stage of the real-to-complex / complex-to-real slab plans (dfft_plan_create_r2c): rows of n2 reals <-> rows of
// n2/2 + 1 Hermitian bins.
//
// A real row x[0 .. n2) is read as the n2/2 = M complex values z[n] = x[2n] + i x[2n+1] (the same bytes) and transformed with the M-point
// FFT of the library (run_stages of dfft_fft_impl.h on the tuned plan of dfft_plans.h -- the arithmetic and register twiddles of the C2C
// row kernel).  The split step then pairs bin k with bin M - k through one LDS exchange:
//     Xe[k] = (Z[k] + conj Z[M-k]) / 2,   Xo[k] = -i (Z[k] - conj Z[M-k]) / 2,   X[k] = Xe[k] + W^k Xo[k]   (k = 0 .. M, Z[M] = Z[0])
// with W = e^{-2 pi i / n2} from the plan's n2-entry table (rounded once from extended precision, get_twiddles).  The inverse merges
//     Z[k] = (X[k] + conj X[M-k]) + i (X[k] - conj X[M-k]) conj(W^k)
// with the imaginary parts of X[0] and X[M] taken as zero, runs the inverse M-point FFT and stores Re / Im as the even / odd reals --
// n2 * numpy.fft.irfft of the row for any input (the rule numpy applies to the DC and Nyquist bins).
//
// Kernels (stable names for rocprofv3): r2c_rows_kernel / c2r_rows_kernel (one launch, tuned half-lengths); half-lengths served by the
// run-time-scheduled kernel (dfft_generic.hip) run that row kernel on the complex view plus r2c_split_kernel / c2r_merge_kernel.
//
// Compiled once per instantiation group (-DDFFT_INST_GROUP=g, the group column of DFFT_PLAN_TABLE) and once with
// -DDFFT_INST_GROUP=DFFT_NUM_INST_GROUPS for the dispatcher and the split / merge kernels.
#include "dfft_fft_impl.h"
#include "dfft_internal.h"
#include "dfft_plans.h"
#include "dfft_real.h"

#include <algorithm>
#include <cstring>

#ifndef DFFT_INST_GROUP
#error "compile with -DDFFT_INST_GROUP=<g>"
#endif

namespace dfft {

// Geometry: the C2C row kernel's (one FFT of M points per thread group, about 256 threads per workgroup, twiddles where KernelGeom puts
// them); the LDS tile of a group also holds the M + 1 bins of the split / merge step in natural order.
template <class V, class P> struct RealGeom {
    static constexpr int G = ConstMax1<256 / P::T>::value;
    using KG = KernelGeom<V, P, 1, G, TuneDefault>;
    static constexpr int M = P::N;
    static constexpr int SPLIT = (KG::PAD ? M + M / 8 : M) + 1;
    static constexpr int EXR = ((KG::LDS_ELEMS > SPLIT ? KG::LDS_ELEMS : SPLIT) + 1) / 2 * 2;
    static constexpr size_t LDS_BYTES = (size_t)EXR * G * sizeof(V) + KG::TW_BYTES;
    // the split twiddles W^k of a thread's E bins do not depend on the row: kept in registers where they are few
    static constexpr bool TWH_REG = P::E * (int)sizeof(V) / 4 <= 32;
};

template <class V, class P>
__global__ void __attribute__((amdgpu_flat_work_group_size(1, RealGeom<V, P>::KG::THREADS)))
r2c_rows_kernel(const V* __restrict__ in, V* __restrict__ out, const typename VecTraits<V>::W* __restrict__ tw,
                const typename VecTraits<V>::W* __restrict__ twh, unsigned rows, unsigned rows_per_plane, long long ipitch, long long iplane,
                long long opitch, long long oplane, double scale) {
    using RG = RealGeom<V, P>;
    using KG = typename RG::KG;
    using W = typename VecTraits<V>::W;
    using RT = typename real_of<W>::type;
    constexpr int E = P::E, T = P::T, M = P::N, G = RG::G, GT = KG::GT;
    constexpr bool TWPOW = KG::TWMODE == TW_REG;
    extern __shared__ __attribute__((aligned(16))) char dfft_smem[];
    const int g = threadIdx.x / GT;
    const int j = tile_j<1, KG::NW>((int)threadIdx.x - g * GT);
    V*        lds = reinterpret_cast<V*>(dfft_smem + KG::TW_BYTES) + g * RG::EXR;
    W         twreg[KG::TWMODE == TW_REG && KG::TWN > 0 ? KG::TWN : 1];
    const W*  twr = stage_twiddles<V, P, +1, KG>(twreg, reinterpret_cast<W*>(dfft_smem), tw, j);
    W         wh[RG::TWH_REG ? E : 1];
    if constexpr (RG::TWH_REG) {
#pragma unroll
        for (int k = 0; k < E; ++k) wh[k] = twh[j + T * k];
    }
    const RT sc = (RT)scale, half = (RT)0.5;
    for (unsigned r0 = blockIdx.x * G; r0 < rows; r0 += gridDim.x * G) {
        const unsigned row = r0 + g;
        const bool     valid = row < rows;
        const unsigned a = valid ? row / rows_per_plane : 0u, b = valid ? row - a * rows_per_plane : 0u;
        const V*       ip = in + (long long)a * iplane + (long long)b * ipitch;
        V              v[E];
#pragma unroll
        for (int k = 0; k < E; ++k) v[k] = valid ? ip[j + T * k] : V{0, 0};
        run_stages<V, P, 0, +1, 1, KG::PAD, KG::WAVE_LOCAL, KG::TWMODE, TWPOW, 1, 1, KG::NW, KG::LOCALX>(v, twr, lds, j, 0);
        group_sync<KG::WAVE_LOCAL>();
#pragma unroll
        for (int k = 0; k < E; ++k) lds[lds_index<1, KG::PAD>(j + T * k, 0)] = v[k];
        group_sync<KG::WAVE_LOCAL>();
        if (valid) {
            V* op = out + (long long)a * oplane + (long long)b * opitch;
#pragma unroll
            for (int k = 0; k < E; ++k) {
                const int kk = j + T * k;
                const V   zm = lds[lds_index<1, KG::PAD>(kk == 0 ? 0 : M - kk, 0)];
                const V   xe{(v[k].x + zm.x) * half, (v[k].y - zm.y) * half};
                const V   xo{(v[k].y + zm.y) * half, (zm.x - v[k].x) * half};
                const W   w = RG::TWH_REG ? wh[RG::TWH_REG ? k : 0] : twh[kk];
                op[kk] = cscale(cadd(xe, cmul(xo, w)), sc);
            }
            if (j == 0) op[M] = V{(v[0].x - v[0].y) * sc, (RT)0};
        }
        group_sync<KG::WAVE_LOCAL>();  // the next row's exchanges reuse the tile
    }
}

template <class V, class P>
__global__ void __attribute__((amdgpu_flat_work_group_size(1, RealGeom<V, P>::KG::THREADS)))
c2r_rows_kernel(const V* __restrict__ in, V* __restrict__ out, const typename VecTraits<V>::W* __restrict__ tw,
                const typename VecTraits<V>::W* __restrict__ twh, unsigned rows, unsigned rows_per_plane, long long ipitch, long long iplane,
                long long opitch, long long oplane, double scale) {
    using RG = RealGeom<V, P>;
    using KG = typename RG::KG;
    using W = typename VecTraits<V>::W;
    using RT = typename real_of<W>::type;
    constexpr int E = P::E, T = P::T, M = P::N, G = RG::G, GT = KG::GT;
    constexpr bool TWPOW = KG::TWMODE == TW_REG;
    extern __shared__ __attribute__((aligned(16))) char dfft_smem[];
    const int g = threadIdx.x / GT;
    const int j = tile_j<1, KG::NW>((int)threadIdx.x - g * GT);
    V*        lds = reinterpret_cast<V*>(dfft_smem + KG::TW_BYTES) + g * RG::EXR;
    W         twreg[KG::TWMODE == TW_REG && KG::TWN > 0 ? KG::TWN : 1];
    const W*  twr = stage_twiddles<V, P, -1, KG>(twreg, reinterpret_cast<W*>(dfft_smem), tw, j);
    W         wh[RG::TWH_REG ? E : 1];
    if constexpr (RG::TWH_REG) {
#pragma unroll
        for (int k = 0; k < E; ++k) wh[k] = twh[j + T * k];
    }
    const RT sc = (RT)scale;
    for (unsigned r0 = blockIdx.x * G; r0 < rows; r0 += gridDim.x * G) {
        const unsigned row = r0 + g;
        const bool     valid = row < rows;
        const unsigned a = valid ? row / rows_per_plane : 0u, b = valid ? row - a * rows_per_plane : 0u;
        const V*       ip = in + (long long)a * iplane + (long long)b * ipitch;
        V              v[E];
#pragma unroll
        for (int k = 0; k < E; ++k) v[k] = valid ? ip[j + T * k] : V{0, 0};
        V xm = (valid && j == 0) ? ip[M] : V{0, 0};
        if (j == 0) {  // the imaginary parts of the DC and Nyquist bins are ignored
            v[0].y = (RT)0;
            xm.y = (RT)0;
        }
        group_sync<KG::WAVE_LOCAL>();  // the previous row's exchanges are done with the tile
#pragma unroll
        for (int k = 0; k < E; ++k) lds[lds_index<1, KG::PAD>(j + T * k, 0)] = v[k];
        if (j == 0) lds[lds_index<1, KG::PAD>(M, 0)] = xm;
        group_sync<KG::WAVE_LOCAL>();
#pragma unroll
        for (int k = 0; k < E; ++k) {
            const int kk = j + T * k;
            const V   xp = lds[lds_index<1, KG::PAD>(M - kk, 0)];
            const W   w = RG::TWH_REG ? wh[RG::TWH_REG ? k : 0] : twh[kk];
            const V   xe{v[k].x + xp.x, v[k].y - xp.y};
            const V   d{v[k].x - xp.x, v[k].y + xp.y};
            const V   xo{d.x * w.x + d.y * w.y, d.y * w.x - d.x * w.y};  // d * conj(w)
            v[k] = V{xe.x - xo.y, xe.y + xo.x};                          // xe + i xo
        }
        group_sync<KG::WAVE_LOCAL>();  // the exchanges below overwrite the bins
        run_stages<V, P, 0, -1, 1, KG::PAD, KG::WAVE_LOCAL, KG::TWMODE, TWPOW, 1, 1, KG::NW, KG::LOCALX>(v, twr, lds, j, 0);
        if (valid) {
            V* op = out + (long long)a * oplane + (long long)b * opitch;
#pragma unroll
            for (int k = 0; k < E; ++k) op[j + T * k] = cscale(v[k], sc);
        }
    }
}

template <class V, class P> hipError_t launch_real_plan(const RealLaunch& L, const void* tw, const void* twh, hipStream_t stream) {
    using RG = RealGeom<V, P>;
    using W = typename VecTraits<V>::W;
    auto kern = L.dir > 0 ? r2c_rows_kernel<V, P> : c2r_rows_kernel<V, P>;
    static std::atomic<int> blocks_per_cu[2][kMaxDevices];  // per kernel: R2C, C2R
    hipError_t              e;
    const int               bpc = resident_blocks_per_cu(reinterpret_cast<const void*>(kern), RG::KG::THREADS, RG::LDS_BYTES, blocks_per_cu[L.dir > 0 ? 0 : 1], &e);
    if (bpc == 0) return e;
    const bool      fwd = L.dir > 0;
    // in units of V: the real side's strides count reals, two per complex value
    const long long ip = fwd ? L.rpitch / 2 : L.cpitch, ipl = fwd ? L.rplane / 2 : L.cplane;
    const long long op = fwd ? L.cpitch : L.rpitch / 2, opl = fwd ? L.cplane : L.rplane / 2;
    const long long grid = persistent_grid(device_info().cus, bpc, (L.rows + RG::G - 1) / RG::G);
    if (grid < 1) return hipSuccess;
    (void)hipGetLastError();
    hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(RG::KG::THREADS), RG::LDS_BYTES, stream, (const V*)L.in, (V*)L.out, (const W*)tw,
                       (const W*)twh, (unsigned)L.rows, (unsigned)L.rows_per_plane, ip, ipl, op, opl, L.scale == 0.0 ? 1.0 : L.scale);
    return hipGetLastError();
}

// entry point of length N: defined (and explicitly instantiated) in the translation unit of N's group only
template <bool ON, int N> struct RealInst {};
template <int N> struct RealInst<true, N> {
    static hipError_t run(const RealLaunch& L, const void* tw, const void* twh, hipStream_t stream);
};

#if DFFT_INST_GROUP < DFFT_NUM_INST_GROUPS

template <int N> hipError_t RealInst<true, N>::run(const RealLaunch& L, const void* tw, const void* twh, hipStream_t stream) {
    if (L.dtype == F64) return launch_real_plan<double2, typename PlanFor<N>::type>(L, tw, twh, stream);
    if (L.dtype == F32) return launch_real_plan<float2, typename PlanFor<N>::type>(L, tw, twh, stream);
    return hipErrorInvalidValue;
}
#define DFFT_REAL_INST(N, GRP, E, ...) template struct RealInst<(GRP == DFFT_INST_GROUP), N>;
DFFT_PLAN_TABLE(DFFT_REAL_INST)
#undef DFFT_REAL_INST

#else  // the dispatcher, and the split / merge kernels of the two-launch form

// R2C split after the row kernel of the M-point view (in place on the complex rows): thread t of a row handles the pair (t, M - t)
template <class V>
__global__ void __launch_bounds__(256) r2c_split_kernel(V* __restrict__ buf, const typename VecTraits<V>::W* __restrict__ twh, int m,
                                                        long long rows, long long rows_per_plane, long long pitch, long long plane, double scale) {
    using W = typename VecTraits<V>::W;
    using RT = typename real_of<W>::type;
    const int       pairs = m / 2 + 1;
    const long long total = rows * pairs;
    const RT        sc = (RT)scale, half = (RT)0.5;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const long long row = i / pairs;
        const int       k = (int)(i - row * pairs);
        const long long a = row / rows_per_plane, b = row - a * rows_per_plane;
        V*              z = buf + a * plane + b * pitch;
        if (k == 0) {
            const V z0 = z[0];
            z[0] = V{(z0.x + z0.y) * sc, (RT)0};
            z[m] = V{(z0.x - z0.y) * sc, (RT)0};
            continue;
        }
        const int kk[2] = {k, m - k};
        const V   zz[2] = {z[k], z[m - k]};
        V         x[2];
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const V zk = zz[s], zm = zz[1 - s];
            const V xe{(zk.x + zm.x) * half, (zk.y - zm.y) * half};
            const V xo{(zk.y + zm.y) * half, (zm.x - zk.x) * half};
            x[s] = cscale(cadd(xe, cmul(xo, twh[kk[s]])), sc);
        }
        z[k] = x[0];
        if (m - k != k) z[m - k] = x[1];
    }
}

// C2R merge before the inverse row kernel of the M-point view (in place on the bins)
template <class V>
__global__ void __launch_bounds__(256) c2r_merge_kernel(V* __restrict__ buf, const typename VecTraits<V>::W* __restrict__ twh, int m,
                                                        long long rows, long long rows_per_plane, long long pitch, long long plane) {
    using W = typename VecTraits<V>::W;
    using RT = typename real_of<W>::type;
    const int       pairs = m / 2 + 1;
    const long long total = rows * pairs;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const long long row = i / pairs;
        const int       k = (int)(i - row * pairs);
        const long long a = row / rows_per_plane, b = row - a * rows_per_plane;
        V*              x = buf + a * plane + b * pitch;
        const int       kk[2] = {k, m - k};
        V               xx[2] = {x[k], x[m - k]};
        if (k == 0) {  // bins 0 and M, imaginary parts ignored
            xx[0].y = (RT)0;
            xx[1].y = (RT)0;
        }
        V z[2];
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const V xk = xx[s], xp = xx[1 - s];
            const W w = twh[kk[s]];
            const V xe{xk.x + xp.x, xk.y - xp.y};
            const V d{xk.x - xp.x, xk.y + xp.y};
            const V xo{d.x * w.x + d.y * w.y, d.y * w.x - d.x * w.y};
            z[s] = V{xe.x - xo.y, xe.y + xo.x};
        }
        x[k] = z[0];
        if (k != 0 && m - k != k) x[m - k] = z[1];
    }
}

template <class V> hipError_t launch_split_merge(const RealLaunch& L, const void* twh, bool split, void* buf, hipStream_t stream) {
    using W = typename VecTraits<V>::W;
    const int       m = L.n2 / 2;
    const long long total = L.rows * (m / 2 + 1);
    const long long grid = std::max(1ll, std::min((total + 255) / 256, (long long)device_info().cus * 8));
    (void)hipGetLastError();
    if (split)
        hipLaunchKernelGGL(r2c_split_kernel<V>, dim3((unsigned)grid), dim3(256), 0, stream, (V*)buf, (const W*)twh, m, L.rows, L.rows_per_plane,
                           L.cpitch, L.cplane, L.scale == 0.0 ? 1.0 : L.scale);
    else
        hipLaunchKernelGGL(c2r_merge_kernel<V>, dim3((unsigned)grid), dim3(256), 0, stream, (V*)buf, (const W*)twh, m, L.rows, L.rows_per_plane,
                           L.cpitch, L.cplane);
    return hipGetLastError();
}

bool real_length_supported(long long n2) {
    return n2 >= 2 && n2 % 2 == 0 && n2 / 2 <= 4096 && fft_length_supported((int)(n2 / 2));
}

hipError_t launch_real_rows(const RealLaunch& L, hipStream_t stream) {
    if (!real_length_supported(L.n2) || (L.dir != 1 && L.dir != -1) || (L.dtype != F64 && L.dtype != F32)) return hipErrorInvalidValue;
    if ((L.rpitch | L.rplane) & 1) return hipErrorInvalidValue;
    if (L.rows <= 0) return hipSuccess;
    if (L.rows >= (1ll << 31) || L.rows_per_plane < 1 || L.rows_per_plane >= (1ll << 31)) return hipErrorInvalidValue;
    const int   m = L.n2 / 2;
    const void *tw = nullptr, *twh = nullptr;
    if (get_twiddles(m, L.dtype, &tw) != DFFT_OK || get_twiddles(L.n2, L.dtype, &twh) != DFFT_OK) return hipErrorOutOfMemory;
    switch (m) {
#define DFFT_REAL_CASE(N, GRP, E, ...) \
    case N: return RealInst<true, N>::run(L, tw, twh, stream);
        DFFT_PLAN_TABLE(DFFT_REAL_CASE)
#undef DFFT_REAL_CASE
        default: break;
    }
    // run-time-scheduled half-length: its kernel on the complex view + split / merge.  That kernel's row launches assume contiguous rows,
    // so the rows go in as a COLUMN launch of the transposed view (FFT index unit-stride, column c = row c of the plane; what
    // dfft_generic.hip makes of a row launch itself), which carries the row pitch of each side.
    if (L.rows % L.rows_per_plane != 0) return hipErrorInvalidValue;
    const bool fwd = L.dir > 0;
    FftLaunch  F;
    std::memset(&F, 0, sizeof(F));
    F.dtype = L.dtype;
    F.n = m;
    F.dir = L.dir;
    F.cols = 1;
    F.tw = tw;
    const AxisMap rm{m, 1, 0, 1, L.rpitch / 2, 0, 1, 0}, cm{m, 1, 0, 1, L.cpitch, 0, 1, 0};
    const TileMap rt{L.rplane / 2, L.rpitch / 2}, ct{L.cplane, L.cpitch};
    F.in = L.in;
    F.out = L.out;
    F.imap = fwd ? rm : cm;
    F.omap = fwd ? cm : rm;
    F.itile = fwd ? rt : ct;
    F.otile = fwd ? ct : rt;
    F.na = L.rows / L.rows_per_plane;
    F.ncols = (int)L.rows_per_plane;
    F.scale = fwd ? 1.0 : L.scale;
    hipError_t e;
    if (fwd) {
        e = launch_fft(F, stream);
        if (e == hipSuccess) e = L.dtype == F64 ? launch_split_merge<double2>(L, twh, true, L.out, stream) : launch_split_merge<float2>(L, twh, true, L.out, stream);
    } else {
        e = L.dtype == F64 ? launch_split_merge<double2>(L, twh, false, const_cast<void*>(L.in), stream)
                           : launch_split_merge<float2>(L, twh, false, const_cast<void*>(L.in), stream);
        if (e == hipSuccess) e = launch_fft(F, stream);
    }
    return e;
}

#endif

}  // namespace dfft
