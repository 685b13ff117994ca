// dfft_lxspec.hip -- long batched 1-D real cross-spectrum: two real fields x, g [batch][channels][n], every row zero-padded to m = 2 M,
//     S[c, k] = sum_b conj(rfft(x[b, c, :], m)[k]) rfft(g[b, c, :], m)[k],        k = 0 ... M,   out [channels][M + 1], unnormalised,
// for M = N1 * N2 beyond the single-pass range (the lengths of dfft_lconv.hip): the filter gradient of dfft_rconv1d_long.  It is the
// accumulating kernel of dfft_xspec.hip cut along the four-step decomposition of dfft_lconv.hip.  With z[j] = x[2j] + i x[2j+1] (zeros
// beyond n), j = j1 N2 + j2, k = k1 + N1 k2 and W_M = e^{-2 pi i / M}, per chunk of rows (lxspec_chunk_rows):
//   A    lxspec_a_kernel    what lconv_a_kernel does, once per field: N1-point forward transforms down the columns j2 of the row seen as
//                           [N1][N2] complex, read straight from the reals (rows of the tile beyond n are zeros in registers), times
//                           W_M^{k1 j2}, into scratch [field][rows][N1][N2].  The auto-spectrum (g == x) runs one field only.
//   Mid  lxspec_mid_kernel  one item per (slice, channel, pair of scratch rows (k1, N1 - k1)), one thread group per row (LxspecMidGeom, the
//                           geometry of lconv_mid_kernel; item 0 holds rows 0 and N1/2).  For every row of the channel in its slice, in
//                           order: load the two scratch rows of x, N2-point forward stages, ONE LDS exchange for Z[M - k] (the positions
//                           lconv_mid_kernel reads), 2 X[k] = (Z[k] + conj Z[M-k]) - i (Z[k] - conj Z[M-k]) w_k for the thread's own bins
//                           k = ka + N1 k2 with w_k = rowc[ka] colt[k2]; the same for g; conj(2 X[k]) 2 G[k] added to E running sums per
//                           thread.  Nothing is written per row.  Bins 0 and M come from Z[0] alone; the thread of (ka, k2) = (0, 0)
//                           keeps both, imaginary parts stored as exact zeros.  The auto-spectrum skips the second transform and adds
//                           |2 X[k]|^2 to the real parts alone (dfft_xspec.hip says why).  Times 1/4 once, at the store, in the order of
//                           the scratch: dest[slice][channel][ka N2 + k2], dest[slice][channel][M].
//   Red  lxspec_reduce_kernel  sums the slices in order and writes (first chunk) or adds to (later chunks) `out`, in natural order
//                           (order 0: bin k1 + N1 k2) or as it stands (order 1, the order of lconv_filter).
// A call of one chunk and one slice in order 1 has the Mid kernel store straight to `out`.  No atomics: rows of a slice in order, slices
// in order, chunks in order -- the same bits from call to call.  The cuts (lxspec_chunk_rows, lxspec_slices) are host arithmetic on
// (m, channels, batch, dtype) and fixed constants.
//
// Composed route (DFFT_RXSPEC_LONG_FUSED=0, the splits lxspec_fused_ok leaves out): dfft_batch.cpp runs pad -> real rows of length m as
// dfft_rfft1d dispatches them, on both fields -> lxspec_mac_kernel, which adds each channel's rows to `out` in row order.
//
// Compiled once per instantiation group (-DDFFT_INST_GROUP=g: the kernels of the factor lengths of group g) and once with
// -DDFFT_INST_GROUP=DFFT_NUM_INST_GROUPS (the dispatcher, the tables, the reduction and the kernels of the composed route).
#include "dfft_fused_host.h"
#include "dfft_lconv.h"
#include "dfft_lxspec.h"

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <tuple>
#include <vector>

#ifndef DFFT_INST_GROUP
#error "compile with -DDFFT_INST_GROUP=<g>"
#endif

namespace dfft {

constexpr int kLxspecLoBits = 12, kLxspecLo = 1 << kLxspecLoBits;

enum { LXSPEC_PASS_A = 0, LXSPEC_PASS_MID = 1 };

// One launch of one pass on a chunk of rows
struct LxspecPass {
    int         pass;
    int         dtype;
    long long   n, m, channels, rows, row0;  // row0: first row of the chunk in the call (channel = (row0 + r) % channels)
    long long   slices, steps;               // Mid: the cut of the chunk
    int         n1, n2;
    bool        vec, autos;
    const void* in;    // the chunk's rows of one field (pass A)
    void*       scr;   // pass A: [rows][N1][N2] complex of that field
    const void* sx;    // Mid: the scratch of x and of g
    const void* sg;
    void*       dest;  // Mid: [slices][channels][M + 1]
    const void* tw;    // e^{-2 pi i k / N}, N the length of the pass (N1: A; N2: Mid)
    const void* hi;    // W_M^{4096 t}
    const void* lo;    // W_M^t, t < 4096
    const void* rowc;  // e^{-2 pi i k1 / m}, k1 < N1
    const void* colt;  // e^{-2 pi i k2 / (2 N2)}, k2 < N2
};

// (N2, dtype) whose accumulating Mid kernel would keep values in scratch memory (tools/fused_resources.py lxspec, profiles/2026-10-20_rxspec1d_long/
// kernel_resources.txt) are not built: a split with such a longer factor runs the composed route.  Pass A of every factor length is built.
constexpr bool lxspec_fused_ok(int N, bool f64) {
#ifdef DFFT_LXSPEC_BUILD_ALL  // tools/fused_resources.py lxspec --build-all: every Mid kernel, to find the ones that spill
    return N > 0 || f64;
#endif
    // 24 and 20 points per thread in fp64, three live arrays: 208, 108, 164 and 288 bytes per lane (tools/fused_resources.py lxspec --build-all)
    if (f64 && (N == 384 || N == 640 || N == 1280 || N == 1536)) return false;
    return true;
}

// the family (dfft_fused_host.h); ok: the Mid kernel of N2 = N is built; run<N>, one pass of the factor length N: defined in the
// translation unit of N's group only
struct LxspecTag {
    using Launch = LxspecPass;
    static constexpr bool ok(int N, bool f64) { return lconv_factor(N) && N > 64 && lxspec_fused_ok(N, f64); }
    template <int N> static hipError_t run(const Launch& F, hipStream_t stream);
};

#if DFFT_INST_GROUP < DFFT_NUM_INST_GROUPS

// Column tiles of pass A: the rule of dfft_lconv.hip (LconvColsGeom)
template <class V, class P> constexpr int lxspec_max_threads() {
    constexpr bool f64 = sizeof(V) == 16;
    constexpr int  N = P::N;
    return (f64 ? N == 1024 : (N == 640 || N == 1280)) ? 256 : 512;
}
template <class V, class P> constexpr int lxspec_cols_per_tile() {
    int cb = cols_per_tile<V, P>();
    while (cb > 1 && ((long long)P::N * cb * (long long)sizeof(V) > 128 * 1024 || cb * P::T > lxspec_max_threads<V, P>())) cb /= 2;
    return cb;
}
template <class V, class P> struct LxspecColsGeom {
    static constexpr int CB = lxspec_cols_per_tile<V, P>();
    static constexpr int G = ConstMax1<256 / (CB * P::T)>::value;
    using KG = KernelGeom<V, P, CB, G, TuneDefault>;
    static_assert(KG::PH == 1, "one-phase tiles");
    static constexpr int EXR = (KG::LDS_ELEMS + 1) / 2 * 2;
    static constexpr size_t LDS_BYTES = (size_t)EXR * G * sizeof(V) + KG::TW_BYTES;
};

template <class V> __device__ __forceinline__ V lxspec_wm(const V* __restrict__ hi, const V* __restrict__ lo, int p) {
    return cmul(hi[p >> kLxspecLoBits], lo[p & (kLxspecLo - 1)]);
}

// Pass A.  Tile t = (row, block of CB columns j2); VEC: n even and `in` aligned to V, so z[j] is the complex element j of the row.
template <class V, class P, bool VEC>
__global__ void __attribute__((amdgpu_flat_work_group_size(1, LxspecColsGeom<V, P>::KG::THREADS)))
lxspec_a_kernel(const typename real_of<V>::type* __restrict__ in, V* __restrict__ scr, const typename VecTraits<V>::W* __restrict__ tw,
                const V* __restrict__ hi, const V* __restrict__ lo, long long n, int N2, unsigned tiles, unsigned tiles_per_row) {
    using CG = LxspecColsGeom<V, P>;
    using KG = typename CG::KG;
    using W = typename VecTraits<V>::W;
    using RT = typename real_of<V>::type;
    constexpr int  E = P::E, T = P::T, N1 = P::N, G = CG::G, GT = KG::GT, CB = CG::CB;
    constexpr bool TWPOW = KG::TWMODE == TW_REG;
    extern __shared__ __attribute__((aligned(16))) char dfft_smem[];
    const int g = threadIdx.x / GT;
    const int tid = (int)threadIdx.x - g * GT;
    const int c = tid % CB;
    const int j = tile_j<CB, KG::NW>(tid);
    V*        lds = reinterpret_cast<V*>(dfft_smem + KG::TW_BYTES) + g * CG::EXR;
    W         twreg[KG::TWMODE == TW_REG && KG::TWN > 0 ? KG::TWN : 1];
    const W*  twr = stage_twiddles<V, P, +1, KG>(twreg, reinterpret_cast<W*>(dfft_smem), tw, j);
    for (unsigned r0 = blockIdx.x * G; r0 < tiles; r0 += gridDim.x * G) {
        const unsigned  t = r0 + g;
        const unsigned  row = t < tiles ? t / tiles_per_row : 0u, cb = t < tiles ? t - row * tiles_per_row : 0u;
        const int       j2 = (int)cb * CB + c;
        const bool      va = t < tiles && j2 < N2;
        const long long base = (long long)row * n;  // 64-bit row bases
        V               v[E];
        if constexpr (VEC) {  // n even: a two-real value lies wholly inside the row or wholly in the padding
            const V* ip = reinterpret_cast<const V*>(in + base);
#pragma unroll
            for (int k = 0; k < E; ++k) {
                const long long idx = (long long)(j + T * k) * N2 + j2;
                v[k] = (va && 2 * idx < n) ? ip[idx] : V{0, 0};
            }
        } else {
            const RT* ip = in + base;
#pragma unroll
            for (int k = 0; k < E; ++k) {
                const long long idx = (long long)(j + T * k) * N2 + j2;
                v[k] = V{(va && 2 * idx < n) ? ip[2 * idx] : (RT)0, (va && 2 * idx + 1 < n) ? ip[2 * idx + 1] : (RT)0};
            }
        }
        group_sync<KG::WAVE_LOCAL>();  // the previous tile's stages are done with the tile
        run_stages<V, P, 0, +1, CB, KG::PAD, KG::WAVE_LOCAL, KG::TWMODE, TWPOW, KG::PH, 1, KG::NW, KG::LOCALX>(v, twr, lds, j, c);
        if (va) {
            V* op = scr + (long long)row * N1 * N2 + j2;
#pragma unroll
            for (int k = 0; k < E; ++k) {
                const int k1 = j + T * k;
                op[(long long)k1 * N2] = cmul(v[k], lxspec_wm<V>(hi, lo, k1 * j2));  // k1 j2 < M <= 2^22
            }
        }
    }
}

// Mid.  The geometry of lconv_mid_kernel: an even number of thread groups, groups 2q and 2q + 1 share item q of the workgroup.
template <class V, class P> struct LxspecMidGeom {
    static constexpr int IPB = ConstMax1<128 / P::T>::value;  // items per workgroup
    static constexpr int G = 2 * IPB;
    using KG = KernelGeom<V, P, 1, G, TuneDefault>;
    static constexpr int N2 = P::N;
    static constexpr int SPLIT = (KG::PAD ? N2 + N2 / 8 : N2) + 1;
    static constexpr int EXR = ((KG::LDS_ELEMS > SPLIT ? KG::LDS_ELEMS : SPLIT) + 1) / 2 * 2;
    static constexpr size_t LDS_BYTES = (size_t)EXR * G * sizeof(V) + KG::TW_BYTES;
    static_assert(LDS_BYTES <= 160 * 1024, "two rows and the twiddle copy fit the LDS");
    static constexpr bool TWH_REG = P::E * (int)sizeof(V) / 4 <= 32;
};

// v: one scratch row (the group's row ka) -> 2 X[k] of the thread's bins k = ka + N1 (j + T * (0 ... E-1)); returns 2 X[M] in the thread
// of bin 0.  Ends behind a workgroup barrier: every partner is read before the next transform's exchanges reuse the tiles.
template <class V, class P, class MG>
__device__ __forceinline__ typename real_of<V>::type lxspec_bins(V (&v)[P::E], const typename VecTraits<V>::W* twr, V* lds, const V* ptile,
                                                                  const typename VecTraits<V>::W (&wh)[MG::TWH_REG ? P::E : 1],
                                                                  const typename VecTraits<V>::W* __restrict__ colt,
                                                                  const typename VecTraits<V>::W wr, int ka, int j) {
    using KG = typename MG::KG;
    using W = typename VecTraits<V>::W;
    using RT = typename real_of<V>::type;
    constexpr int  E = P::E, T = P::T, N2 = P::N;
    constexpr bool TWPOW = KG::TWMODE == TW_REG;
    run_stages<V, P, 0, +1, 1, KG::PAD, KG::WAVE_LOCAL, KG::TWMODE, TWPOW, 1, 1, KG::NW, KG::LOCALX>(v, twr, lds, j, 0);
    __syncthreads();
#pragma unroll
    for (int k = 0; k < E; ++k) lds[lds_index<1, KG::PAD>(j + T * k, 0)] = v[k];
    __syncthreads();
    RT nyq = (RT)0;
#pragma unroll
    for (int k = 0; k < E; ++k) {
        const int kk = j + T * k;                                          // k2; the bin is ka + N1 kk
        const int pk = ka == 0 ? (kk == 0 ? 0 : N2 - kk) : N2 - 1 - kk;    // position of Z[M - k] in the partner's row
        const V   zm = ptile[lds_index<1, KG::PAD>(pk, 0)];
        const W   w = cmul(wr, MG::TWH_REG ? wh[MG::TWH_REG ? k : 0] : colt[kk]);  // e^{-2 pi i (ka + N1 kk) / m}
        const V   xe{v[k].x + zm.x, v[k].y - zm.y};                        // 2 Xe[k]
        const V   xo{v[k].y + zm.y, zm.x - v[k].x};                        // 2 Xo[k]
        const V   t = cmul(xo, w);
        if (ka == 0 && kk == 0) nyq = xe.x - xo.x;                         // 2 X[M] = 2 (Re Z[0] - Im Z[0])
        v[k] = V{xe.x + t.x, xe.y + t.y};
    }
    __syncthreads();
    return nyq;
}

// Item t = ((slice * channels + channel) * NI + i), i < NI = (N1 + 1) / 2: i == 0 holds the self-paired scratch rows 0 (group 0) and, N1
// even, N1/2 (group 1); i > 0 the rows i (group 0) and N1 - i (group 1), each the other's partner.  Step q of a channel is row
// rc + q * channels of the chunk, rc the channel's first row there; slice s holds steps [s per + min(s, rem), ...), per = steps / slices,
// rem = steps % slices.  Every group runs the trip count of the longest slice (the exchanges are workgroup barriers); steps beyond a
// group's own count, rows beyond the chunk and the groups without a row load zeros.
template <class V, class P>
__global__ void __attribute__((amdgpu_flat_work_group_size(1, LxspecMidGeom<V, P>::KG::THREADS)))
lxspec_mid_kernel(const V* __restrict__ sx, const V* __restrict__ sg, V* __restrict__ dest, const typename VecTraits<V>::W* __restrict__ tw,
                  const typename VecTraits<V>::W* __restrict__ rowc, const typename VecTraits<V>::W* __restrict__ colt, unsigned items, int N1,
                  unsigned channels, unsigned slices, unsigned steps, unsigned c0, unsigned nr, int autos) {
    using MG = LxspecMidGeom<V, P>;
    using KG = typename MG::KG;
    using W = typename VecTraits<V>::W;
    using RT = typename real_of<V>::type;
    constexpr int E = P::E, T = P::T, N2 = P::N, IPB = MG::IPB, GT = KG::GT;
    extern __shared__ __attribute__((aligned(16))) char dfft_smem[];
    const int g = threadIdx.x / GT;
    const int j = tile_j<1, KG::NW>((int)threadIdx.x - g * GT);
    V*        tiles = reinterpret_cast<V*>(dfft_smem + KG::TW_BYTES);
    V*        lds = tiles + g * MG::EXR;
    W         twreg[KG::TWMODE == TW_REG && KG::TWN > 0 ? KG::TWN : 1];
    const W*  twr = stage_twiddles<V, P, +1, KG>(twreg, reinterpret_cast<W*>(dfft_smem), tw, j);
    W         wh[MG::TWH_REG ? E : 1];
    if constexpr (MG::TWH_REG) {
#pragma unroll
        for (int k = 0; k < E; ++k) wh[k] = colt[j + T * k];
    }
    const unsigned  NI = (unsigned)(N1 + 1) / 2;
    const long long M = (long long)N1 * N2;
    const unsigned  per = steps / slices, rem = steps % slices, trips = per + (rem ? 1u : 0u);
    for (unsigned t0 = blockIdx.x * IPB; t0 < items; t0 += gridDim.x * IPB) {
        const unsigned t = t0 + (unsigned)(g >> 1);
        const bool     in_range = t < items;
        const unsigned sc = in_range ? t / NI : 0u;  // slice * channels + channel
        const int      i = in_range ? (int)(t - sc * NI) : 0;
        const unsigned s = sc / channels, c = sc - s * channels;
        const int      ka = i == 0 ? ((g & 1) ? N1 / 2 : 0) : ((g & 1) ? N1 - i : i);  // this group's scratch row
        const bool     valid = in_range && !(i == 0 && (g & 1) && (N1 & 1));           // odd N1: row 0 has no companion
        const V*       ptile = i == 0 ? lds : tiles + (g ^ 1) * MG::EXR;
        const unsigned q0 = s * per + (s < rem ? s : rem), count = valid ? per + (s < rem ? 1u : 0u) : 0u;
        const unsigned rc = (c + channels - c0) % channels;  // the channel's first row in the chunk
        const W        wr = rowc[valid ? ka : 0];
        V              acc[E];
        RT             accn = (RT)0;
#pragma unroll
        for (int k = 0; k < E; ++k) acc[k] = V{0, 0};
        for (unsigned q = 0; q < trips; ++q) {
            const unsigned long long r = rc + (unsigned long long)(q0 + q) * channels;
            const bool               live = q < count && r < nr;
            const long long          base = live ? (long long)r * M + (long long)ka * N2 : 0ll;  // 64-bit row bases
            V                        v[E];
#pragma unroll
            for (int k = 0; k < E; ++k) v[k] = live ? sx[base + j + T * k] : V{0, 0};
            const RT xn = lxspec_bins<V, P, MG>(v, twr, lds, ptile, wh, colt, wr, ka, j);
            RT       gn = xn;
            V        xr[E];
#pragma unroll
            for (int k = 0; k < E; ++k) xr[k] = v[k];
            if (!autos) {  // (the same in every thread of the launch)
#pragma unroll
                for (int k = 0; k < E; ++k) v[k] = live ? sg[base + j + T * k] : V{0, 0};
                gn = lxspec_bins<V, P, MG>(v, twr, lds, ptile, wh, colt, wr, ka, j);
            }
#pragma unroll
            for (int k = 0; k < E; ++k) {  // conj(X) G; the auto-spectrum's imaginary parts stay exact zeros
                const RT re = xr[k].x * v[k].x + xr[k].y * v[k].y, im = xr[k].x * v[k].y - xr[k].y * v[k].x;
                acc[k].x += re;
                acc[k].y += autos ? (RT)0 : im;
            }
            accn += xn * gn;
        }
        if (valid) {
            V* op = dest + (size_t)sc * (size_t)(M + 1) + (size_t)ka * N2;
#pragma unroll
            for (int k = 0; k < E; ++k) {
                const int  kk = j + T * k;
                const bool k0 = ka == 0 && kk == 0;
                op[kk] = V{acc[k].x * (RT)0.25, k0 ? (RT)0 : acc[k].y * (RT)0.25};
                if (k0) op[M] = V{accn * (RT)0.25, (RT)0};
            }
        }
    }
}

template <class V, class P, bool VEC> hipError_t launch_lxspec_a(const LxspecPass& F, hipStream_t stream) {
    using CG = LxspecColsGeom<V, P>;
    using W = typename VecTraits<V>::W;
    using RT = typename real_of<V>::type;
    auto                    kern = lxspec_a_kernel<V, P, VEC>;
    static std::atomic<int> blocks_per_cu[kMaxDevices];
    hipError_t              e;
    const int               bpc = resident_blocks_per_cu(reinterpret_cast<const void*>(kern), CG::KG::THREADS, CG::LDS_BYTES, blocks_per_cu, &e);
    if (bpc == 0) return e;
    const long long per_row = (F.n2 + CG::CB - 1) / CG::CB, tiles = F.rows * per_row;
    if (tiles >= (1ll << 31)) return hipErrorInvalidValue;
    const long long grid = std::max(1ll, persistent_grid(device_info().cus, bpc, (tiles + CG::G - 1) / CG::G));
    (void)hipGetLastError();
    hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(CG::KG::THREADS), CG::LDS_BYTES, stream, (const RT*)F.in, (V*)F.scr, (const W*)F.tw, (const V*)F.hi,
                       (const V*)F.lo, F.n, F.n2, (unsigned)tiles, (unsigned)per_row);
    return hipGetLastError();
}

template <class V, class P> hipError_t launch_lxspec_mid(const LxspecPass& F, hipStream_t stream) {
    using MG = LxspecMidGeom<V, P>;
    using W = typename VecTraits<V>::W;
    auto                    kern = lxspec_mid_kernel<V, P>;
    static std::atomic<int> blocks_per_cu[kMaxDevices];
    hipError_t              e;
    const int               bpc = resident_blocks_per_cu(reinterpret_cast<const void*>(kern), MG::KG::THREADS, MG::LDS_BYTES, blocks_per_cu, &e);
    if (bpc == 0) return e;
    const long long items = F.slices * F.channels * ((F.n1 + 1) / 2);
    if (items >= (1ll << 31) || F.steps >= (1ll << 31) || F.slices < 1 || F.slices > F.steps) return hipErrorInvalidValue;
    const long long grid = std::max(1ll, persistent_grid(device_info().cus, bpc, (items + MG::IPB - 1) / MG::IPB));
    (void)hipGetLastError();
    hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(MG::KG::THREADS), MG::LDS_BYTES, stream, (const V*)F.sx, (const V*)F.sg, (V*)F.dest, (const W*)F.tw,
                       (const W*)F.rowc, (const W*)F.colt, (unsigned)items, F.n1, (unsigned)F.channels, (unsigned)F.slices, (unsigned)F.steps,
                       (unsigned)(F.row0 % F.channels), (unsigned)F.rows, F.autos ? 1 : 0);
    return hipGetLastError();
}

template <class V, int N> hipError_t lxspec_run_typed(const LxspecPass& F, hipStream_t stream) {
    using P = typename PlanFor<N>::type;
    if constexpr (lconv_factor(N)) {
        if (F.pass == LXSPEC_PASS_MID) {
            if constexpr (N > 64 && lxspec_fused_ok(N, sizeof(V) == 16))  // N2 >= N1 >= 64 and N1 N2 > 4096: 64 is never the longer factor
                return launch_lxspec_mid<V, P>(F, stream);
            return hipErrorInvalidValue;
        }
        return F.vec ? launch_lxspec_a<V, P, true>(F, stream) : launch_lxspec_a<V, P, false>(F, stream);
    }
    return hipErrorInvalidValue;  // not built (lconv_factor, lxspec_fused_ok): the dispatcher does not come here
}
template <int N> hipError_t LxspecTag::run(const LxspecPass& F, hipStream_t stream) {
    if (F.dtype == F64) return lxspec_run_typed<double2, N>(F, stream);
    if (F.dtype == F32) return lxspec_run_typed<float2, N>(F, stream);
    return hipErrorInvalidValue;
}
DFFT_FUSED_INSTANTIATE(LxspecTag)

#else  // the dispatcher, the tables, the reduction and the kernels of the composed route

// position of natural bin order's element for position i of the scratch order: i = k1 N2 + k2 -> k1 + N1 k2; i = M -> M
__device__ __forceinline__ long long lxspec_natural(long long i, int N1, int N2) {
    const long long k1 = i / N2, k2 = i - k1 * N2;
    return i == (long long)N1 * N2 ? i : k1 + N1 * k2;
}

// out[c][pos(i)] (+)= partial[0][c][i] + partial[1][c][i] + ... in slice order; pos(i) = i (order 1) or the natural bin (order 0)
template <class V>
__global__ void __launch_bounds__(256) lxspec_reduce_kernel(const V* __restrict__ partial, V* __restrict__ out, long long channels, int N1, int N2,
                                                            unsigned slices, int order, int first) {
    const long long nb = (long long)N1 * N2 + 1, ce = channels * nb;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < ce; e += (long long)gridDim.x * 256) {
        V acc = partial[e];
        for (unsigned s = 1; s < slices; ++s) {
            const V p = partial[(long long)s * ce + e];
            acc.x += p.x;
            acc.y += p.y;
        }
        const long long c = e / nb, i = e - c * nb;
        V*              op = out + c * nb + (order ? i : lxspec_natural(i, N1, N2));
        if (first) {
            *op = acc;
        } else {
            const V o = *op;
            *op = V{o.x + acc.x, o.y + acc.y};
        }
    }
}
// rxspec_mac_kernel of dfft_xspec.hip with the store order: out[c][i] (+)= sum over the chunk's rows r of channel c, in row order, of
// conj(xb[r][k]) gb[r][k], k the natural bin of position i.  `first`: the chunk starts the sum.  autos: gb is xb, the sum is of |xb|^2.
template <class V>
__global__ void __launch_bounds__(256) lxspec_mac_kernel(const V* xb, const V* gb, V* __restrict__ out, int N1, int N2, long long row0, long long nr,
                                                         long long channels, int order, int first, int autos) {
    using RT = typename real_of<V>::type;
    const long long nb = (long long)N1 * N2 + 1, total = channels * nb;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
        const long long c = e / nb, i = e - c * nb;
        const long long k = order ? lxspec_natural(i, N1, N2) : i;
        V               acc = first ? V{0, 0} : out[e];
        for (long long r = (c - row0 % channels + channels) % channels; r < nr; r += channels) {
            const V a = xb[r * nb + k];
            if (autos) {
                acc.x += a.x * a.x + a.y * a.y;
            } else {
                const V b = gb[r * nb + k];
                acc.x += a.x * b.x + a.y * b.y;
                acc.y += a.x * b.y - a.y * b.x;
            }
        }
        if (k == 0 || k == nb - 1) acc.y = (RT)0;  // DC and Nyquist
        out[e] = acc;
    }
}

namespace {

// the tables of one (device, m, dtype): built once, kept for the life of the process (about 100 KiB)
struct LxspecTables {
    void *hi, *lo, *rowc, *colt;
};
std::mutex                                              g_mutex;
std::map<std::tuple<int, long long, int>, LxspecTables> g_tables;

int upload_table(long long count, long long num_step, long long den, int dtype, void** dptr) {  // e^{-2 pi i (t num_step mod den) / den}
    const long double two_pi = 6.283185307179586476925286766559005768L;
    const size_t      eb = elem_bytes(dtype);
    std::vector<char> h((size_t)count * eb);
    for (long long t = 0; t < count; ++t) {
        const long double a = two_pi * (long double)((t * num_step) % den) / (long double)den;
        if (dtype == F64) {
            ((double*)h.data())[2 * t] = (double)cosl(a);
            ((double*)h.data())[2 * t + 1] = (double)(-sinl(a));
        } else {
            ((float*)h.data())[2 * t] = (float)cosl(a);
            ((float*)h.data())[2 * t + 1] = (float)(-sinl(a));
        }
    }
    DFFT_HIP_TRY(hipMalloc(dptr, h.size()));
    DFFT_HIP_TRY(hipMemcpy(*dptr, h.data(), h.size(), hipMemcpyHostToDevice));
    return DFFT_OK;
}

int lxspec_tables(long long m, int n1, int n2, int dtype, LxspecTables* out) {
    int dev = 0;
    DFFT_HIP_TRY(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lk(g_mutex);
    const auto                  key = std::make_tuple(dev, m, dtype);
    const auto                  it = g_tables.find(key);
    if (it != g_tables.end()) {
        *out = it->second;
        return DFFT_OK;
    }
    const long long M = m / 2;
    LxspecTables    t{nullptr, nullptr, nullptr, nullptr};
    int             rc = upload_table((M + kLxspecLo - 1) >> kLxspecLoBits, kLxspecLo, M, dtype, &t.hi);
    if (rc == DFFT_OK) rc = upload_table(kLxspecLo, 1, M, dtype, &t.lo);
    if (rc == DFFT_OK) rc = upload_table(n1, 1, m, dtype, &t.rowc);
    if (rc == DFFT_OK) rc = upload_table(n2, 1, 2ll * n2, dtype, &t.colt);
    if (rc) {
        for (void* p : {t.hi, t.lo, t.rowc, t.colt})
            if (p) (void)hipFree(p);
        return rc;
    }
    g_tables[key] = t;
    *out = t;
    return DFFT_OK;
}

bool rows_ok(long long channels, long long rows) { return channels >= 1 && rows >= 1 && channels < (1ll << 31) && rows < (1ll << 31); }

}  // namespace

bool lxspec_fused_env() { return env_switch_on("DFFT_RXSPEC_LONG_FUSED"); }

bool lxspec_fused(long long m, int dtype) {
    int n1 = 0, n2 = 0;
    if ((dtype != F64 && dtype != F32) || !lconv_split(m, &n1, &n2)) return false;
    return tuned_built<LxspecTag>(n2, dtype == F64);
}

long long lxspec_chunk_rows(long long m, int dtype, long long rows, size_t cap) { return chunk_units(2 * (size_t)(m / 2) * elem_bytes(dtype), rows, cap); }

long long lxspec_slices(long long m, long long channels, long long rows) {
    int n1 = 0, n2 = 0;
    if (!rows_ok(channels, rows) || !lconv_split(m, &n1, &n2)) return 0;
    const long long steps = (rows + channels - 1) / channels;
    return std::max(1ll, std::min(kLxspecTargetItems / (channels * ((n1 + 1) / 2)), steps / kLxspecMinSteps));
}

size_t lxspec_scratch_bytes(long long m, int dtype, long long channels, long long rows, size_t cap) {
    if (!rows_ok(channels, rows) || !lconv_split(m, nullptr, nullptr) || (dtype != F64 && dtype != F32)) return 0;
    const long long nr = lxspec_chunk_rows(m, dtype, rows, cap);
    return ((size_t)nr * 2 * (size_t)(m / 2) + (size_t)lxspec_slices(m, channels, nr) * (size_t)channels * (size_t)(m / 2 + 1)) * elem_bytes(dtype);
}

int lxspec_run(const LxspecLaunch& L, size_t cap, void* scratch, size_t scratch_bytes, hipStream_t stream) {
    int n1 = 0, n2 = 0;
    if (L.n < 1 || L.m < L.n || !lconv_split(L.m, &n1, &n2) || L.channels < 1 || L.batch < 1 || (L.dtype != F64 && L.dtype != F32) ||
        (L.order != 0 && L.order != 1) || !L.x || !L.g || !L.out)
        return fail(DFFT_EINVAL, "lxspec: bad arguments");
    if (!lxspec_fused(L.m, L.dtype)) return fail(DFFT_EINVAL, "lxspec: m = " + std::to_string(L.m) + " has no fused kernels");
    const long long rows = L.batch * L.channels, M = L.m / 2;
    if (L.channels >= (1ll << 31) || L.batch >= (1ll << 31) || rows >= (1ll << 31)) return fail(DFFT_EINVAL, "lxspec: 2^31 or more rows");
    const size_t    cs = elem_bytes(L.dtype), rs = cs / 2;
    const long long nr = lxspec_chunk_rows(L.m, L.dtype, rows, cap);
    if (!scratch || scratch_bytes < lxspec_scratch_bytes(L.m, L.dtype, L.channels, rows, cap)) return fail(DFFT_EINVAL, "lxspec: scratch buffer too small");
    if (L.channels * ((n1 + 1) / 2) >= (1ll << 31)) return fail(DFFT_EUNSUPPORTED, "lxspec: channels * ceil(N1 / 2) = 2^31 or more items");
    LxspecTables T;
    if (int rc = lxspec_tables(L.m, n1, n2, L.dtype, &T)) return rc;
    const bool autos = L.x == L.g;
    char*      sx = (char*)scratch;                                // [nr][M]
    char*      sg = autos ? sx : sx + (size_t)nr * M * cs;         // [nr][M]
    char*      partial = sx + (size_t)nr * 2 * (size_t)M * cs;     // [slices][channels][M + 1]
    LxspecPass F;
    std::memset(&F, 0, sizeof(F));
    F.dtype = L.dtype;
    F.n = L.n;
    F.m = L.m;
    F.channels = L.channels;
    F.n1 = n1;
    F.n2 = n2;
    F.vec = L.n % 2 == 0 && (uintptr_t)L.x % cs == 0 && (uintptr_t)L.g % cs == 0;
    F.autos = autos;
    F.sx = sx;
    F.sg = sg;
    F.hi = T.hi;
    F.lo = T.lo;
    F.rowc = T.rowc;
    F.colt = T.colt;
    const void *tw1 = nullptr, *tw2 = nullptr;
    if (int rc = get_twiddles(n1, L.dtype, &tw1)) return rc;
    if (int rc = get_twiddles(n2, L.dtype, &tw2)) return rc;
    for (long long r0 = 0; r0 < rows; r0 += nr) {
        F.rows = std::min(nr, rows - r0);
        F.row0 = r0;
        F.steps = (F.rows + L.channels - 1) / L.channels;
        F.slices = lxspec_slices(L.m, L.channels, F.rows);
        const bool direct = rows <= nr && F.slices == 1 && L.order == 1;
        F.dest = direct ? L.out : (void*)partial;
        F.pass = LXSPEC_PASS_A;
        F.tw = tw1;
        for (int field = 0; field < (autos ? 1 : 2); ++field) {
            F.in = (const char*)(field ? L.g : L.x) + (size_t)r0 * L.n * rs;
            F.scr = field ? sg : sx;
            const hipError_t e = run_tuned<LxspecTag>(n1, F, stream);
            if (e != hipSuccess) return fail(DFFT_EHIP, std::string("lxspec (pass A): ") + hipGetErrorString(e));
        }
        F.pass = LXSPEC_PASS_MID;
        F.tw = tw2;
        const hipError_t e = run_tuned<LxspecTag>(n2, F, stream);
        if (e != hipSuccess) return fail(DFFT_EHIP, std::string("lxspec (mid): ") + hipGetErrorString(e));
        if (!direct) {
            const dim3 grid(elementwise_grid(L.channels * (M + 1)));
            (void)hipGetLastError();
            if (L.dtype == F64)
                hipLaunchKernelGGL(lxspec_reduce_kernel<double2>, grid, dim3(256), 0, stream, (const double2*)partial, (double2*)L.out, L.channels, n1, n2,
                                   (unsigned)F.slices, L.order, r0 == 0 ? 1 : 0);
            else
                hipLaunchKernelGGL(lxspec_reduce_kernel<float2>, grid, dim3(256), 0, stream, (const float2*)partial, (float2*)L.out, L.channels, n1, n2,
                                   (unsigned)F.slices, L.order, r0 == 0 ? 1 : 0);
            DFFT_HIP_TRY(hipGetLastError());
        }
    }
    return DFFT_OK;
}

int lxspec_mac(const void* xb, const void* gb, void* out, long long m, long long row0, long long nr, long long channels, int dtype, int order,
               hipStream_t stream) {
    int n1 = 0, n2 = 0;
    if (!lconv_split(m, &n1, &n2)) return fail(DFFT_EINVAL, "lxspec_mac: bad arguments");
    const dim3 grid(elementwise_grid(channels * (m / 2 + 1)));
    const int  autos = xb == gb ? 1 : 0, first = row0 == 0 ? 1 : 0;
    (void)hipGetLastError();
    if (dtype == F64)
        hipLaunchKernelGGL(lxspec_mac_kernel<double2>, grid, dim3(256), 0, stream, (const double2*)xb, (const double2*)gb, (double2*)out, n1, n2, row0, nr,
                           channels, order, first, autos);
    else
        hipLaunchKernelGGL(lxspec_mac_kernel<float2>, grid, dim3(256), 0, stream, (const float2*)xb, (const float2*)gb, (float2*)out, n1, n2, row0, nr, channels,
                           order, first, autos);
    DFFT_HIP_TRY(hipGetLastError());
    return DFFT_OK;
}

#endif

}  // namespace dfft
