// dfft_lconv.hip -- long batched 1-D real FFT convolution: every row of reals [batch][channels][n] filtered by its channel's spectrum,
//     y[b, c, :] = irfft(rfft(x[b, c, :], m) * H[c, :], m)[:n],        H [channels][m/2 + 1],  n <= m,  m = 2 M,
// for M = N1 * N2 beyond the single-pass range (8192 < m <= 2^23; N1 <= N2 two tuned single-pass lengths, lconv_factor): the fused kernel
// of dfft_rconv.hip cut along the four-step decomposition of its two M-point transforms (dfft_long.hip).  With z[j] = x[2j] + i x[2j+1]
// (zeros beyond n), j = j1 N2 + j2, k = k1 + N1 k2 and W_M = e^{-2 pi i / M}, per chunk of rows:
//   A    lconv_a_kernel    N1-point forward transforms down the columns j2 of the row seen as [N1][N2] complex -- tiles of CB adjacent
//                          columns (the tiles of dfft_real_cols.hip), read straight from the reals: rows of the tile beyond n are zeros in
//                          registers -- times W_M^{k1 j2}, into scratch [rows][N1][N2]
//   Mid  lconv_mid_kernel  one item per pair of scratch rows (k1, N1 - k1), one thread group per row: N2-point forward stages, after which
//                          row k1 holds Z[k1 + N1 k2] at position k2; ONE LDS exchange brings Z[M - k] -- row N1 - k1, position
//                          N2 - 1 - k2 (row 0: itself, position (N2 - k2) mod N2, Z[M] = Z[0]) -- and the pair / multiply / merge step of
//                          rconv_rows_kernel (dfft_rconv.hip) forms Z'[k]; N2-point inverse as conj . forward . conj; back over the same rows.
//                          The pairing twiddle e^{-2 pi i k / m} = e^{-2 pi i k1 / m} e^{-2 pi i k2 / (2 N2)}: a per-row constant times a
//                          per-thread table.  The filter is read in the order of the scratch (lconv_filter_kernel: hp[c][k1 N2 + k2] =
//                          H[c][k1 + N1 k2], hp[c][M] = H[c][M]), so both H[k] and H[M - k] are contiguous runs.
//   C    lconv_c_kernel    Z' W_M^{-k1 j2}, N1-point inverse transforms down the columns, Re / Im stored as the reals 2j, 2j + 1 < n.
// Three launches, 2 n + 4 m reals of traffic per row; the zero padding, the spectrum and the truncated tail never exist in memory.  In
// place (out == in): pass A of a chunk has read all of the chunk's rows before its pass C stores any (stream order).
// W_M^p (p = k1 j2 < M) is hi[p / 4096] * lo[p % 4096], the two small tables of dfft_long.hip's twiddle pass.
//
// Composed route (DFFT_RCONV_LONG_FUSED=0, the splits lconv_fused_ok leaves out): dfft_batch.cpp runs pad -> real rows of length m as
// dfft_rfft1d dispatches them -> multiply -> inverse -> truncate with the three small kernels at the end of this file.
//
// Compiled once per instantiation group (-DDFFT_INST_GROUP=g: the kernels of the factor lengths of group g) and once with
// -DDFFT_INST_GROUP=DFFT_NUM_INST_GROUPS (the dispatcher, the tables, the filter permutation and the kernels of the composed route).
#include "dfft_fused_host.h"
#include "dfft_lconv.h"

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

constexpr int kLconvLoBits = 12, kLconvLo = 1 << kLconvLoBits;

enum { LCONV_PASS_A = 0, LCONV_PASS_MID = 1, LCONV_PASS_C = 2 };

// One launch of one pass on a chunk of rows
struct LconvPass {
    int         pass;
    int         dtype, filter_kind;
    long long   n, m, channels, rows, row0;  // row0: first row of the chunk in the call (filter row = (row0 + r) % channels)
    int         n1, n2;
    bool        vec;
    const void* in;    // the chunk's rows (pass A)
    void*       out;   // the chunk's rows (pass C)
    void*       scr;   // [rows][N1][N2] complex
    const void* hp;
    const void* tw;    // e^{-2 pi i k / N}, N the length of the pass (N1: A, C; N2: Mid)
    const void* hi;    // W_M^{4096 t}
    const void* lo;    // W_M^t, t < 4096
    const void* rowc;  // e^{-2 pi i k1 / m}, k1 < N1
    const void* colt;  // e^{-2 pi i k2 / (2 N2)}, k2 < N2
};

// (N, dtype) whose instantiations would keep values in scratch memory (tools/fused_resources.py lconv, profiles/2026-10-20_rconv1d_long/
// kernel_resources.txt) are not built: a split with such a factor runs the composed route.  All kernels of an (N, dtype) go together.
constexpr bool lconv_fused_ok(int N, bool f64) {
    (void)N;
    (void)f64;
    return true;
}

// the family (dfft_fused_host.h); run<N>, one pass of the factor length N: defined in the translation unit of N's group only
struct LconvTag {
    using Launch = LconvPass;
    static constexpr bool ok(int N, bool f64) { return lconv_factor(N) && lconv_fused_ok(N, f64); }
    template <int N> static hipError_t run(const Launch& F, hipStream_t stream);
};

#if DFFT_INST_GROUP < DFFT_NUM_INST_GROUPS

// Column tiles of passes A and C: the rule of dfft_real_cols.hip (the C2C column kernel's width, halved until the tile holds at most
// 128 KiB in one phase and the workgroup at most 512 threads -- 256 for the lengths that kept 16 ... 128 bytes per lane in scratch at 512)
template <class V, class P> constexpr int lconv_max_threads() {
    constexpr bool f64 = sizeof(V) == 16;
    constexpr int  N = P::N;
    return (f64 ? N == 1024 : (N == 640 || N == 1280)) ? 256 : 512;
}
template <class V, class P> constexpr int lconv_cols_per_tile() {
    int cb = cols_per_tile<V, P>();
    while (cb > 1 && ((long long)P::N * cb * (long long)sizeof(V) > 128 * 1024 || cb * P::T > lconv_max_threads<V, P>())) cb /= 2;
    return cb;
}
template <class V, class P> struct LconvColsGeom {
    static constexpr int CB = lconv_cols_per_tile<V, P>();
    static constexpr int G = ConstMax1<256 / (CB * P::T)>::value;
    using KG = KernelGeom<V, P, CB, G, TuneDefault>;
    static_assert(KG::PH == 1, "one-phase tiles");
    static constexpr int EXR = (KG::LDS_ELEMS + 1) / 2 * 2;
    static constexpr size_t LDS_BYTES = (size_t)EXR * G * sizeof(V) + KG::TW_BYTES;
};

template <class V> __device__ __forceinline__ V lconv_wm(const V* __restrict__ hi, const V* __restrict__ lo, int p) {
    return cmul(hi[p >> kLconvLoBits], lo[p & (kLconvLo - 1)]);
}

// Pass A.  Tile t = (row, block of CB columns j2); VEC: n even and `in` aligned to V, so z[j] is the complex element j of the row.
template <class V, class P, bool VEC>
__global__ void __attribute__((amdgpu_flat_work_group_size(1, LconvColsGeom<V, P>::KG::THREADS)))
lconv_a_kernel(const typename real_of<V>::type* __restrict__ in, V* __restrict__ scr, const typename VecTraits<V>::W* __restrict__ tw,
               const V* __restrict__ hi, const V* __restrict__ lo, long long n, int N2, unsigned tiles, unsigned tiles_per_row) {
    using CG = LconvColsGeom<V, P>;
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
                op[(long long)k1 * N2] = cmul(v[k], lconv_wm<V>(hi, lo, k1 * j2));  // k1 j2 < M <= 2^22
            }
        }
    }
}

// Pass C.  VEC: n even and `out` aligned to V.
template <class V, class P, bool VEC>
__global__ void __attribute__((amdgpu_flat_work_group_size(1, LconvColsGeom<V, P>::KG::THREADS)))
lconv_c_kernel(const V* __restrict__ scr, typename real_of<V>::type* __restrict__ out, const typename VecTraits<V>::W* __restrict__ tw,
               const V* __restrict__ hi, const V* __restrict__ lo, long long n, int N2, unsigned tiles, unsigned tiles_per_row) {
    using CG = LconvColsGeom<V, P>;
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
    const W*  twr = stage_twiddles<V, P, -1, KG>(twreg, reinterpret_cast<W*>(dfft_smem), tw, j);
    for (unsigned r0 = blockIdx.x * G; r0 < tiles; r0 += gridDim.x * G) {
        const unsigned  t = r0 + g;
        const unsigned  row = t < tiles ? t / tiles_per_row : 0u, cb = t < tiles ? t - row * tiles_per_row : 0u;
        const int       j2 = (int)cb * CB + c;
        const bool      va = t < tiles && j2 < N2;
        const V*        ip = scr + (long long)row * N1 * N2 + (va ? j2 : 0);
        V               v[E];
#pragma unroll
        for (int k = 0; k < E; ++k) {
            const int k1 = j + T * k;
            if (va) {
                const V w = lconv_wm<V>(hi, lo, k1 * j2);
                v[k] = cmul(ip[(long long)k1 * N2], V{w.x, -w.y});
            } else {
                v[k] = V{0, 0};
            }
        }
        group_sync<KG::WAVE_LOCAL>();  // the previous tile's stages are done with the tile
        run_stages<V, P, 0, -1, CB, KG::PAD, KG::WAVE_LOCAL, KG::TWMODE, TWPOW, KG::PH, 1, KG::NW, KG::LOCALX>(v, twr, lds, j, c);
        if (va) {
            const long long base = (long long)row * n;
            if constexpr (VEC) {
                V* op = reinterpret_cast<V*>(out + base);
#pragma unroll
                for (int k = 0; k < E; ++k) {
                    const long long idx = (long long)(j + T * k) * N2 + j2;
                    if (2 * idx < n) op[idx] = v[k];
                }
            } else {
                RT* op = out + base;
#pragma unroll
                for (int k = 0; k < E; ++k) {
                    const long long idx = (long long)(j + T * k) * N2 + j2;
                    if (2 * idx < n) op[2 * idx] = v[k].x;
                    if (2 * idx + 1 < n) op[2 * idx + 1] = v[k].y;
                }
            }
        }
    }
}

// Mid.  Geometry of the row kernels (RconvGeom) with an even number of thread groups: groups 2q and 2q + 1 share item q of the workgroup.
template <class V, class P> struct LconvMidGeom {
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

// Item t = (row, i), i < NI = (N1 + 1) / 2: i == 0 holds the self-paired scratch rows 0 (group 0) and, N1 even, N1/2 (group 1); i > 0 the
// rows i (group 0) and N1 - i (group 1), each the other's partner.
template <class V, class P, bool HREAL>
__global__ void __attribute__((amdgpu_flat_work_group_size(1, LconvMidGeom<V, P>::KG::THREADS)))
lconv_mid_kernel(V* scr, const typename RconvFilter<V, HREAL>::T* __restrict__ h, const typename VecTraits<V>::W* __restrict__ tw,
                 const typename VecTraits<V>::W* __restrict__ rowc, const typename VecTraits<V>::W* __restrict__ colt, unsigned items, int N1,
                 unsigned row0, unsigned channels, double scale) {
    using MG = LconvMidGeom<V, P>;
    using KG = typename MG::KG;
    using W = typename VecTraits<V>::W;
    using RT = typename real_of<V>::type;
    using F = RconvFilter<V, HREAL>;
    constexpr int  E = P::E, T = P::T, N2 = P::N, IPB = MG::IPB, GT = KG::GT;
    constexpr bool TWPOW = KG::TWMODE == TW_REG;
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
    const RT       sc = (RT)scale;
    const unsigned NI = (unsigned)(N1 + 1) / 2;
    const int      M = N1 * N2;
    for (unsigned t0 = blockIdx.x * IPB; t0 < items; t0 += gridDim.x * IPB) {
        const unsigned t = t0 + (unsigned)(g >> 1);
        const unsigned row = t < items ? t / NI : 0u;
        const int      i = t < items ? (int)(t - row * NI) : 0;
        const int      ka = i == 0 ? ((g & 1) ? N1 / 2 : 0) : ((g & 1) ? N1 - i : i);  // this group's scratch row
        const bool     valid = t < items && !(i == 0 && (g & 1) && (N1 & 1));           // odd N1: row 0 has no companion
        const int      kb = ka == 0 ? 0 : N1 - ka;                                       // the partner's row
        const V*       ptile = i == 0 ? lds : tiles + (g ^ 1) * MG::EXR;
        V*             sp = scr + (long long)row * M + (long long)ka * N2;
        V              v[E];
#pragma unroll
        for (int k = 0; k < E; ++k) v[k] = valid ? sp[j + T * k] : V{0, 0};
        run_stages<V, P, 0, +1, 1, KG::PAD, KG::WAVE_LOCAL, KG::TWMODE, TWPOW, 1, 1, KG::NW, KG::LOCALX>(v, twr, lds, j, 0);
        __syncthreads();
#pragma unroll
        for (int k = 0; k < E; ++k) lds[lds_index<1, KG::PAD>(j + T * k, 0)] = v[k];
        __syncthreads();
        const typename F::T* hc = h + (size_t)(valid ? (row0 + row) % channels : 0u) * (size_t)(M + 1);
        const W              wr = rowc[valid ? ka : 0];
#pragma unroll
        for (int k = 0; k < E; ++k) {
            const int  kk = j + T * k;                                                  // k2; the bin is ka + N1 kk
            const int  pk = ka == 0 ? (kk == 0 ? 0 : N2 - kk) : N2 - 1 - kk;            // position of Z[M - k] in the partner's row
            const bool k0 = ka == 0 && kk == 0;
            const V    zm = ptile[lds_index<1, KG::PAD>(pk, 0)];
            const W    w = cmul(wr, MG::TWH_REG ? wh[MG::TWH_REG ? k : 0] : colt[kk]);  // e^{-2 pi i (ka + N1 kk) / m}
            const V    xe{v[k].x + zm.x, v[k].y - zm.y};                                // 2 Xe[k]
            const V    xo{v[k].y + zm.y, zm.x - v[k].x};                                // 2 Xo[k]
            const V    tt = cmul(xo, w);
            V          ya = F::mul(V{xe.x + tt.x, xe.y + tt.y}, hc[ka * N2 + kk], sc);              // Y[k]   = X[k] H[k] / m
            V          yb = F::mul(V{xe.x - tt.x, tt.y - xe.y}, hc[k0 ? M : kb * N2 + pk], sc);     // Y[M-k] = conj(Xe - W^k Xo) H[M-k] / m
            if (k0) {  // the imaginary parts of the DC and Nyquist products are ignored
                ya.y = (RT)0;
                yb.y = (RT)0;
            }
            const V s{ya.x + yb.x, ya.y - yb.y};
            const V d{ya.x - yb.x, ya.y + yb.y};
            const V o{d.x * w.x + d.y * w.y, d.y * w.x - d.x * w.y};  // d conj(w)
            v[k] = V{s.x - o.y, -(s.y + o.x)};                        // conj(s + i o): the inverse is conj(FFT(conj Z'))
        }
        __syncthreads();  // every partner is read before the second transform's exchanges reuse the tiles
        run_stages<V, P, 0, +1, 1, KG::PAD, KG::WAVE_LOCAL, KG::TWMODE, TWPOW, 1, 1, KG::NW, KG::LOCALX>(v, twr, lds, j, 0);
        if (valid) {
#pragma unroll
            for (int k = 0; k < E; ++k) sp[j + T * k] = V{v[k].x, -v[k].y};
        }
        __syncthreads();  // the next item's exchanges reuse the tiles
    }
}

template <class V, class P, bool VEC> hipError_t launch_lconv_cols(const LconvPass& F, bool fwd, hipStream_t stream) {
    using CG = LconvColsGeom<V, P>;
    using W = typename VecTraits<V>::W;
    using RT = typename real_of<V>::type;
    static std::atomic<int> blocks_per_cu[2][kMaxDevices];
    const void*             kern = fwd ? reinterpret_cast<const void*>(lconv_a_kernel<V, P, VEC>) : reinterpret_cast<const void*>(lconv_c_kernel<V, P, VEC>);
    hipError_t              e;
    const int               bpc = resident_blocks_per_cu(kern, CG::KG::THREADS, CG::LDS_BYTES, blocks_per_cu[fwd ? 0 : 1], &e);
    if (bpc == 0) return e;
    const long long per_row = (F.n2 + CG::CB - 1) / CG::CB, tiles = F.rows * per_row;
    if (tiles >= (1ll << 31)) return hipErrorInvalidValue;
    const long long grid = std::max(1ll, persistent_grid(device_info().cus, bpc, (tiles + CG::G - 1) / CG::G));
    (void)hipGetLastError();
    if (fwd)
        hipLaunchKernelGGL((lconv_a_kernel<V, P, VEC>), dim3((unsigned)grid), dim3(CG::KG::THREADS), CG::LDS_BYTES, stream, (const RT*)F.in, (V*)F.scr,
                           (const W*)F.tw, (const V*)F.hi, (const V*)F.lo, F.n, F.n2, (unsigned)tiles, (unsigned)per_row);
    else
        hipLaunchKernelGGL((lconv_c_kernel<V, P, VEC>), dim3((unsigned)grid), dim3(CG::KG::THREADS), CG::LDS_BYTES, stream, (const V*)F.scr, (RT*)F.out,
                           (const W*)F.tw, (const V*)F.hi, (const V*)F.lo, F.n, F.n2, (unsigned)tiles, (unsigned)per_row);
    return hipGetLastError();
}

template <class V, class P, bool HREAL> hipError_t launch_lconv_mid(const LconvPass& F, hipStream_t stream) {
    using MG = LconvMidGeom<V, P>;
    using W = typename VecTraits<V>::W;
    using HT = typename RconvFilter<V, HREAL>::T;
    auto                    kern = lconv_mid_kernel<V, P, HREAL>;
    static std::atomic<int> blocks_per_cu[kMaxDevices];
    hipError_t              e;
    const int               bpc = resident_blocks_per_cu(reinterpret_cast<const void*>(kern), MG::KG::THREADS, MG::LDS_BYTES, blocks_per_cu, &e);
    if (bpc == 0) return e;
    const long long items = F.rows * ((F.n1 + 1) / 2);
    if (items >= (1ll << 31)) return hipErrorInvalidValue;
    const long long grid = std::max(1ll, persistent_grid(device_info().cus, bpc, (items + MG::IPB - 1) / MG::IPB));
    (void)hipGetLastError();
    hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(MG::KG::THREADS), MG::LDS_BYTES, stream, (V*)F.scr, (const HT*)F.hp, (const W*)F.tw,
                       (const W*)F.rowc, (const W*)F.colt, (unsigned)items, F.n1, (unsigned)(F.row0 % F.channels), (unsigned)F.channels,
                       0.5 / (double)F.m);
    return hipGetLastError();
}

template <class V, int N> hipError_t lconv_run_typed(const LconvPass& F, hipStream_t stream) {
    using P = typename PlanFor<N>::type;
    if constexpr (lconv_factor(N) && lconv_fused_ok(N, sizeof(V) == 16)) {
        if (F.pass == LCONV_PASS_MID) {
            if constexpr (N > 64)  // N2 >= N1 >= 64 and N1 N2 > 4096: 64 is never the longer factor
                return F.filter_kind == RCONV_FILTER_REAL ? launch_lconv_mid<V, P, true>(F, stream) : launch_lconv_mid<V, P, false>(F, stream);
            return hipErrorInvalidValue;
        }
        const bool fwd = F.pass == LCONV_PASS_A;
        return F.vec ? launch_lconv_cols<V, P, true>(F, fwd, stream) : launch_lconv_cols<V, P, false>(F, fwd, stream);
    }
    return hipErrorInvalidValue;  // not built (lconv_factor, lconv_fused_ok): the dispatcher does not come here
}
template <int N> hipError_t LconvTag::run(const LconvPass& F, hipStream_t stream) {
    if (F.dtype == F64) return lconv_run_typed<double2, N>(F, stream);
    if (F.dtype == F32) return lconv_run_typed<float2, N>(F, stream);
    return hipErrorInvalidValue;
}
DFFT_FUSED_INSTANTIATE(LconvTag)

#else  // the dispatcher, the tables, the filter permutation and the multiply kernel of the composed route

// hp[c][k1 N2 + k2] = h[c][k1 + N1 k2], hp[c][M] = h[c][M]
template <class T>
__global__ void __launch_bounds__(256) lconv_filter_kernel(const T* __restrict__ h, T* __restrict__ hp, int N1, int N2, long long total) {
    const long long nb = (long long)N1 * N2 + 1;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
        const long long c = e / nb, i = e - c * nb;
        const long long k1 = i / N2, k2 = i - k1 * N2;
        hp[e] = h[c * nb + (i == nb - 1 ? i : k1 + N1 * k2)];
    }
}
// bins[r][k] *= H[(row0 + r) % channels][k] / m, k <= M, with H[k] at hp[(k % N1) N2 + k / N1] (k < M), hp[M]
template <class V, class HT>
__global__ void __launch_bounds__(256) lconv_mul_kernel(V* __restrict__ bins, const HT* __restrict__ hp, int N1, int N2, long long row0, long long channels,
                                                        long long total, double scale) {
    using RT = typename real_of<V>::type;
    const RT        sc = (RT)scale;
    const long long nb = (long long)N1 * N2 + 1;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
        const long long r = e / nb, k = e - r * nb;
        const long long k2 = k / N1, k1 = k - k2 * N1;
        const HT        hk = hp[((row0 + r) % channels) * nb + (k == nb - 1 ? k : k1 * N2 + k2)];
        const V         x = bins[e];
        if constexpr (sizeof(HT) == sizeof(V)) bins[e] = cmul(x, V{hk.x * sc, hk.y * sc});
        else bins[e] = V{x.x * (hk * sc), x.y * (hk * sc)};
    }
}

namespace {

// every accepted m in ascending order: twice the products of two factor lengths, 8192 < m <= 2^23
const std::vector<long long>& accepted_lengths() {
    static const std::vector<long long> v = [] {
        std::vector<long long> f, out;
        for (long long N = 64; N <= 2048; ++N)
            if (lconv_factor(N)) f.push_back(N);
        for (long long a : f)
            for (long long b : f)
                if (a <= b && 2 * a * b > 8192 && 2 * a * b <= (1ll << 23)) out.push_back(2 * a * b);
        std::sort(out.begin(), out.end());
        out.erase(std::unique(out.begin(), out.end()), out.end());
        return out;
    }();
    return v;
}

// the tables of one (device, m, dtype): built once, kept for the life of the process (about 100 KiB)
struct LconvTables {
    void *hi, *lo, *rowc, *colt;
};
std::mutex                                             g_mutex;
std::map<std::tuple<int, long long, int>, LconvTables> g_tables;

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

int lconv_tables(long long m, int n1, int n2, int dtype, LconvTables* out) {
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
    LconvTables     t{nullptr, nullptr, nullptr, nullptr};
    int             rc = upload_table((M + kLconvLo - 1) >> kLconvLoBits, kLconvLo, M, dtype, &t.hi);
    if (rc == DFFT_OK) rc = upload_table(kLconvLo, 1, M, dtype, &t.lo);
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

}  // namespace

bool lconv_split(long long m, int* n1, int* n2) {
    if (m <= 8192 || m > (1ll << 23) || (m & 1)) return false;
    const long long M = m / 2;
    int             best1 = 0, best2 = 0;
    for (long long a = 64; a * a <= M && a <= 2048; ++a) {
        if (M % a || !lconv_factor(a) || !lconv_factor(M / a)) continue;
        best1 = (int)a;
        best2 = (int)(M / a);
    }
    if (!best1) return false;
    if (n1) *n1 = best1;
    if (n2) *n2 = best2;
    return true;
}

long long lconv_length(long long at_least) {
    const std::vector<long long>& v = accepted_lengths();
    const auto                    it = std::lower_bound(v.begin(), v.end(), at_least);
    return it == v.end() ? 0 : *it;
}

bool lconv_fused_env() { return env_switch_on("DFFT_RCONV_LONG_FUSED"); }

bool lconv_fused(long long m, int dtype) {
    int n1 = 0, n2 = 0;
    if ((dtype != F64 && dtype != F32) || !lconv_split(m, &n1, &n2)) return false;
    return tuned_built<LconvTag>(n1, dtype == F64) && tuned_built<LconvTag>(n2, dtype == F64);
}

long long lconv_chunk_rows(long long m, int dtype, long long rows, size_t cap) { return chunk_units((size_t)(m / 2) * elem_bytes(dtype), rows, cap); }
size_t lconv_scratch_bytes(long long m, int dtype, long long rows, size_t cap) {
    if (rows < 1 || !lconv_split(m, nullptr, nullptr)) return 0;
    return (size_t)lconv_chunk_rows(m, dtype, rows, cap) * (size_t)(m / 2) * elem_bytes(dtype);
}

int lconv_run(const LconvLaunch& L, size_t cap, void* scratch, size_t scratch_bytes, hipStream_t stream) {
    int n1 = 0, n2 = 0;
    if (L.n < 1 || L.m < L.n || !lconv_split(L.m, &n1, &n2) || L.channels < 1 || L.batch < 1 || (L.dtype != F64 && L.dtype != F32) ||
        (L.filter_kind != RCONV_FILTER_COMPLEX && L.filter_kind != RCONV_FILTER_REAL) || !L.in || !L.out || !L.hp)
        return fail(DFFT_EINVAL, "lconv: bad arguments");
    if (!lconv_fused(L.m, L.dtype)) return fail(DFFT_EINVAL, "lconv: m = " + std::to_string(L.m) + " has no fused kernels");
    const long long rows = L.batch * L.channels;
    if (rows >= (1ll << 31)) return fail(DFFT_EINVAL, "lconv: 2^31 or more rows");
    const size_t rb = (size_t)(L.m / 2) * elem_bytes(L.dtype), rs = elem_bytes(L.dtype) / 2;
    const long long nr = fit_chunk_to_lease("lconv", lconv_chunk_rows(L.m, L.dtype, rows, cap), rb, scratch, scratch_bytes);
    if (nr < 1) return DFFT_EINVAL;
    LconvTables T;
    if (int rc = lconv_tables(L.m, n1, n2, L.dtype, &T)) return rc;
    LconvPass F;
    std::memset(&F, 0, sizeof(F));
    F.dtype = L.dtype;
    F.filter_kind = L.filter_kind;
    F.n = L.n;
    F.m = L.m;
    F.channels = L.channels;
    F.n1 = n1;
    F.n2 = n2;
    F.vec = rconv_vec(L.in, L.out, L.n, L.dtype);
    F.scr = scratch;
    F.hp = L.hp;
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
        F.in = (const char*)L.in + (size_t)r0 * L.n * rs;
        F.out = (char*)L.out + (size_t)r0 * L.n * rs;
        static const char* const names[3] = {"lconv (pass A): ", "lconv (mid): ", "lconv (pass C): "};
        for (int pass = 0; pass < 3; ++pass) {
            F.pass = pass;
            F.tw = pass == LCONV_PASS_MID ? tw2 : tw1;
            const hipError_t e = run_tuned<LconvTag>(pass == LCONV_PASS_MID ? n2 : n1, F, stream);
            if (e != hipSuccess) return fail(DFFT_EHIP, std::string(names[pass]) + hipGetErrorString(e));
        }
    }
    return DFFT_OK;
}

int lconv_filter(const void* h, void* hp, long long m, long long channels, int esize, hipStream_t stream) {
    int n1 = 0, n2 = 0;
    if (!h || !hp || channels < 1 || !lconv_split(m, &n1, &n2)) return fail(DFFT_EINVAL, "lconv_filter: bad arguments");
    const long long total = channels * (m / 2 + 1);
    (void)hipGetLastError();
    if (esize == 16) hipLaunchKernelGGL(lconv_filter_kernel<double2>, dim3(elementwise_grid(total)), dim3(256), 0, stream, (const double2*)h, (double2*)hp, n1, n2, total);
    else if (esize == 8) hipLaunchKernelGGL(lconv_filter_kernel<double>, dim3(elementwise_grid(total)), dim3(256), 0, stream, (const double*)h, (double*)hp, n1, n2, total);
    else if (esize == 4) hipLaunchKernelGGL(lconv_filter_kernel<float>, dim3(elementwise_grid(total)), dim3(256), 0, stream, (const float*)h, (float*)hp, n1, n2, total);
    else return fail(DFFT_EINVAL, "lconv_filter: bad element size");
    DFFT_HIP_TRY(hipGetLastError());
    return DFFT_OK;
}

int lconv_mul(void* bins, const void* hp, long long m, long long row0, long long channels, long long nr, int dtype, int filter_kind, hipStream_t stream) {
    int n1 = 0, n2 = 0;
    if (!lconv_split(m, &n1, &n2)) return fail(DFFT_EINVAL, "lconv_mul: bad arguments");
    const long long total = nr * (m / 2 + 1);
    const dim3      grid(elementwise_grid(total));
    const double    sc = 1.0 / (double)m;
    (void)hipGetLastError();
    if (dtype == F64 && filter_kind == RCONV_FILTER_REAL)
        hipLaunchKernelGGL((lconv_mul_kernel<double2, double>), grid, dim3(256), 0, stream, (double2*)bins, (const double*)hp, n1, n2, row0, channels, total, sc);
    else if (dtype == F64)
        hipLaunchKernelGGL((lconv_mul_kernel<double2, double2>), grid, dim3(256), 0, stream, (double2*)bins, (const double2*)hp, n1, n2, row0, channels, total, sc);
    else if (filter_kind == RCONV_FILTER_REAL)
        hipLaunchKernelGGL((lconv_mul_kernel<float2, float>), grid, dim3(256), 0, stream, (float2*)bins, (const float*)hp, n1, n2, row0, channels, total, sc);
    else
        hipLaunchKernelGGL((lconv_mul_kernel<float2, float2>), grid, dim3(256), 0, stream, (float2*)bins, (const float2*)hp, n1, n2, row0, channels, total, sc);
    DFFT_HIP_TRY(hipGetLastError());
    return DFFT_OK;
}

#endif

}  // namespace dfft
