// dfft_real_cols.hip -- real-to-complex / complex-to-real transforms along the middle axis of [batch][n][s] (s > 1) for ANY n with an
// n-point complex transform, by the two-for-one method of dfft_real_pair.hip applied to columns: real columns a = 2c and b = 2c + 1 of a
// row-major [n][s] matrix already sit in memory as one complex column z = a + i b, so one n-point complex transform down that column gives
// both spectra
//     A[k] = (Z[k] + conj Z[(n-k) mod n]) / 2,   B[k] = (Z[k] - conj Z[(n-k) mod n]) / (2i),   k = 0 .. n/2,
// and A goes to bin column 2c, B to bin column 2c + 1 -- a tile's output rows stay contiguous.  The inverse builds Z[k] = A[k] + i B[k]
// (k <= n/2) and conj A[n-k] + i conj B[n-k] (k > n/2) from the two bin columns -- the imaginary parts of bin 0 and, n even, bin n/2 taken
// as zero (numpy's rule) -- runs the inverse transform and stores Re into column 2c and Im into column 2c + 1.  An odd last column is
// paired with a zero column (forward) or its partner's output is dropped (backward): nothing outside the caller's columns is read or
// written.  The two columns of a pair share one transform, so each column's rounding error is bounded relative to the pair's combined
// magnitude, not its own (a column 1000x smaller than its partner keeps an error of about 1000 ulps of its own size).
//
// Forms:
//   * n with a tuned single-pass plan (dfft_plans.h), odd or even, and n * s < 2^31: ONE launch, r2c_pair_cols_kernel /
//     c2r_pair_cols_kernel -- tiles of CB adjacent complex (column-pair) columns of one batch item as the C2C column kernel has them
//     (cols_per_tile, kept to at most 128 KiB of exchange tile and 512 threads, so the tile holds all n points of its columns in natural
//     order), run_stages (dfft_fft_impl.h); R2C puts Z into the tile in natural order and after one barrier the thread holding Z[k] stores
//     A[k] for k <= n/2 and B[n-k] for k > n/2.  Where s is even and the real side is aligned to a complex element, a column pair is
//     loaded (R2C) / stored (C2R) as one complex value, otherwise as two reals.  Per-point offsets are 32-bit within a batch item.
//     No instantiation keeps anything in scratch memory (rc_cols_per_tile; profiles/r11/kernel_resources.txt, which
//     tests/test_real_strided_host.py pins).  A few tuned lengths run the multi-pass form because it measured faster (multi_pass_faster).
//   * every other n (the run-time-scheduled single-pass lengths, four-step lengths, Bluestein lengths, multi_pass_faster, n * s >=
//     2^31), per batch chunk of at most max(256 MiB, one item's) packed pairs: R2C -- pack (or, s even and `in` aligned, nothing: `in`
//     already is the complex matrix [batch][n][s/2]), the n-point transform down the columns (the C2C column launch, long_fft or
//     bluestein_fft) into scratch, split into `out`; C2R -- merge into scratch, the inverse transform (straight into `out` viewed as
//     complex where s is even and `out` aligned), unpack otherwise.
//
// Compiled once per instantiation group (-DDFFT_INST_GROUP=g: the fused kernels of the tuned lengths of group g) and once with
// -DDFFT_INST_GROUP=DFFT_NUM_INST_GROUPS (the dispatcher and the pack / split / merge / unpack kernels).
#include "dfft_fused_host.h"
#include "dfft_bluestein.h"
#include "dfft_long.h"
#include "dfft_real_cols.h"

#include <algorithm>
#include <atomic>
#include <cstring>

#ifndef DFFT_INST_GROUP
#error "compile with -DDFFT_INST_GROUP=<g>"
#endif

namespace dfft {

struct ColsFusedLaunch {
    int         dtype;
    int         dir;
    long long   s, batch;
    bool        vec;  // s even and the real side aligned to a complex element: a column pair is one complex load / store
    const void* in;
    void*       out;
    const void* tw;
};

// the family (dfft_fused_host.h): every tuned length is built; run<N>: defined in the translation unit of N's group only
struct ColsTag {
    using Launch = ColsFusedLaunch;
    static constexpr bool ok(int) { return true; }
    template <int N> static hipError_t run(const Launch& F, hipStream_t stream);
};

#if DFFT_INST_GROUP < DFFT_NUM_INST_GROUPS

// Column tiles: the C2C column kernel's width (cols_per_tile), halved until the tile holds at most 128 KiB -- the split step needs all
// n points of its columns in the exchange tile at once, so no two-phase tiles -- and the workgroup at most 512 threads (at 1024, 44 of the
// 400 instantiations kept values in scratch memory), 256 for the ones that kept 24 ... 464 bytes per lane in scratch at 512
template <class V, class P> constexpr int rc_max_threads() {
    constexpr bool f64 = sizeof(V) == 16;
    constexpr int  N = P::N;
    if (f64 ? (N == 1024 || N == 4096) : (N == 400 || N == 640 || N == 1280 || N == 1536 || N == 3125 || N == 4096)) return 256;
    return 512;
}
template <class V, class P> constexpr int rc_cols_per_tile() {
    int cb = cols_per_tile<V, P>();
    while (cb > 1 && ((long long)P::N * cb * (long long)sizeof(V) > 128 * 1024 || cb * P::T > rc_max_threads<V, P>())) cb /= 2;
    return cb;
}

template <class V, class P> struct ColsGeom {
    static constexpr int CB = rc_cols_per_tile<V, P>();
    static constexpr int G = ConstMax1<256 / (CB * P::T)>::value;
    using KG = KernelGeom<V, P, CB, G, TuneDefault>;
    static_assert(KG::PH == 1, "the split step needs the whole tile in the LDS");
    static constexpr int SPLIT = (KG::PAD ? P::N + P::N / 8 : P::N) * CB;  // > lds_index<CB, PAD>(N - 1, CB - 1)
    static constexpr int EXR = ((KG::LDS_ELEMS > SPLIT ? KG::LDS_ELEMS : SPLIT) + 1) / 2 * 2;
    static constexpr size_t LDS_BYTES = (size_t)EXR * G * sizeof(V) + KG::TW_BYTES;
};

// XCD-aware tile order for tiles narrower than a 128-byte line, exactly as fft_tiles_kernel has it (dfft_fft_impl.h, map_tile): the Q
// tiles that share the lines of one row segment go to workgroups Q consecutive slots apart on the SAME XCD (workgroup b runs on XCD
// b % 8; used for speed only, any placement gives the same result), so the rest of every line is served by that XCD's L2 instead of
// being fetched again by another XCD.  A permutation of [0, remap_full); on only where a batch item's tile count is a multiple of Q.
// (fp32 only: with it the 2048-point fp64 C2R kernels keep 8-12 bytes per lane in scratch, and the fp64 sub-line tiles measured
// 0.77-0.94 of the widened route without it)
template <class V, int CB, int G> constexpr int cols_line_share() {
    return (sizeof(V) == 8 && CB > 1 && G == 1 && CB * (int)sizeof(V) < 128) ? 128 / (CB * (int)sizeof(V)) : 1;
}
template <class V, int CB, int G> __device__ __forceinline__ unsigned cols_remap_full(unsigned tiles, unsigned tiles_per_b) {
    constexpr unsigned Q = cols_line_share<V, CB, G>();
    return (Q > 1 && tiles_per_b % Q == 0) ? (tiles / (8u * Q)) * (8u * Q) : 0u;
}
template <class V, int CB, int G> __device__ __forceinline__ unsigned cols_map_tile(unsigned lin, unsigned remap_full) {
    constexpr unsigned Q = cols_line_share<V, CB, G>();
    if constexpr (Q > 1) {
        if (lin < remap_full) {
            const unsigned xcd = lin & 7u, s = lin >> 3;
            return ((s / Q) * 8u + xcd) * Q + (s % Q);
        }
    }
    return lin;
}

// R2C: reals [batch][N][s] -> bins [batch][N/2 + 1][s].  Tile t = (batch item b, block of CB column pairs); VEC: s even and `in` aligned
// to V, so column pair pc is the complex element pc of a row of s/2.
template <class V, class P, bool VEC>
__global__ void __attribute__((amdgpu_flat_work_group_size(1, ColsGeom<V, P>::KG::THREADS)))
r2c_pair_cols_kernel(const typename real_of<V>::type* __restrict__ in, V* __restrict__ out, const typename VecTraits<V>::W* __restrict__ tw,
                     long long s, unsigned tiles, unsigned tiles_per_b) {
    using CG = ColsGeom<V, P>;
    using KG = typename CG::KG;
    using W = typename VecTraits<V>::W;
    using RT = typename real_of<V>::type;
    constexpr int  E = P::E, T = P::T, N = P::N, NH = N / 2 + 1, G = CG::G, GT = KG::GT, CB = CG::CB;
    constexpr bool TWPOW = KG::TWMODE == TW_REG;
    extern __shared__ __attribute__((aligned(16))) char dfft_smem[];
    const int g = threadIdx.x / GT;
    const int tid = (int)threadIdx.x - g * GT;
    const int c = tid % CB;
    const int j = tile_j<CB, KG::NW>(tid);
    V*        lds = reinterpret_cast<V*>(dfft_smem + KG::TW_BYTES) + g * CG::EXR;
    W         twreg[KG::TWMODE == TW_REG && KG::TWN > 0 ? KG::TWN : 1];
    const W*  twr = stage_twiddles<V, P, +1, KG>(twreg, reinterpret_cast<W*>(dfft_smem), tw, j);
    const RT  half = (RT)0.5;
    const long long sp = (s + 1) / 2;
    const unsigned  us = (unsigned)s;
    const unsigned  remap_full = cols_remap_full<V, CB, G>(tiles, tiles_per_b);
    for (unsigned r0 = blockIdx.x * G; r0 < tiles; r0 += gridDim.x * G) {
        const unsigned  t = cols_map_tile<V, CB, G>(r0 + g, remap_full);
        const unsigned  b = t < tiles ? t / tiles_per_b : 0u, cb = t < tiles ? t - b * tiles_per_b : 0u;
        const long long pc = (long long)cb * CB + c;
        const bool      va = t < tiles && pc < sp, vb = va && 2 * pc + 1 < s;
        // per-point offsets in 32 bits from the column's base pointer (N * s < 2^31, checked on the host)
        V v[E];
        if constexpr (VEC) {
            const V*       ip = reinterpret_cast<const V*>(in) + (long long)b * N * (s / 2) + (va ? pc : 0);
            const unsigned uh = (unsigned)(s / 2);
#pragma unroll
            for (int k = 0; k < E; ++k) v[k] = va ? ip[(unsigned)(j + T * k) * uh] : V{0, 0};
        } else {
            const RT* ip = in + (long long)b * N * s + (va ? 2 * pc : 0);
#pragma unroll
            for (int k = 0; k < E; ++k) {
                const unsigned o = (unsigned)(j + T * k) * us;
                v[k] = V{va ? ip[o] : (RT)0, vb ? ip[o + 1] : (RT)0};
            }
        }
        run_stages<V, P, 0, +1, CB, KG::PAD, KG::WAVE_LOCAL, KG::TWMODE, TWPOW, KG::PH, 1, KG::NW, KG::LOCALX>(v, twr, lds, j, c);
        group_sync<KG::WAVE_LOCAL>();
#pragma unroll
        for (int k = 0; k < E; ++k) lds[lds_index<CB, KG::PAD>(j + T * k, c)] = v[k];
        group_sync<KG::WAVE_LOCAL>();
        if (va) {
            V* op = out + (long long)b * NH * s + 2 * pc;
#pragma unroll
            for (int k = 0; k < E; ++k) {
                const int kk = j + T * k, km = kk == 0 ? 0 : N - kk;
                const V   zm = lds[lds_index<CB, KG::PAD>(km, c)];
                if (2 * kk <= N) {  // A[kk] (and B[kk] for the self-paired bins 0 and n/2)
                    op[(unsigned)kk * us] = V{(v[k].x + zm.x) * half, (v[k].y - zm.y) * half};
                    if (vb && (kk == 0 || 2 * kk == N)) op[(unsigned)kk * us + 1] = V{(v[k].y + zm.y) * half, (zm.x - v[k].x) * half};
                } else if (vb) {  // B[n - kk] from Z[n - kk] = zm and its partner Z[kk]
                    op[(unsigned)km * us + 1] = V{(zm.y + v[k].y) * half, (v[k].x - zm.x) * half};
                }
            }
        }
        group_sync<KG::WAVE_LOCAL>();  // the next tile's exchanges reuse the tile
    }
}

// C2R: bins [batch][N/2 + 1][s] -> reals [batch][N][s].  VEC: s even and `out` aligned to V, so column pair pc is stored as one complex
// element.
template <class V, class P, bool VEC>
__global__ void __attribute__((amdgpu_flat_work_group_size(1, ColsGeom<V, P>::KG::THREADS)))
c2r_pair_cols_kernel(const V* __restrict__ in, typename real_of<V>::type* __restrict__ out, const typename VecTraits<V>::W* __restrict__ tw,
                     long long s, unsigned tiles, unsigned tiles_per_b) {
    using CG = ColsGeom<V, P>;
    using KG = typename CG::KG;
    using W = typename VecTraits<V>::W;
    using RT = typename real_of<V>::type;
    constexpr int  E = P::E, T = P::T, N = P::N, NH = N / 2 + 1, G = CG::G, GT = KG::GT, CB = CG::CB;
    constexpr bool TWPOW = KG::TWMODE == TW_REG;
    extern __shared__ __attribute__((aligned(16))) char dfft_smem[];
    const int g = threadIdx.x / GT;
    const int tid = (int)threadIdx.x - g * GT;
    const int c = tid % CB;
    const int j = tile_j<CB, KG::NW>(tid);
    V*        lds = reinterpret_cast<V*>(dfft_smem + KG::TW_BYTES) + g * CG::EXR;
    W         twreg[KG::TWMODE == TW_REG && KG::TWN > 0 ? KG::TWN : 1];
    const W*  twr = stage_twiddles<V, P, -1, KG>(twreg, reinterpret_cast<W*>(dfft_smem), tw, j);
    const long long sp = (s + 1) / 2;
    const unsigned  us = (unsigned)s;
    const unsigned  remap_full = cols_remap_full<V, CB, G>(tiles, tiles_per_b);
    for (unsigned r0 = blockIdx.x * G; r0 < tiles; r0 += gridDim.x * G) {
        const unsigned  t = cols_map_tile<V, CB, G>(r0 + g, remap_full);
        const unsigned  b = t < tiles ? t / tiles_per_b : 0u, cb = t < tiles ? t - b * tiles_per_b : 0u;
        const long long pc = (long long)cb * CB + c;
        const bool      va = t < tiles && pc < sp, vb = va && 2 * pc + 1 < s;
        const V*        ip = in + (long long)b * NH * s + (va ? 2 * pc : 0);
        V               v[E];
#pragma unroll
        for (int k = 0; k < E; ++k) {
            const int  kk = j + T * k;
            const bool lo = 2 * kk <= N;
            const int  m = lo ? kk : N - kk;
            V          a = va ? ip[(unsigned)m * us] : V{0, 0};
            V          bb = vb ? ip[(unsigned)m * us + 1] : V{0, 0};
            if (m == 0 || 2 * m == N) {  // the imaginary parts of the DC and Nyquist bins are ignored
                a.y = (RT)0;
                bb.y = (RT)0;
            }
            v[k] = lo ? V{a.x - bb.y, a.y + bb.x} : V{a.x + bb.y, bb.x - a.y};  // A + i B, or conj A + i conj B
        }
        group_sync<KG::WAVE_LOCAL>();  // the previous tile's stages are done with the tile
        run_stages<V, P, 0, -1, CB, KG::PAD, KG::WAVE_LOCAL, KG::TWMODE, TWPOW, KG::PH, 1, KG::NW, KG::LOCALX>(v, twr, lds, j, c);
        if (va) {
            if constexpr (VEC) {
                V*             op = reinterpret_cast<V*>(out) + (long long)b * N * (s / 2) + pc;
                const unsigned uh = (unsigned)(s / 2);
#pragma unroll
                for (int k = 0; k < E; ++k) op[(unsigned)(j + T * k) * uh] = v[k];
            } else {
                RT* op = out + (long long)b * N * s + 2 * pc;
#pragma unroll
                for (int k = 0; k < E; ++k) {
                    const unsigned o = (unsigned)(j + T * k) * us;
                    op[o] = v[k].x;
                    if (vb) op[o + 1] = v[k].y;
                }
            }
        }
    }
}

template <class V, class P, bool VEC> const void* cols_kernel(bool fwd) {
    return fwd ? reinterpret_cast<const void*>(r2c_pair_cols_kernel<V, P, VEC>) : reinterpret_cast<const void*>(c2r_pair_cols_kernel<V, P, VEC>);
}

template <class V, class P> hipError_t launch_cols_plan(const ColsFusedLaunch& F, bool fwd, hipStream_t stream) {
    using CG = ColsGeom<V, P>;
    using W = typename VecTraits<V>::W;
    using RT = typename real_of<V>::type;
    constexpr int           N = P::N, NH = N / 2 + 1;
    static std::atomic<int> blocks_per_cu[2][2][kMaxDevices];  // per kernel: direction, VEC
    const void*             kern = F.vec ? cols_kernel<V, P, true>(fwd) : cols_kernel<V, P, false>(fwd);
    hipError_t              e;
    const int               bpc = resident_blocks_per_cu(kern, CG::KG::THREADS, CG::LDS_BYTES, blocks_per_cu[fwd ? 0 : 1][F.vec ? 1 : 0], &e);
    if (bpc == 0) return e;
    const long long per_b = ((F.s + 1) / 2 + CG::CB - 1) / CG::CB;
    const long long max_b = std::max(1ll, ((1ll << 31) - 1) / per_b);  // tile indices stay below 2^31 per launch
    const long long rstep = (long long)N * F.s, cstep = (long long)NH * F.s;
    (void)hipGetLastError();
    for (long long b0 = 0; b0 < F.batch; b0 += max_b) {
        const long long nb = std::min(max_b, F.batch - b0), tiles = nb * per_b;
        const long long grid = std::max(1ll, persistent_grid(device_info().cus, bpc, (tiles + CG::G - 1) / CG::G));
        if (fwd) {
            const RT* ip = (const RT*)F.in + b0 * rstep;
            V*        op = (V*)F.out + b0 * cstep;
            if (F.vec)
                hipLaunchKernelGGL((r2c_pair_cols_kernel<V, P, true>), dim3((unsigned)grid), dim3(CG::KG::THREADS), CG::LDS_BYTES, stream, ip, op,
                                   (const W*)F.tw, F.s, (unsigned)tiles, (unsigned)per_b);
            else
                hipLaunchKernelGGL((r2c_pair_cols_kernel<V, P, false>), dim3((unsigned)grid), dim3(CG::KG::THREADS), CG::LDS_BYTES, stream, ip, op,
                                   (const W*)F.tw, F.s, (unsigned)tiles, (unsigned)per_b);
        } else {
            const V* ip = (const V*)F.in + b0 * cstep;
            RT*      op = (RT*)F.out + b0 * rstep;
            if (F.vec)
                hipLaunchKernelGGL((c2r_pair_cols_kernel<V, P, true>), dim3((unsigned)grid), dim3(CG::KG::THREADS), CG::LDS_BYTES, stream, ip, op,
                                   (const W*)F.tw, F.s, (unsigned)tiles, (unsigned)per_b);
            else
                hipLaunchKernelGGL((c2r_pair_cols_kernel<V, P, false>), dim3((unsigned)grid), dim3(CG::KG::THREADS), CG::LDS_BYTES, stream, ip, op,
                                   (const W*)F.tw, F.s, (unsigned)tiles, (unsigned)per_b);
        }
        e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

template <int N> hipError_t ColsTag::run(const ColsFusedLaunch& F, hipStream_t stream) {
    if (F.dtype == F64) return launch_cols_plan<double2, typename PlanFor<N>::type>(F, F.dir > 0, stream);
    if (F.dtype == F32) return launch_cols_plan<float2, typename PlanFor<N>::type>(F, F.dir > 0, stream);
    return hipErrorInvalidValue;
}
DFFT_FUSED_INSTANTIATE(ColsTag)

#else  // the dispatcher, and the kernels of the multi-pass form

// z[b][k][pc] = a + i b for the real columns a = 2pc, b = 2pc + 1 (a zero column past s) of in[b][k][s]   (e runs over nb * n * sp)
template <class V>
__global__ void __launch_bounds__(256) r2c_cols_pack_kernel(const typename real_of<V>::type* __restrict__ in, V* __restrict__ z, long long s,
                                                            long long sp, long long total) {
    using RT = typename real_of<V>::type;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
        const long long r = e / sp, pc = e - r * sp;  // r = b * n + k
        const RT*       ip = in + r * s + 2 * pc;
        z[e] = V{ip[0], 2 * pc + 1 < s ? ip[1] : (RT)0};
    }
}

// A[m] -> out[b][m][2pc], B[m] -> out[b][m][2pc + 1] (dropped past s), m <= n/2, from z[b][n][sp]   (e runs over nb * (n/2 + 1) * sp)
template <class V>
__global__ void __launch_bounds__(256) r2c_cols_split_kernel(const V* __restrict__ z, V* __restrict__ out, long long n, long long s, long long sp,
                                                             long long total) {
    using RT = typename real_of<V>::type;
    const long long nh = n / 2 + 1;
    const RT        half = (RT)0.5;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
        const long long r = e / sp, pc = e - r * sp;  // r = b * nh + m
        const long long b = r / nh, m = r - b * nh;
        const V         zk = z[(b * n + m) * sp + pc], zm = z[(b * n + (m == 0 ? 0 : n - m)) * sp + pc];
        V*              op = out + r * s + 2 * pc;
        op[0] = V{(zk.x + zm.x) * half, (zk.y - zm.y) * half};
        if (2 * pc + 1 < s) op[1] = V{(zk.y + zm.y) * half, (zm.x - zk.x) * half};
    }
}

// z[b][k][pc] from the bin columns 2pc, 2pc + 1 of in[b][n/2 + 1][s] (conjugates above n/2; imaginary parts of bins 0 and n/2 ignored)
// (e runs over nb * n * sp)
template <class V>
__global__ void __launch_bounds__(256) c2r_cols_merge_kernel(const V* __restrict__ in, V* __restrict__ z, long long n, long long s, long long sp,
                                                             long long total) {
    using RT = typename real_of<V>::type;
    const long long nh = n / 2 + 1;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
        const long long r = e / sp, pc = e - r * sp;  // r = b * n + k
        const long long b = r / n, k = r - b * n;
        const bool      lo = 2 * k <= n;
        const long long m = lo ? k : n - k;
        const V*        ip = in + (b * nh + m) * s + 2 * pc;
        V               a = ip[0];
        V               bb = 2 * pc + 1 < s ? ip[1] : V{0, 0};
        if (m == 0 || 2 * m == n) {
            a.y = (RT)0;
            bb.y = (RT)0;
        }
        z[e] = lo ? V{a.x - bb.y, a.y + bb.x} : V{a.x + bb.y, bb.x - a.y};
    }
}

// out[b][k][2pc] = Re z, out[b][k][2pc + 1] = Im z (dropped past s)   (e runs over nb * n * sp)
template <class V>
__global__ void __launch_bounds__(256) c2r_cols_unpack_kernel(const V* __restrict__ z, typename real_of<V>::type* __restrict__ out, long long s,
                                                              long long sp, long long total) {
    using RT = typename real_of<V>::type;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
        const long long r = e / sp, pc = e - r * sp;
        const V         v = z[e];
        RT*             op = out + r * s + 2 * pc;
        op[0] = v.x;
        if (2 * pc + 1 < s) op[1] = v.y;
    }
}

namespace {

bool tuned_length(long long n) { return tuned_built<ColsTag>(n); }

// batch items per chunk of the multi-pass form (their packed pairs within max(256 MiB, one item's)), and the scratch such a chunk needs
long long chunk_items(long long n, long long sp, int dtype, long long batch, size_t cap) {
    const size_t zb = (size_t)n * sp * elem_bytes(dtype);
    return chunk_units(zb, batch, cap);
}
size_t chunk_bytes(long long n, long long sp, int dtype, long long nb, const BluesteinTables* T, bool bs_fused, size_t cap) {
    const size_t zb = (size_t)nb * n * sp * elem_bytes(dtype);
    if (T) return zb + bluestein_scratch_bytes(*T, sp, nb, bs_fused, cap);
    return n > 4096 ? 2 * zb : zb;  // four-step: long_fft's scratch as large as its data
}

// n-point transforms down the sp columns of the nb items of zin [nb][n][sp] into zout (in == out allowed)
int cols_fft(const void* zin, void* zout, long long sp, long long nb, const RealColsLaunch& L, const BluesteinTables* T, bool bs_fused,
             void* inner, size_t inner_bytes, hipStream_t stream) {
    if (T) return bluestein_fft(*T, zin, zout, sp, nb, 1.0, bs_fused, inner, inner_bytes, stream);
    if (L.n > 4096) return long_fft(zin, zout, L.n, sp, nb, L.dtype, L.dir, 1.0, inner, stream);
    // single-pass lengths: the entry points' own launches (they take no scratch for n <= 4096)
    return sp == 1 ? dfft_fft1d_rows(const_cast<void*>(zin), zout, L.n, nb, L.dtype, L.dir, stream)
                   : dfft_fft1d_cols(const_cast<void*>(zin), zout, L.n, sp, nb, L.dtype, L.dir, stream);
}

template <class V>
int cols_chunk(const RealColsLaunch& L, long long b0, long long nb, const BluesteinTables* T, bool bs_fused, void* z, void* inner,
               size_t inner_bytes, hipStream_t stream) {
    using RT = typename real_of<V>::type;
    const long long n = L.n, s = L.s, sp = (s + 1) / 2, nh = n / 2 + 1;
    const long long tz = nb * n * sp, tb = nb * nh * sp;
    (void)hipGetLastError();
    if (L.dir > 0) {
        const RT* in = (const RT*)L.in + b0 * n * s;
        V*        out = (V*)L.out + b0 * nh * s;
        if (s % 2 == 0 && (uintptr_t)L.in % sizeof(V) == 0) {  // `in` already is the packed complex matrix [nb][n][s/2]
            if (int rc = cols_fft(in, z, sp, nb, L, T, bs_fused, inner, inner_bytes, stream)) return rc;
        } else {
            hipLaunchKernelGGL(r2c_cols_pack_kernel<V>, dim3(elementwise_grid(tz)), dim3(256), 0, stream, in, (V*)z, s, sp, tz);
            DFFT_HIP_TRY(hipGetLastError());
            if (int rc = cols_fft(z, z, sp, nb, L, T, bs_fused, inner, inner_bytes, stream)) return rc;
        }
        hipLaunchKernelGGL(r2c_cols_split_kernel<V>, dim3(elementwise_grid(tb)), dim3(256), 0, stream, (const V*)z, out, n, s, sp, tb);
        DFFT_HIP_TRY(hipGetLastError());
    } else {
        const V* in = (const V*)L.in + b0 * nh * s;
        RT*      out = (RT*)L.out + b0 * n * s;
        hipLaunchKernelGGL(c2r_cols_merge_kernel<V>, dim3(elementwise_grid(tz)), dim3(256), 0, stream, in, (V*)z, n, s, sp, tz);
        DFFT_HIP_TRY(hipGetLastError());
        if (s % 2 == 0 && (uintptr_t)L.out % sizeof(V) == 0) {  // `out` viewed as complex [nb][n][s/2]
            if (int rc = cols_fft(z, out, sp, nb, L, T, bs_fused, inner, inner_bytes, stream)) return rc;
        } else {
            if (int rc = cols_fft(z, z, sp, nb, L, T, bs_fused, inner, inner_bytes, stream)) return rc;
            hipLaunchKernelGGL(c2r_cols_unpack_kernel<V>, dim3(elementwise_grid(tz)), dim3(256), 0, stream, (const V*)z, out, s, sp, tz);
            DFFT_HIP_TRY(hipGetLastError());
        }
    }
    return DFFT_OK;
}

}  // namespace

// Tuned lengths that run the multi-pass form although they have fused kernels, because it measured faster (real / widened-complex time,
// profiles/r11/README.md): their fused tiles hold one column pair or row segments of 8-16 bytes, where the C2C column kernel behind the
// multi-pass form reads full or half lines -- fp64 2401 and 4096 (fused 1.05-1.32, multi-pass 0.72-1.08); fp32 2187, 2401, 3125 and 4096
// (fused 0.75-2.11, multi-pass 0.65-0.84).  fp32 2048 (32-byte fused segments, 64-byte C2C ones) goes multi-pass where the C2C column
// kernel's XCD-aware tile order is on, i.e. its 8-column tiles per row are even in number (s = 512: fused 1.05-1.07, multi-pass 0.95-0.99;
// s = 1000: fused 0.83-0.93, multi-pass 0.95-1.01).
static bool multi_pass_faster(long long n, long long s, int dtype) {
    if (dtype == F64) return n == 2401 || n == 4096;
    if (n == 2187 || n == 2401 || n == 3125 || n == 4096) return true;
    return n == 2048 && ((s + 1) / 2 + 7) / 8 % 2 == 0;
}

bool real_cols_fused(long long n, long long s, int dtype) {
    return tuned_length(n) && s >= 1 && n * s < (1ll << 31) && !multi_pass_faster(n, s, dtype);
}

size_t real_cols_scratch_bytes(long long n, long long s, long long batch, int dtype, const BluesteinTables* T, bool bluestein_fused, size_t cap) {
    if (n < 1 || s < 1 || batch <= 0 || real_cols_fused(n, s, dtype)) return 0;
    const long long sp = (s + 1) / 2;
    return chunk_bytes(n, sp, dtype, chunk_items(n, sp, dtype, batch, cap), T, bluestein_fused, cap);
}

int real_cols(const RealColsLaunch& L, const BluesteinTables* T, bool bluestein_fused, size_t cap, void* scratch, size_t scratch_bytes, hipStream_t stream) {
    if (L.n < 1 || L.s < 1 || L.batch < 0 || (L.dir != 1 && L.dir != -1) || (L.dtype != F64 && L.dtype != F32) || !L.in || !L.out)
        return fail(DFFT_EINVAL, "real columns: bad arguments");
    if (L.batch == 0) return DFFT_OK;
    if (T && (T->n != L.n || T->dtype != L.dtype || T->dir != L.dir)) return fail(DFFT_EINVAL, "real columns: Bluestein tables of another transform");
    if (real_cols_fused(L.n, L.s, L.dtype)) {
        ColsFusedLaunch F;
        std::memset(&F, 0, sizeof(F));
        F.dtype = L.dtype;
        F.dir = L.dir;
        F.s = L.s;
        F.batch = L.batch;
        F.in = L.in;
        F.out = L.out;
        F.vec = L.s % 2 == 0 && (uintptr_t)(L.dir > 0 ? L.in : L.out) % elem_bytes(L.dtype) == 0;
        if (int rc = get_twiddles((int)L.n, L.dtype, &F.tw)) return rc;
        const hipError_t e = run_tuned<ColsTag>(L.n, F, stream);
        if (e == hipSuccess) return DFFT_OK;
        return fail(DFFT_EHIP, std::string(L.dir > 0 ? "R2C pair columns: " : "C2R pair columns: ") + hipGetErrorString(e));
    }
    if (!T && L.n > 4096) {
        int a, b;
        if (!long_split(L.n, &a, &b)) return fail(DFFT_EINVAL, "real columns: length " + std::to_string(L.n) + " needs Bluestein tables");
    }
    // batch chunks whose packed pairs and transform scratch fit the scratch buffer
    const long long sp = (L.s + 1) / 2;
    long long       nb = chunk_items(L.n, sp, L.dtype, L.batch, cap);
    while (nb > 1 && chunk_bytes(L.n, sp, L.dtype, nb, T, bluestein_fused, cap) > scratch_bytes) nb = (nb + 1) / 2;
    if (!scratch || chunk_bytes(L.n, sp, L.dtype, nb, T, bluestein_fused, cap) > scratch_bytes) return fail(DFFT_EINVAL, "real columns: scratch buffer too small");
    const size_t zb = (size_t)nb * L.n * sp * elem_bytes(L.dtype);
    void*        inner = (char*)scratch + zb;
    const size_t inner_bytes = scratch_bytes - zb;
    for (long long b0 = 0; b0 < L.batch; b0 += nb) {
        const long long m = std::min(nb, L.batch - b0);
        const int       rc = L.dtype == F64 ? cols_chunk<double2>(L, b0, m, T, bluestein_fused, scratch, inner, inner_bytes, stream)
                                            : cols_chunk<float2>(L, b0, m, T, bluestein_fused, scratch, inner, inner_bytes, stream);
        if (rc) return rc;
    }
    return DFFT_OK;
}

#endif

}  // namespace dfft
