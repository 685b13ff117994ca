// dfft_osconv.hip -- overlap-save 1-D real FFT convolution: rows of reals [batch][channels][n] of ANY length filtered block by block
// with the spectra H [channels][m/2 + 1] of a block length m = 2 M (M a single-pass length, real form 1, m <= 8192).  With d the samples
// dropped per block (0 <= d < m), S = m - d and nb = ceil(n_out / S), block b of row r is
//     xb[i] = x[r][b S - d + i]  (0 where b S - d + i is outside [0, n)),   cb = irfft(rfft(xb, m) * H[r % channels], m),
//     y[r][b S + j] = cb[d + j]   (0 <= j < S, b S + j < n_out),
// which for H = rfft of taps <= d + 1 zero-padded taps is numpy.convolve(x[r], k)[:n_out].  Four-step and Bluestein halves (taps about
// n beyond 8192) are not built.
//
// Fused form, osconv_blocks_kernel (M with a tuned plan, osconv_fused_ok): ONE launch, the persistent loop of rconv_rows_kernel
// (dfft_rconv.hip) over the items it = row * nb + b, one item per thread group.  The arithmetic between load and store is that
// kernel's (run_stages, the pairing / multiply / merge step, run_stages; geometry and filter types of dfft_rconv_impl.h); what changes is the load base row * n + b S - d, bounded
// to the row -- a block at the start of a row reads zeros, not the end of the row before it --, the store window i in [d, m) with
// b S + i - d < n_out at row * n_out + b S + i - d, and the filter row, taken from the item's row.  The padded blocks, the dropped
// samples and the spectrum exist in registers and LDS only.  The input position b S - d + i and the output position b S + (i - d) of
// real i are the same number s0 + i, so a 64-bit base and a 32-bit window per side -- [lo, hi) for loads, [d, he) for stores -- serve an
// item.  The item is decoded (row = it / nb, b = it % nb) three times, for the loads, the filter row and the stores, each time from a
// copy of `it` the compiler cannot trace back: held across the transforms, the store base and window cost the 24-point fp64 kernels
// (M = 48 ... 384) up to 244 bytes of scratch per lane; a division per item costs nothing against the butterflies.
//
// Where n, n_out and d are even and both pointers are aligned to two reals (VEC) every complex value z[j] = (x[2j], x[2j+1]) lies
// wholly inside or outside each window and moves as one two-real value; otherwise real by real (with d odd an output pair straddles
// two complex values).  There is no in-place form: a block reads d samples that its left neighbour's store window covers.
//
// Composed form (every other accepted M, the instantiations osconv_fused_ok leaves out, DFFT_RCONV_FUSED=0): per chunk of items of at
// most max(256 MiB, one item's) scratch -- osconv_gather_kernel into zero-filled blocks, launch_real_rows forward, osconv_mul_kernel
// (H / m, in place on the bins, the channel from the item's row), launch_real_rows backward, osconv_scatter_kernel into `out`.
//
// Compiled once per instantiation group (-DDFFT_INST_GROUP=g: the fused kernels of the tuned lengths of group g) and once with
// -DDFFT_INST_GROUP=DFFT_NUM_INST_GROUPS (the dispatcher, the block chooser and the kernels of the composed form).
#include "dfft_fused_host.h"
#include "dfft_osconv.h"
#include "dfft_rconv.h"

#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <cstring>

#ifndef DFFT_INST_GROUP
#error "compile with -DDFFT_INST_GROUP=<g>"
#endif

namespace dfft {

// One fused launch
struct OsconvFusedLaunch {
    int         dtype, filter_kind;
    long long   n, n_out, m, discard, channels, items, nb;
    bool        vec;
    const void* in;
    void*       out;
    const void* h;
    const void* tw;   // e^{-2 pi i k / M}
    const void* twh;  // e^{-2 pi i k / m}
};

// (M, dtype) whose block kernels would keep values in scratch memory (tools/fused_resources.py osconv, profiles/2026-10-20_rconv1d_os/
// kernel_resources.txt) are not built: they run the composed form.  The first two lines are rconv_fused_ok's (dfft_rconv.hip), whose
// rule the dispatcher applies through rconv_fused as well.
constexpr bool osconv_fused_ok(int M, bool f64) {
    if (M == 3125) return false;
    if (M == 1536 && f64) return false;
    if (M == 2401 && !f64) return false;  // 7 points per thread on 343 threads: 8 ... 44 bytes per lane in fp32, either access width (none in fp64)
    return true;
}

// the family (dfft_fused_host.h); run<M>: defined in the translation unit of M's group only
struct OsconvTag {
    using Launch = OsconvFusedLaunch;
    static constexpr bool ok(int M, bool f64) { return osconv_fused_ok(M, f64); }
    template <int M> static hipError_t run(const Launch& F, hipStream_t stream);
};

#if DFFT_INST_GROUP < DFFT_NUM_INST_GROUPS

template <class V, class P, bool HREAL, bool VEC>
__global__ void __attribute__((amdgpu_flat_work_group_size(1, RconvGeom<V, P>::KG::THREADS)))
osconv_blocks_kernel(const typename real_of<V>::type* __restrict__ in, typename real_of<V>::type* __restrict__ out,
                     const typename RconvFilter<V, HREAL>::T* __restrict__ h, const typename VecTraits<V>::W* __restrict__ tw,
                     const typename VecTraits<V>::W* __restrict__ twh, unsigned items, unsigned nb, unsigned channels, long long n, long long n_out, int S,
                     int disc, double scale) {
    using RG = RconvGeom<V, P>;
    using KG = typename RG::KG;
    using W = typename VecTraits<V>::W;
    using RT = typename real_of<V>::type;
    using F = RconvFilter<V, HREAL>;
    constexpr int  E = P::E, T = P::T, M = P::N, G = RG::G, GT = KG::GT;
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
    const RT   sc = (RT)scale;
    const auto clamp_m = [](long long x) { return (int)(x < 0 ? 0 : x > 2 * M ? 2 * M : x); };
    for (unsigned i0 = blockIdx.x * G; i0 < items; i0 += gridDim.x * G) {
        const unsigned it = i0 + g;
        const bool     valid = it < items;
        const unsigned row = valid ? it / nb : 0u;
        // real i of the block sits at position s0 + i of its row, on the input side and on the output side alike
        const long long s0 = (long long)(valid ? it - row * nb : 0u) * S - disc;
        // loads i in [lo, hi): inside [0, n).  An item past the last one moves nothing.
        const int       lo = valid ? clamp_m(-s0) : 0, hi = valid ? clamp_m(n - s0) : 0;
        const long long ibase = (long long)row * n + s0;  // 64-bit bases; dereferenced inside the windows only
        V               v[E];
        if constexpr (VEC) {  // n, d even: s0, lo and hi are even, so a two-real value lies wholly inside the window or wholly outside
#pragma unroll
            for (int k = 0; k < E; ++k) {
                const int i = 2 * (j + T * k);
                v[k] = (i >= lo && i < hi) ? *reinterpret_cast<const V*>(in + (ibase + i)) : V{0, 0};
            }
        } else {
#pragma unroll
            for (int k = 0; k < E; ++k) {
                const int i = 2 * (j + T * k);
                v[k] = V{(i >= lo && i < hi) ? in[ibase + i] : (RT)0, (i + 1 >= lo && i + 1 < hi) ? in[ibase + i + 1] : (RT)0};
            }
        }
        run_stages<V, P, 0, +1, 1, KG::PAD, KG::WAVE_LOCAL, KG::TWMODE, TWPOW, 1, 1, KG::NW, KG::LOCALX>(v, twr, lds, j, 0);
        group_sync<KG::WAVE_LOCAL>();
#pragma unroll
        for (int k = 0; k < E; ++k) lds[lds_index<1, KG::PAD>(j + T * k, 0)] = v[k];
        group_sync<KG::WAVE_LOCAL>();
        unsigned it1 = it;  // the filter row of the item, decoded afresh (see the stores below)
        asm volatile("" : "+v"(it1));
        const typename F::T* hp = h + (size_t)(it1 < items ? (it1 / nb) % channels : 0u) * (M + 1);
#pragma unroll
        for (int k = 0; k < E; ++k) {
            const int kk = j + T * k;
            const V   zm = lds[lds_index<1, KG::PAD>(kk == 0 ? 0 : M - kk, 0)];
            const W   w = RG::TWH_REG ? wh[RG::TWH_REG ? k : 0] : twh[kk];
            const V   xe{v[k].x + zm.x, v[k].y - zm.y};  // 2 Xe[k]
            const V   xo{v[k].y + zm.y, zm.x - v[k].x};  // 2 Xo[k]
            const V   t = cmul(xo, w);
            V         ya = F::mul(V{xe.x + t.x, xe.y + t.y}, hp[kk], sc);      // Y[k]   = X[k] H[k] / m
            V         yb = F::mul(V{xe.x - t.x, t.y - xe.y}, hp[M - kk], sc);  // Y[M-k] = conj(Xe - W^k Xo) H[M-k] / m
            if (kk == 0) {  // the imaginary parts of the DC and Nyquist products are ignored
                ya.y = (RT)0;
                yb.y = (RT)0;
            }
            const V s{ya.x + yb.x, ya.y - yb.y};
            const V d{ya.x - yb.x, ya.y + yb.y};
            const V o{d.x * w.x + d.y * w.y, d.y * w.x - d.x * w.y};  // d conj(w)
            v[k] = V{s.x - o.y, -(s.y + o.x)};                        // conj(s + i o): the inverse is conj(FFT(conj Z'))
        }
        group_sync<KG::WAVE_LOCAL>();  // every partner is read before the second transform's exchanges reuse the tile
        run_stages<V, P, 0, +1, 1, KG::PAD, KG::WAVE_LOCAL, KG::TWMODE, TWPOW, 1, 1, KG::NW, KG::LOCALX>(v, twr, lds, j, 0);
        // stores i in [disc, he): below n_out.  The item is decoded once more from a copy the compiler cannot trace back, so that the
        // store base and window do not occupy registers across the two transforms (a division per item against 24-point butterflies).
        unsigned it2 = it;
        asm volatile("" : "+v"(it2));
        const bool      valid2 = it2 < items;
        const unsigned  row2 = valid2 ? it2 / nb : 0u;
        const long long t0 = (long long)(valid2 ? it2 - row2 * nb : 0u) * S - disc;
        const int       he = valid2 ? clamp_m(n_out - t0) : 0;
        const long long obase = (long long)row2 * n_out + t0;
        if constexpr (VEC) {  // disc, n_out even: as above for [disc, he)
#pragma unroll
            for (int k = 0; k < E; ++k) {
                const int i = 2 * (j + T * k);
                if (i >= disc && i < he) *reinterpret_cast<V*>(out + (obase + i)) = V{v[k].x, -v[k].y};
            }
        } else {
#pragma unroll
            for (int k = 0; k < E; ++k) {
                const int i = 2 * (j + T * k);
                if (i >= disc && i < he) out[obase + i] = v[k].x;
                if (i + 1 >= disc && i + 1 < he) out[obase + i + 1] = -v[k].y;
            }
        }
        group_sync<KG::WAVE_LOCAL>();  // the next item's exchanges reuse the tile
    }
}

template <class V, class P, bool HREAL, bool VEC> hipError_t launch_osconv_plan(const OsconvFusedLaunch& F, hipStream_t stream) {
    using RG = RconvGeom<V, P>;
    using W = typename VecTraits<V>::W;
    using RT = typename real_of<V>::type;
    using HT = typename RconvFilter<V, HREAL>::T;
    auto                    kern = osconv_blocks_kernel<V, P, HREAL, VEC>;
    static std::atomic<int> blocks_per_cu[kMaxDevices];
    hipError_t              e;
    const int               bpc = resident_blocks_per_cu(reinterpret_cast<const void*>(kern), RG::KG::THREADS, RG::LDS_BYTES, blocks_per_cu, &e);
    if (bpc == 0) return e;
    const long long grid = persistent_grid(device_info().cus, bpc, (F.items + RG::G - 1) / RG::G);
    if (grid < 1) return hipSuccess;
    (void)hipGetLastError();
    hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(RG::KG::THREADS), RG::LDS_BYTES, stream, (const RT*)F.in, (RT*)F.out, (const HT*)F.h,
                       (const W*)F.tw, (const W*)F.twh, (unsigned)F.items, (unsigned)F.nb, (unsigned)F.channels, F.n, F.n_out, (int)(F.m - F.discard),
                       (int)F.discard, 0.5 / (double)F.m);
    return hipGetLastError();
}

template <class V, int M> hipError_t osconv_run_typed(const OsconvFusedLaunch& F, hipStream_t stream) {
    using P = typename PlanFor<M>::type;
    if constexpr (osconv_fused_ok(M, sizeof(V) == 16)) {
        if (F.filter_kind == RCONV_FILTER_REAL)
            return F.vec ? launch_osconv_plan<V, P, true, true>(F, stream) : launch_osconv_plan<V, P, true, false>(F, stream);
        return F.vec ? launch_osconv_plan<V, P, false, true>(F, stream) : launch_osconv_plan<V, P, false, false>(F, stream);
    }
    return hipErrorInvalidValue;  // not built (osconv_fused_ok): the dispatcher does not come here
}
template <int M> hipError_t OsconvTag::run(const OsconvFusedLaunch& F, hipStream_t stream) {
    if (F.dtype == F64) return osconv_run_typed<double2, M>(F, stream);
    if (F.dtype == F32) return osconv_run_typed<float2, M>(F, stream);
    return hipErrorInvalidValue;
}
DFFT_FUSED_INSTANTIATE(OsconvTag)

#else  // the dispatcher, the block chooser and the kernels of the composed form

// item (it0 + t) = (row, b): row = item / nb, b = item % nb
// zero-filled blocks: p[t][i] = x[row][b S - d + i] inside [0, n), else 0
template <class RT>
__global__ void __launch_bounds__(256) osconv_gather_kernel(const RT* __restrict__ in, RT* __restrict__ p, long long n, long long m, long long S, long long d,
                                                            long long nb, long long it0, long long total) {
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
        const long long t = e / m, i = e - t * m;
        const long long row = (it0 + t) / nb, b = (it0 + t) - row * nb;
        const long long s = b * S - d + i;
        p[e] = (s >= 0 && s < n) ? in[row * n + s] : (RT)0;
    }
}
// valid windows: y[row][b S + j] = p[t][d + j], 0 <= j < S, b S + j < n_out
template <class RT>
__global__ void __launch_bounds__(256) osconv_scatter_kernel(const RT* __restrict__ p, RT* __restrict__ out, long long n_out, long long m, long long S,
                                                             long long d, long long nb, long long it0, long long total) {
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
        const long long t = e / S, jj = e - t * S;
        const long long row = (it0 + t) / nb, b = (it0 + t) - row * nb;
        const long long o = b * S + jj;
        if (o < n_out) out[row * n_out + o] = p[t * m + d + jj];
    }
}
// bins[t][k] *= H[row(it0 + t) % channels][k] / m, k <= M
template <class V, class HT>
__global__ void __launch_bounds__(256) osconv_mul_kernel(V* __restrict__ bins, const HT* __restrict__ h, long long nbins, long long nb, long long it0,
                                                         long long channels, long long total, double scale) {
    using RT = typename real_of<V>::type;
    const RT sc = (RT)scale;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
        const long long t = e / nbins, k = e - t * nbins;
        const HT        hk = h[(((it0 + t) / nb) % channels) * nbins + k];
        const V         x = bins[e];
        if constexpr (sizeof(HT) == sizeof(V)) bins[e] = cmul(x, V{hk.x * sc, hk.y * sc});
        else bins[e] = V{x.x * (hk * sc), x.y * (hk * sc)};
    }
}

namespace {

// one item of the composed form: its m/2 + 1 bins and its m gathered reals
size_t item_bytes(long long m, int dtype) { return (size_t)(m / 2 + 1) * elem_bytes(dtype) + (size_t)m * (elem_bytes(dtype) / 2); }

bool sizes_ok(const OsconvLaunch& L) {
    if (L.n < 1 || L.n_out < 1 || L.discard < 0 || L.m <= L.discard || L.n_out - L.discard > L.n || !real_length_supported(L.m) || L.channels < 1 ||
        L.batch < 1 || L.channels >= (1ll << 31) || L.batch >= (1ll << 31) || L.batch * L.channels >= (1ll << 31))
        return false;
    return osconv_blocks(L.n_out, L.m, L.discard) <= ((1ll << 31) - 1) / (L.batch * L.channels);  // fewer than 2^31 items
}

template <class V> int osconv_chunk(const OsconvLaunch& L, long long nb, long long it0, long long ni, void* scratch, hipStream_t stream) {
    using RT = typename real_of<V>::type;
    const long long m = L.m, d = L.discard, S = m - d, nbins = m / 2 + 1;
    V*              bins = (V*)scratch;              // [ni][nbins]; a multiple of sizeof(V) bytes, so the blocks behind it stay aligned to V
    RT*             pad = (RT*)(bins + ni * nbins);  // [ni][m]
    (void)hipGetLastError();
    hipLaunchKernelGGL(osconv_gather_kernel<RT>, dim3(elementwise_grid(ni * m)), dim3(256), 0, stream, (const RT*)L.in, pad, L.n, m, S, d, nb, it0, ni * m);
    DFFT_HIP_TRY(hipGetLastError());
    hipError_t e = launch_real_rows(contiguous_real_rows(L.dtype, m, ni, +1, 1.0, pad, bins), stream);
    if (e != hipSuccess) return fail(DFFT_EHIP, std::string("rconv_os (R2C rows): ") + hipGetErrorString(e));
    if (L.filter_kind == RCONV_FILTER_REAL)
        hipLaunchKernelGGL((osconv_mul_kernel<V, RT>), dim3(elementwise_grid(ni * nbins)), dim3(256), 0, stream, bins, (const RT*)L.h, nbins, nb, it0, L.channels,
                           ni * nbins, 1.0 / (double)m);
    else
        hipLaunchKernelGGL((osconv_mul_kernel<V, V>), dim3(elementwise_grid(ni * nbins)), dim3(256), 0, stream, bins, (const V*)L.h, nbins, nb, it0, L.channels,
                           ni * nbins, 1.0 / (double)m);
    DFFT_HIP_TRY(hipGetLastError());
    // (the two-launch form of an untuned m/2 merges in place on its input: the bins are scratch)
    e = launch_real_rows(contiguous_real_rows(L.dtype, m, ni, -1, 1.0, bins, pad), stream);
    if (e != hipSuccess) return fail(DFFT_EHIP, std::string("rconv_os (C2R rows): ") + hipGetErrorString(e));
    hipLaunchKernelGGL(osconv_scatter_kernel<RT>, dim3(elementwise_grid(ni * S)), dim3(256), 0, stream, (const RT*)pad, (RT*)L.out, L.n_out, m, S, d, nb, it0,
                       ni * S);
    DFFT_HIP_TRY(hipGetLastError());
    return DFFT_OK;
}

// Per-block time t(m) of the chooser, in nanoseconds of the fused route with many blocks in flight.  ONE table: the power-of-two block
// lengths were measured on an MI355X (tools/osconv_bench.py --blocks: 1024 rows of 131072 samples, discard = m / 4, medians of two runs
// that agree within 1 %; profiles/2026-10-20_rconv1d_os/README.md) and replaced the seed m log2 m.  Every other length takes the time per
// sample of the measured entry next above it (below 256: of 256), so an unmeasured length never looks cheaper per sample than a
// measured one: the three unmeasured lengths the seeded table chose (2000, 4374, 4802) all measured slower than it predicted.  The step between 1024 and 2048 is the kernels': up
// to m = 1024 a block streams at 3.5 / 2.4 TB/s (fp64 / fp32), from 2048 on at 1.5 - 1.7 / 1.3 - 1.6 TB/s.  Lengths on the composed
// route cost kComposedFactor times as much (measured 1.4 - 2.6 x the fused route; the factor also keeps a block the library cannot fuse
// from winning by a hair).
struct BlockTime {
    int    m;
    double ns[2];  // fp64, fp32
};
constexpr BlockTime kBlockTimes[] = {
    // OSCONV_BLOCK_TIMES_BEGIN
    {256, {0.781, 0.591}},  {512, {1.659, 1.227}},   {1024, {3.531, 2.552}},
    {2048, {14.10, 7.437}}, {4096, {31.72, 18.63}}, {8192, {63.21, 35.56}},
    // OSCONV_BLOCK_TIMES_END
};
constexpr double kComposedFactor = 3.0;

double block_time(long long m, int dtype) {
    const int   col = dtype == F64 ? 0 : 1;
    const auto* e = &kBlockTimes[0];
    for (const auto& r : kBlockTimes) {
        e = &r;
        if (r.m >= m) break;
    }
    const double t = e->ns[col] * (double)m / (double)e->m;
    return osconv_fused(m, dtype) ? t : kComposedFactor * t;
}

}  // namespace

long long osconv_blocks(long long n_out, long long m, long long discard) {
    if (n_out < 1 || discard < 0 || m <= discard) return 0;
    const long long S = m - discard;
    return n_out / S + (n_out % S != 0);
}

bool osconv_vec(const void* in, const void* out, long long n, long long n_out, long long discard, int dtype) {
    return n % 2 == 0 && n_out % 2 == 0 && discard % 2 == 0 && (uintptr_t)in % elem_bytes(dtype) == 0 && (uintptr_t)out % elem_bytes(dtype) == 0;
}

bool osconv_fused(long long m, int dtype) {
    if ((dtype != F64 && dtype != F32) || !rconv_fused(1, m, dtype, RCONV_FILTER_COMPLEX, false)) return false;
    return tuned_built<OsconvTag>(m / 2, dtype == F64);
}

size_t osconv_scratch_bytes(const OsconvLaunch& L, bool fused_on, size_t cap) {
    if ((L.dtype != F64 && L.dtype != F32) || !sizes_ok(L)) return 0;
    if (fused_on && osconv_fused(L.m, L.dtype)) return 0;
    return (size_t)chunk_units(item_bytes(L.m, L.dtype), L.batch * L.channels * osconv_blocks(L.n_out, L.m, L.discard), cap) * item_bytes(L.m, L.dtype);
}

int osconv(const OsconvLaunch& L, bool fused_on, size_t cap, void* scratch, size_t scratch_bytes, hipStream_t stream) {
    if ((L.dtype != F64 && L.dtype != F32) || (L.filter_kind != RCONV_FILTER_COMPLEX && L.filter_kind != RCONV_FILTER_REAL) || !L.in || !L.out || !L.h ||
        !sizes_ok(L))
        return fail(DFFT_EINVAL, "rconv_os: bad arguments");
    const long long nb = osconv_blocks(L.n_out, L.m, L.discard), items = L.batch * L.channels * nb;
    if (fused_on && osconv_fused(L.m, L.dtype)) {
        OsconvFusedLaunch F;
        std::memset(&F, 0, sizeof(F));
        F.dtype = L.dtype;
        F.filter_kind = L.filter_kind;
        F.n = L.n;
        F.n_out = L.n_out;
        F.m = L.m;
        F.discard = L.discard;
        F.channels = L.channels;
        F.items = items;
        F.nb = nb;
        F.vec = osconv_vec(L.in, L.out, L.n, L.n_out, L.discard, L.dtype);
        F.in = L.in;
        F.out = L.out;
        F.h = L.h;
        if (int rc = get_twiddles((int)(L.m / 2), L.dtype, &F.tw)) return rc;
        if (int rc = get_twiddles((int)L.m, L.dtype, &F.twh)) return rc;
        const hipError_t e = run_tuned<OsconvTag>(L.m / 2, F, stream);
        if (e == hipSuccess) return DFFT_OK;
        return fail(DFFT_EHIP, std::string("rconv_os (fused): ") + hipGetErrorString(e));
    }
    // chunks of items whose gathered blocks and bins fit the scratch buffer
    const size_t    ib = item_bytes(L.m, L.dtype);
    const long long ni = fit_chunk_to_lease("rconv_os", chunk_units(ib, items, cap), ib, scratch, scratch_bytes);
    if (ni < 1) return DFFT_EINVAL;
    for (long long i0 = 0; i0 < items; i0 += ni) {
        const long long k = std::min(ni, items - i0);
        const int       rc = L.dtype == F64 ? osconv_chunk<double2>(L, nb, i0, k, scratch, stream) : osconv_chunk<float2>(L, nb, i0, k, scratch, stream);
        if (rc) return rc;
    }
    return DFFT_OK;
}

bool osconv_block(long long taps, long long n_out, int dtype, long long* m_out, long long* d_out) {
    if (taps < 1 || taps > 8191 || n_out < 1 || (dtype != F64 && dtype != F32)) return false;
    const long long d = (taps - 1) + ((taps - 1) & 1);
    long long       best_m = 0, best_nb = 0;
    double          best = 0.0;
    for (long long m = std::max(d + 1, 4ll) + (std::max(d + 1, 4ll) & 1); m <= 8192; m += 2) {
        if (!real_length_supported(m)) continue;
        const long long nb = osconv_blocks(n_out, m, d);
        const double cost = (double)nb * block_time(m, dtype);
        // a problem that fits one block comes out as one block, whatever the table says about several smaller ones
        if (!best_m || (nb == 1 && best_nb != 1) || ((nb == 1) == (best_nb == 1) && cost < best)) {
            best_m = m;
            best_nb = nb;
            best = cost;
        }
    }
    if (!best_m) return false;
    *m_out = best_m;
    *d_out = d;
    return true;
}

#endif

}  // namespace dfft
