// dfft_rconv.hip -- batched 1-D real FFT convolution: every row of reals [batch][channels][n] filtered by its channel's spectrum,
//     y[b, c, :] = irfft(rfft(x[b, c, :], m) * H[c, :], m)[:n],        H [channels][m/2 + 1],  n <= m,  m = 2 M,
// for M a single-pass length (real form 1, m <= 8192).  m == n is the circular convolution, m >= n + taps - 1 the first n samples of
// the linear one.  Longer sequences run block by block through dfft_osconv.hip (overlap-save); four-step and Bluestein halves are not built.
//
// Fused form, rconv_rows_kernel (M with a tuned plan of dfft_plans.h): ONE launch that reads a row once and writes it once.  The row
// is loaded as the M complex values z[j] = x[2j] + i x[2j+1], zeros beyond n -- the padded part of the row exists in registers only --
// and transformed with the M-point stages of the row kernels (run_stages, dfft_fft_impl.h; geometry and twiddle placement of
// dfft_real.hip's RealGeom).  ONE LDS exchange brings Z[M-k] to the thread that holds Z[k]; with W = e^{-2 pi i / m} that thread forms
//     Xe = (Z[k] + conj Z[M-k]) / 2,  Xo = -i (Z[k] - conj Z[M-k]) / 2,  X[k] = Xe + W^k Xo,  X[M-k] = conj(Xe - W^k Xo)
// (Xe[M-k] = conj Xe[k], Xo[M-k] = conj Xo[k], W^(M-k) = -conj W^k), multiplies them by H[c][k] / m and H[c][M-k] / m, and merges the
// two products straight into the inverse's input
//     Z'[k] = (Y[k] + conj Y[M-k]) + i (Y[k] - conj Y[M-k]) conj(W^k)
// -- the partner thread does the same for M-k, so no second exchange and no spectrum in memory are needed (the price: every product is
// formed twice).  k = 0 pairs with itself through Z[M] = Z[0] and takes H[c][0], H[c][M]; the imaginary parts of those two products
// are dropped (the rule of dfft_rfft1d backward, numpy's).  For even M the bin k = M/2 pairs with itself and the general formulas
// hold.  The inverse M-point transform runs as conj . forward . conj, so ONE set of forward twiddles serves both transforms (the form
// of the fused X stage, dfft_conv.hip); Re / Im of its result are the even / odd reals, of which the first n are stored.
//
// Where n is even and both pointers are aligned to two reals (VEC) a row is loaded and stored as two-real values, otherwise real by
// real (the rule of dfft_r2r_fused_applies).  In place (out == in): a thread group owns its row and has loaded all of it before it
// stores any -- every load feeds the first run_stages and every store follows the group barriers behind it -- and rows of different
// groups are disjoint; for the same reason the kernel does not mark its real pointers __restrict__.
//
// Composed form (every other accepted M, the instantiations rconv_fused_ok leaves out, DFFT_RCONV_FUSED=0): per chunk of rows of at
// most max(256 MiB, one row's) scratch -- pad_rows (dfft_rows_common.hip) into padded rows, launch_real_rows forward, rconv_mul_kernel
// (H / m, in place on the bins), launch_real_rows backward, trunc_rows into `out`.
//
// Compiled once per instantiation group (-DDFFT_INST_GROUP=g: the fused kernels of the tuned lengths of group g) and once with
// -DDFFT_INST_GROUP=DFFT_NUM_INST_GROUPS (the dispatcher and the kernels of the composed form).
#include "dfft_fused_host.h"
#include "dfft_rconv.h"
#include "dfft_rconv_impl.h"
#include "dfft_rows_common.h"

#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <cstring>

#ifndef DFFT_INST_GROUP
#error "compile with -DDFFT_INST_GROUP=<g>"
#endif

namespace dfft {

// One fused launch
struct RconvFusedLaunch {
    int         dtype, filter_kind;
    long long   n, m, channels, rows;
    bool        vec;
    const void* in;
    void*       out;
    const void* h;
    const void* tw;   // e^{-2 pi i k / M}
    const void* twh;  // e^{-2 pi i k / m}
};

// (M, dtype) whose instantiations would keep values in scratch memory (tools/fused_resources.py rconv, profiles/2026-10-19_rconv1d/
// kernel_resources.txt) or measured slower than the composed form are not built: they run the composed form.
constexpr bool rconv_fused_ok(int M, bool f64) {
    if (M == 3125) return false;         // 25 points per thread: 184 ... 684 bytes per lane in fp64 and fp32, either access width
    if (M == 1536 && f64) return false;  // 24 points: 356 / 388 bytes per lane with per-real accesses (none with two-real ones)
    return true;
}

// the family (dfft_fused_host.h); run<M>: defined in the translation unit of M's group only
struct RconvTag {
    using Launch = RconvFusedLaunch;
    static constexpr bool ok(int M, bool f64) { return rconv_fused_ok(M, f64); }
    template <int M> static hipError_t run(const Launch& F, hipStream_t stream);
};

#if DFFT_INST_GROUP < DFFT_NUM_INST_GROUPS

// RconvGeom (the geometry) and RconvFilter (a filter element and its product with a bin): dfft_rconv_impl.h, shared with the overlap-save
// kernel of dfft_osconv.hip, which repeats the pairing / multiply / merge step below (as a shared function it changed this kernel's registers).

template <class V, class P, bool HREAL, bool VEC>
__global__ void __attribute__((amdgpu_flat_work_group_size(1, RconvGeom<V, P>::KG::THREADS)))
rconv_rows_kernel(const typename real_of<V>::type* in, typename real_of<V>::type* out, const typename RconvFilter<V, HREAL>::T* __restrict__ h,
                  const typename VecTraits<V>::W* __restrict__ tw, const typename VecTraits<V>::W* __restrict__ twh, unsigned rows, unsigned channels,
                  int n, double scale) {
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
    const RT sc = (RT)scale;
    for (unsigned r0 = blockIdx.x * G; r0 < rows; r0 += gridDim.x * G) {
        const unsigned  row = r0 + g;
        const bool      valid = row < rows;
        const long long base = valid ? (long long)row * n : 0ll;  // 64-bit row bases
        V               v[E];
        // rrow_load (dfft_rconv_impl.h) written out: called as a function it changed this kernel's registers
        if constexpr (VEC) {  // n even: a two-real value lies wholly inside the row or wholly in the padding
            const V* ip = reinterpret_cast<const V*>(in + base);
#pragma unroll
            for (int k = 0; k < E; ++k) {
                const int kk = j + T * k;
                v[k] = (valid && 2 * kk < n) ? ip[kk] : V{0, 0};
            }
        } else {
            const RT* ip = in + base;
#pragma unroll
            for (int k = 0; k < E; ++k) {
                const int kk = j + T * k;
                v[k] = V{(valid && 2 * kk < n) ? ip[2 * kk] : (RT)0, (valid && 2 * kk + 1 < n) ? ip[2 * kk + 1] : (RT)0};
            }
        }
        run_stages<V, P, 0, +1, 1, KG::PAD, KG::WAVE_LOCAL, KG::TWMODE, TWPOW, 1, 1, KG::NW, KG::LOCALX>(v, twr, lds, j, 0);
        group_sync<KG::WAVE_LOCAL>();
#pragma unroll
        for (int k = 0; k < E; ++k) lds[lds_index<1, KG::PAD>(j + T * k, 0)] = v[k];
        group_sync<KG::WAVE_LOCAL>();
        const typename F::T* hp = h + (size_t)(valid ? row % channels : 0u) * (M + 1);
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
        if (valid) {
            if constexpr (VEC) {
                V* op = reinterpret_cast<V*>(out + base);
#pragma unroll
                for (int k = 0; k < E; ++k) {
                    const int kk = j + T * k;
                    if (2 * kk < n) op[kk] = V{v[k].x, -v[k].y};
                }
            } else {
                RT* op = out + base;
#pragma unroll
                for (int k = 0; k < E; ++k) {
                    const int kk = j + T * k;
                    if (2 * kk < n) op[2 * kk] = v[k].x;
                    if (2 * kk + 1 < n) op[2 * kk + 1] = -v[k].y;
                }
            }
        }
        group_sync<KG::WAVE_LOCAL>();  // the next row's exchanges reuse the tile
    }
}

template <class V, class P, bool HREAL, bool VEC> hipError_t launch_rconv_plan(const RconvFusedLaunch& F, hipStream_t stream) {
    using RG = RconvGeom<V, P>;
    using W = typename VecTraits<V>::W;
    using RT = typename real_of<V>::type;
    using HT = typename RconvFilter<V, HREAL>::T;
    auto                    kern = rconv_rows_kernel<V, P, HREAL, VEC>;
    static std::atomic<int> blocks_per_cu[kMaxDevices];
    hipError_t              e;
    const int               bpc = resident_blocks_per_cu(reinterpret_cast<const void*>(kern), RG::KG::THREADS, RG::LDS_BYTES, blocks_per_cu, &e);
    if (bpc == 0) return e;
    const long long grid = persistent_grid(device_info().cus, bpc, (F.rows + RG::G - 1) / RG::G);
    if (grid < 1) return hipSuccess;
    (void)hipGetLastError();
    hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(RG::KG::THREADS), RG::LDS_BYTES, stream, (const RT*)F.in, (RT*)F.out, (const HT*)F.h,
                       (const W*)F.tw, (const W*)F.twh, (unsigned)F.rows, (unsigned)F.channels, (int)F.n, 0.5 / (double)F.m);
    return hipGetLastError();
}

template <class V, int M> hipError_t rconv_run_typed(const RconvFusedLaunch& F, hipStream_t stream) {
    using P = typename PlanFor<M>::type;
    if constexpr (rconv_fused_ok(M, sizeof(V) == 16)) {
        if (F.filter_kind == RCONV_FILTER_REAL)
            return F.vec ? launch_rconv_plan<V, P, true, true>(F, stream) : launch_rconv_plan<V, P, true, false>(F, stream);
        return F.vec ? launch_rconv_plan<V, P, false, true>(F, stream) : launch_rconv_plan<V, P, false, false>(F, stream);
    }
    return hipErrorInvalidValue;  // not built (rconv_fused_ok): the dispatcher does not come here
}
template <int M> hipError_t RconvTag::run(const RconvFusedLaunch& F, hipStream_t stream) {
    if (F.dtype == F64) return rconv_run_typed<double2, M>(F, stream);
    if (F.dtype == F32) return rconv_run_typed<float2, M>(F, stream);
    return hipErrorInvalidValue;
}
DFFT_FUSED_INSTANTIATE(RconvTag)

#else  // the dispatcher and the multiply kernel of the composed form

// bins[r][k] *= H[(row0 + r) % channels][k] / m, k <= M
template <class V, class HT>
__global__ void __launch_bounds__(256) rconv_mul_kernel(V* __restrict__ bins, const HT* __restrict__ h, long long nb, long long row0, long long channels,
                                                        long long total, double scale) {
    using RT = typename real_of<V>::type;
    const RT sc = (RT)scale;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
        const long long r = e / nb, k = e - r * nb;
        const HT        hk = h[((row0 + r) % channels) * nb + k];
        const V         x = bins[e];
        if constexpr (sizeof(HT) == sizeof(V)) bins[e] = cmul(x, V{hk.x * sc, hk.y * sc});
        else bins[e] = V{x.x * (hk * sc), x.y * (hk * sc)};
    }
}

namespace {

// one row of the composed form: its m/2 + 1 bins and its m padded reals
size_t row_bytes(long long m, int dtype) { return (size_t)(m / 2 + 1) * elem_bytes(dtype) + (size_t)m * (elem_bytes(dtype) / 2); }

template <class V> int rconv_chunk(const RconvLaunch& L, long long row0, long long nr, void* scratch, hipStream_t stream) {
    using RT = typename real_of<V>::type;
    const long long n = L.n, m = L.m, nb = m / 2 + 1;
    V*              bins = (V*)scratch;             // [nr][nb]; a multiple of sizeof(V) bytes, so the rows behind it stay aligned to V
    RT*             pad = (RT*)(bins + nr * nb);    // [nr][m]
    const RT*       in = (const RT*)L.in + row0 * n;
    RT*             out = (RT*)L.out + row0 * n;
    if (int rc = pad_rows(in, pad, n, m, nr, L.dtype, stream)) return rc;
    hipError_t e = launch_real_rows(contiguous_real_rows(L.dtype, m, nr, +1, 1.0, pad, bins), stream);
    if (e != hipSuccess) return fail(DFFT_EHIP, std::string("rconv (R2C rows): ") + hipGetErrorString(e));
    if (L.filter_kind == RCONV_FILTER_REAL)
        hipLaunchKernelGGL((rconv_mul_kernel<V, RT>), dim3(elementwise_grid(nr * nb)), dim3(256), 0, stream, bins, (const RT*)L.h, nb, row0, L.channels,
                           nr * nb, 1.0 / (double)m);
    else
        hipLaunchKernelGGL((rconv_mul_kernel<V, V>), dim3(elementwise_grid(nr * nb)), dim3(256), 0, stream, bins, (const V*)L.h, nb, row0, L.channels,
                           nr * nb, 1.0 / (double)m);
    DFFT_HIP_TRY(hipGetLastError());
    // (the two-launch form of an untuned m/2 merges in place on its input: the bins are scratch)
    e = launch_real_rows(contiguous_real_rows(L.dtype, m, nr, -1, 1.0, bins, pad), stream);
    if (e != hipSuccess) return fail(DFFT_EHIP, std::string("rconv (C2R rows): ") + hipGetErrorString(e));
    return trunc_rows(pad, out, n, m, nr, L.dtype, stream);
}

}  // namespace

long long rconv_length(long long at_least) {
    for (long long m = std::max(at_least, 2ll) + (std::max(at_least, 2ll) & 1); m <= 8192; m += 2)
        if (real_length_supported(m)) return m;
    return 0;
}

bool rconv_fused_env() { return env_switch_on("DFFT_RCONV_FUSED"); }

bool rconv_vec(const void* in, const void* out, long long n, int dtype) {
    return n % 2 == 0 && (uintptr_t)in % elem_bytes(dtype) == 0 && (uintptr_t)out % elem_bytes(dtype) == 0;
}

bool rconv_fused(long long n, long long m, int dtype, int filter_kind, bool vec) {
    (void)vec;
    if (n < 1 || m < n || !real_length_supported(m) || (dtype != F64 && dtype != F32)) return false;
    if (filter_kind != RCONV_FILTER_COMPLEX && filter_kind != RCONV_FILTER_REAL) return false;
    return tuned_built<RconvTag>(m / 2, dtype == F64);
}

size_t rconv_scratch_bytes(const RconvLaunch& L, bool fused_on, size_t cap) {
    if (L.n < 1 || L.m < L.n || !real_length_supported(L.m) || L.channels < 1 || L.batch < 1) return 0;
    if (fused_on && rconv_fused(L.n, L.m, L.dtype, L.filter_kind, rconv_vec(L.in, L.out, L.n, L.dtype))) return 0;
    return (size_t)chunk_units(row_bytes(L.m, L.dtype), L.batch * L.channels, cap) * row_bytes(L.m, L.dtype);
}

int rconv(const RconvLaunch& L, bool fused_on, size_t cap, void* scratch, size_t scratch_bytes, hipStream_t stream) {
    if (L.n < 1 || L.m < L.n || !real_length_supported(L.m) || L.channels < 1 || L.batch < 1 || (L.dtype != F64 && L.dtype != F32) ||
        (L.filter_kind != RCONV_FILTER_COMPLEX && L.filter_kind != RCONV_FILTER_REAL) || !L.in || !L.out || !L.h)
        return fail(DFFT_EINVAL, "rconv: bad arguments");
    const long long rows = L.batch * L.channels;
    if (rows >= (1ll << 31)) return fail(DFFT_EINVAL, "rconv: 2^31 or more rows");
    const bool vec = rconv_vec(L.in, L.out, L.n, L.dtype);
    if (fused_on && rconv_fused(L.n, L.m, L.dtype, L.filter_kind, vec)) {
        RconvFusedLaunch F;
        std::memset(&F, 0, sizeof(F));
        F.dtype = L.dtype;
        F.filter_kind = L.filter_kind;
        F.n = L.n;
        F.m = L.m;
        F.channels = L.channels;
        F.rows = rows;
        F.vec = vec;
        F.in = L.in;
        F.out = L.out;
        F.h = L.h;
        if (int rc = get_twiddles((int)(L.m / 2), L.dtype, &F.tw)) return rc;
        if (int rc = get_twiddles((int)L.m, L.dtype, &F.twh)) return rc;
        const hipError_t e = run_tuned<RconvTag>(L.m / 2, F, stream);
        if (e == hipSuccess) return DFFT_OK;
        return fail(DFFT_EHIP, std::string("rconv (fused): ") + hipGetErrorString(e));
    }
    // chunks of rows whose padded rows and bins fit the scratch buffer
    const size_t    rb = row_bytes(L.m, L.dtype);
    const long long nr = fit_chunk_to_lease("rconv", chunk_units(rb, rows, cap), rb, scratch, scratch_bytes);
    if (nr < 1) return DFFT_EINVAL;
    for (long long r0 = 0; r0 < rows; r0 += nr) {
        const long long k = std::min(nr, rows - r0);
        const int       rc = L.dtype == F64 ? rconv_chunk<double2>(L, r0, k, scratch, stream) : rconv_chunk<float2>(L, r0, k, scratch, stream);
        if (rc) return rc;
    }
    return DFFT_OK;
}

#endif

}  // namespace dfft
