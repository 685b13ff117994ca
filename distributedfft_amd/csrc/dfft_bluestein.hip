// dfft_bluestein.hip -- any-length transforms by Bluestein's chirp-z algorithm: the lengths the single-pass kernels (7-smooth, <= 4096)
// and the four-step form (dfft_long.hip) do not serve, up to 2^23 points.
//
// Per transform of length n in direction d, with the chirp c_m = exp(-d i pi (m^2 mod 2n) / n) and a padded length M >= 2n - 1:
//     a_j = x_j c_j (j < n), 0 (n <= j < M);   A = FFT_M(a);   conv = IFFT_M(A . B^);   X_k = c_k conv_k   (k < n)
// where B^ = FFT_M(b) / M, b_m = conj(c_|m|) for |m| < n (wrapped mod M), 0 elsewhere -- the 1/M of the inverse is folded into B^, which
// is computed once per (device, n, dtype, direction) in fp64 with the library's own forward FFT (rounded once for fp32) and cached next to
// the twiddle tables.  Why it works: jk = (j^2 + k^2 - (k - j)^2) / 2, so exp(-2 pi i d jk / n) = c_j c_k conj(c_{k-j}) and X is c times
// the convolution of (x c) with conj(c) -- a circular one of length M once M >= 2n - 1.
//
// Fused form, n <= 2048 (one launch, M the smallest tuned length >= 2n - 1, at most 4096): a thread group loads the n points of a
// transform times the chirp (zeros up to M exist only in registers), runs the tuned M-point stages of the C2C kernels (run_stages,
// dfft_fft_impl.h, dfft_plans.h), multiplies by B^ (read from global memory: M elements shared by every transform, L2-resident), runs
// the inverse as conj . forward . conj -- so one set of forward twiddles serves both halves -- and stores n points times the chirp:
// the HBM bytes of an n-point C2C transform.  Rows (s = 1): bluestein_rows_kernel, one transform per thread group like the C2C row
// kernel; columns ([batch][n][s], s > 1): bluestein_cols_kernel, tiles of the C2C column kernel's width (cols_per_tile: adjacent columns
// of one FFT point are one 128-byte line, or a half / quarter line where the tile would not fit the LDS).
//
// Multi-pass form, n > 2048 (or DFFT_BLUESTEIN_FUSED=0), M the smallest length >= 2n - 1 that long_split accepts (at most 2^24; under
// DFFT_BLUESTEIN_FUSED=0 with n <= 2048 the fused form's M): bluestein_pad_kernel (chirp and zero padding into scratch [b][M][s]),
// forward FFT_M (long_fft, or the single-pass kernels for M <= 4096), bluestein_mul_kernel (times B^), inverse FFT_M,
// bluestein_finish_kernel (chirp, scale, truncation into `out`).  Plain, like dfft_long.hip; the batch runs in chunks whose scratch
// stays within max(256 MiB, one transform's).
//
// Compiled once per instantiation group (-DDFFT_INST_GROUP=g: the fused kernels of the tuned lengths of group g) and once with
// -DDFFT_INST_GROUP=DFFT_NUM_INST_GROUPS (the dispatcher, the multi-pass kernels and the tables).
#include "dfft_fused_host.h"
#include "dfft_bluestein.h"
#include "dfft_long.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <map>
#include <mutex>
#include <tuple>
#include <vector>

#ifndef DFFT_INST_GROUP
#error "compile with -DDFFT_INST_GROUP=<g>"
#endif

namespace dfft {

// the smallest M the fused form can be asked for: the smallest length of the Bluestein range is 11 (n = 1 is a scaled copy), 2 * 11 - 1 = 21
constexpr int kFusedMinM = 21;

struct FusedLaunch {
    int         dtype;
    int         n;
    long long   s, batch;
    const void *in, *tw, *chirp, *bhat;
    void*       out;
    double      scale;
};

// entry point of padded length N: defined (and explicitly instantiated) in the translation unit of N's group only
template <bool ON, int N> struct BsInst {};
template <int N> struct BsInst<true, N> {
    static hipError_t run(const FusedLaunch& F, hipStream_t stream);
};

#if DFFT_INST_GROUP < DFFT_NUM_INST_GROUPS

// Geometry: CB adjacent columns per tile (1 for rows; the C2C column kernel's cols_per_tile otherwise), about 256 threads per workgroup,
// twiddles and exchange tile where KernelGeom puts them.
// Column tiles: the C2C column kernel's width (cols_per_tile), narrowed until the workgroup has at most 512 threads -- 256 where a
// thread's points alone take 40 registers or more -- because this kernel keeps a thread's E points live across two transforms and the B^
// multiply (at 1024 threads, i.e. 128 registers, the 2048- and 2187-point fp32 tiles spilled 336 and 108 bytes; at 512 threads the
// 2048-point fp64 tile 92 bytes, the 1280- and 1536-point fp32 tiles 12 and 340 bytes).
template <class V, class P> constexpr int bs_cols_per_tile() {
    int       cb = cols_per_tile<V, P>();
    const int max_threads = P::E * (int)sizeof(V) / 4 >= 40 ? 256 : 512;
    while (cb > 1 && cb * P::T > max_threads) cb /= 2;
    return cb;
}

template <class V, class P, bool COLS> struct BsGeom {
    static constexpr int CB = COLS ? bs_cols_per_tile<V, P>() : 1;
    static constexpr int G = ConstMax1<256 / (CB * P::T)>::value;
    using KG = KernelGeom<V, P, CB, G, TuneDefault>;
};

// One launch per call: thread group g of a workgroup owns tile r0 + g -- a row (COLS = false: data[r][n]) or CB adjacent columns of one
// batch item (COLS = true: data[b][n][s], tile = b * tiles_per_b + column block).  `in` and `out` may be the same buffer: a tile reads
// all its points before the first exchange and writes them after the last one, and no two tiles share an element.
template <class V, class P, bool COLS>
__device__ __forceinline__ void bluestein_tiles(const V* in, V* out, const typename VecTraits<V>::W* __restrict__ tw, const V* __restrict__ chirp,
                                                const V* __restrict__ bhat, int n, long long s, unsigned tiles, unsigned tiles_per_b, double scale) {
    using BG = BsGeom<V, P, COLS>;
    using KG = typename BG::KG;
    using W = typename VecTraits<V>::W;
    using RT = typename real_of<W>::type;
    constexpr int  E = P::E, T = P::T, G = BG::G, GT = KG::GT, CB = BG::CB;
    constexpr bool TWPOW = KG::TWMODE == TW_REG;
    extern __shared__ __attribute__((aligned(16))) char dfft_smem[];
    const int g = threadIdx.x / GT;
    const int tid = (int)threadIdx.x - g * GT;
    const int c = tid % CB;
    const int j = tile_j<CB, KG::NW>(tid);
    V*        lds = reinterpret_cast<V*>(dfft_smem + KG::TW_BYTES) + g * KG::LDS_ELEMS;
    W         twreg[KG::TWMODE == TW_REG && KG::TWN > 0 ? KG::TWN : 1];
    const W*  twr = stage_twiddles<V, P, +1, KG>(twreg, reinterpret_cast<W*>(dfft_smem), tw, j);
    const RT  sc = (RT)scale;
    for (unsigned r0 = blockIdx.x * G; r0 < tiles; r0 += gridDim.x * G) {
        const unsigned t = r0 + g;
        bool           valid = t < tiles;
        long long      base = 0, step = 1;
        if constexpr (COLS) {
            const unsigned b = valid ? t / tiles_per_b : 0u, cb = valid ? t - b * tiles_per_b : 0u;
            const long long col = (long long)cb * CB + c;
            valid = valid && col < s;
            base = (long long)b * n * s + col;
            step = s;
        } else {
            base = valid ? (long long)t * n : 0;
        }
        // per-point offsets in 32 bits from the tile's base pointer (n * s < 2^31, checked at launch): no 64-bit offset per point
        const V* ip = in + base;
        const unsigned ustep = (unsigned)step;
        V v[E];
#pragma unroll
        for (int k = 0; k < E; ++k) {
            const int idx = j + T * k;
            v[k] = (valid && idx < n) ? cmul(ip[(unsigned)idx * ustep], chirp[idx]) : V{0, 0};
        }
        run_stages<V, P, 0, +1, CB, KG::PAD, KG::WAVE_LOCAL, KG::TWMODE, TWPOW, KG::PH, 1, KG::NW, KG::LOCALX>(v, twr, lds, j, c);
        // A . B^, conjugated: the inverse transform is conj(FFT_M(conj(A . B^))) (1/M is in B^)
#pragma unroll
        for (int k = 0; k < E; ++k) v[k] = cconj(cmul(v[k], bhat[j + T * k]));
        group_sync<KG::WAVE_LOCAL>();  // the second transform's exchanges reuse the tile
        run_stages<V, P, 0, +1, CB, KG::PAD, KG::WAVE_LOCAL, KG::TWMODE, TWPOW, KG::PH, 1, KG::NW, KG::LOCALX>(v, twr, lds, j, c);
        if (valid) {
            V* op = out + base;
#pragma unroll
            for (int k = 0; k < E; ++k) {
                const int idx = j + T * k;
                if (idx < n) op[(unsigned)idx * ustep] = cscale(cmul(cconj(v[k]), chirp[idx]), sc);
            }
        }
        group_sync<KG::WAVE_LOCAL>();  // the next tile's exchanges reuse the tile
    }
}

template <class V, class P>
__global__ void __attribute__((amdgpu_flat_work_group_size(1, BsGeom<V, P, false>::KG::THREADS)))
bluestein_rows_kernel(const V* in, V* out, const typename VecTraits<V>::W* __restrict__ tw, const V* __restrict__ chirp,
                      const V* __restrict__ bhat, int n, unsigned rows, double scale) {
    bluestein_tiles<V, P, false>(in, out, tw, chirp, bhat, n, 1, rows, 1, scale);
}

template <class V, class P>
__global__ void __attribute__((amdgpu_flat_work_group_size(1, BsGeom<V, P, true>::KG::THREADS)))
bluestein_cols_kernel(const V* in, V* out, const typename VecTraits<V>::W* __restrict__ tw, const V* __restrict__ chirp,
                      const V* __restrict__ bhat, int n, long long s, unsigned tiles, unsigned tiles_per_b, double scale) {
    bluestein_tiles<V, P, true>(in, out, tw, chirp, bhat, n, s, tiles, tiles_per_b, scale);
}

template <class V, class P> hipError_t launch_bluestein(const FusedLaunch& F, hipStream_t stream) {
    using W = typename VecTraits<V>::W;
    static std::atomic<int> occ_rows[kMaxDevices], occ_cols[kMaxDevices];
    hipError_t              e;
    (void)hipGetLastError();
    if (F.s == 1) {
        using KG = typename BsGeom<V, P, false>::KG;
        constexpr int G = BsGeom<V, P, false>::G;
        if (F.batch >= (1ll << 31)) return hipErrorInvalidValue;
        const int occ = resident_blocks_per_cu(reinterpret_cast<const void*>(bluestein_rows_kernel<V, P>), KG::THREADS, KG::LDS_BYTES, occ_rows, &e);
        if (occ == 0) return e;
        const long long grid = persistent_grid(device_info().cus, occ, (F.batch + G - 1) / G);
        hipLaunchKernelGGL((bluestein_rows_kernel<V, P>), dim3((unsigned)grid), dim3(KG::THREADS), KG::LDS_BYTES, stream, (const V*)F.in,
                           (V*)F.out, (const W*)F.tw, (const V*)F.chirp, (const V*)F.bhat, F.n, (unsigned)F.batch, F.scale);
    } else {
        using KG = typename BsGeom<V, P, true>::KG;
        constexpr int   G = BsGeom<V, P, true>::G, CB = BsGeom<V, P, true>::CB;
        const long long per_b = (F.s + CB - 1) / CB, tiles = F.batch * per_b;
        if (tiles >= (1ll << 31) || (long long)F.n * F.s >= (1ll << 31)) return hipErrorInvalidValue;
        const int occ = resident_blocks_per_cu(reinterpret_cast<const void*>(bluestein_cols_kernel<V, P>), KG::THREADS, KG::LDS_BYTES, occ_cols, &e);
        if (occ == 0) return e;
        const long long grid = persistent_grid(device_info().cus, occ, (tiles + G - 1) / G);
        hipLaunchKernelGGL((bluestein_cols_kernel<V, P>), dim3((unsigned)grid), dim3(KG::THREADS), KG::LDS_BYTES, stream, (const V*)F.in,
                           (V*)F.out, (const W*)F.tw, (const V*)F.chirp, (const V*)F.bhat, F.n, F.s, (unsigned)tiles, (unsigned)per_b,
                           F.scale);
    }
    return hipGetLastError();
}

template <int N> hipError_t BsInst<true, N>::run(const FusedLaunch& F, hipStream_t stream) {
    if (F.dtype == F64) return launch_bluestein<double2, typename PlanFor<N>::type>(F, stream);
    if (F.dtype == F32) return launch_bluestein<float2, typename PlanFor<N>::type>(F, stream);
    return hipErrorInvalidValue;
}
#define DFFT_BS_INST(N, GRP, E, ...) template struct BsInst<(GRP == DFFT_INST_GROUP && N >= kFusedMinM), N>;
DFFT_PLAN_TABLE(DFFT_BS_INST)
#undef DFFT_BS_INST

#else  // the dispatcher, the multi-pass kernels and the tables

namespace {


template <class V> __device__ __forceinline__ V cmulb(V a, V b) { return V{a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x}; }

// scratch[b][m][c] = m < n ? in[b][m][c] * chirp[m] : 0      (e runs over batch * M * s)
template <class V>
__global__ void __launch_bounds__(256) bluestein_pad_kernel(const V* in, V* __restrict__ scratch, const V* __restrict__ chirp, long long n,
                                                            long long M, long long s, long long total) {
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
        const long long r = e / s, c = e - r * s;  // r = b * M + m
        const long long b = r / M, m = r - b * M;
        scratch[e] = m < n ? cmulb(in[(b * n + m) * s + c], chirp[m]) : V{0, 0};
    }
}

// scratch[b][m][c] *= B^[m]
template <class V>
__global__ void __launch_bounds__(256) bluestein_mul_kernel(V* __restrict__ scratch, const V* __restrict__ bhat, long long M, long long s,
                                                            long long total) {
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
        const long long m = (e / s) % M;
        scratch[e] = cmulb(scratch[e], bhat[m]);
    }
}

// out[b][k][c] = scale * chirp[k] * src[b][k][c] for k < n, src of M rows per batch item  (e runs over batch * n * s)
template <class V>
__global__ void __launch_bounds__(256) bluestein_finish_kernel(const V* src, V* out, const V* __restrict__ chirp, long long n, long long M,
                                                               long long s, long long total, typename real_of<V>::type scale) {
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
        const long long r = e / s, c = e - r * s;  // r = b * n + k
        const long long b = r / n, k = r - b * n;
        const V         v = cmulb(src[(b * M + k) * s + c], chirp[k]);
        out[e] = V{v.x * scale, v.y * scale};
    }
}

// M-point transforms of data[batch][M][s] on the single-pass kernels (M a tuned length <= 4096), in place
int single_pass(void* data, long long M, long long s, long long batch, int dtype, int dir, hipStream_t stream) {
    const void* tw = nullptr;
    int         rc = get_twiddles((int)M, dtype, &tw);
    if (rc) return rc;
    FftLaunch L;
    std::memset(&L, 0, sizeof(L));
    L.dtype = dtype;
    L.n = (int)M;
    L.dir = dir;
    L.in = data;
    L.out = data;
    L.tw = tw;
    if (s == 1) {
        L.cols = 0;
        L.imap = L.omap = AxisMap{(int)M, 1, 0, 1, 0, 0, 1, 0};
        L.itile = L.otile = TileMap{M, 0};
        L.ntiles = batch;
        L.tiles_per_a = 1;
        L.ncols = 1;
    } else {
        if (s >= (1ll << 31)) return fail(DFFT_EUNSUPPORTED, "Bluestein FFT: more than 2^31 columns");
        L.cols = 1;
        L.imap = L.omap = AxisMap{(int)M, 1, 0, s, 1, 0, 1, 0};
        L.itile = L.otile = TileMap{M * s, 1};
        L.na = batch;
        L.ncols = (int)s;
    }
    const hipError_t e = launch_fft(L, stream);
    if (e == hipSuccess) return DFFT_OK;
    return fail(e == hipErrorInvalidValue ? DFFT_EUNSUPPORTED : DFFT_EHIP, std::string("Bluestein FFT: ") + hipGetErrorString(e));
}

// M-point transforms in place on data[batch][M][s]; `lscr` (M > 4096 only) holds batch * M * s elements
int fft_m(void* data, long long M, long long s, long long batch, int dtype, int dir, void* lscr, hipStream_t stream) {
    if (M <= 4096) return single_pass(data, M, s, batch, dtype, dir, stream);
    return long_fft(data, data, M, s, batch, dtype, dir, 1.0, lscr, stream);
}

// every tuned single-pass length, ascending
const std::vector<int>& tuned_lengths() {
    static const std::vector<int> v = [] {
        std::vector<int> r = {
#define DFFT_BS_LEN(N, GRP, E, ...) N,
            DFFT_PLAN_TABLE(DFFT_BS_LEN)
#undef DFFT_BS_LEN
        };
        std::sort(r.begin(), r.end());
        return r;
    }();
    return v;
}

// every length long_split accepts (products of two tuned lengths in (4096, 2^24]), ascending
const std::vector<long long>& four_step_lengths() {
    static const std::vector<long long> v = [] {
        std::vector<long long> r;
        for (int a : tuned_lengths())
            for (int b : tuned_lengths()) {
                const long long m = (long long)a * b;
                if (a <= b && m > 4096 && m <= (1ll << 24)) r.push_back(m);
            }
        std::sort(r.begin(), r.end());
        r.erase(std::unique(r.begin(), r.end()), r.end());
        return r;
    }();
    return v;
}

struct BsKey {
    int       dev;
    long long n;
    int       dtype, dir;
    bool      operator<(const BsKey& o) const { return std::tie(dev, n, dtype, dir) < std::tie(o.dev, o.n, o.dtype, o.dir); }
};
std::mutex                         g_bs_mutex;
std::map<BsKey, BluesteinTablesPtr> g_bs;

template <class T> int upload(const std::vector<T>& h, void** dptr) {
    DFFT_HIP_TRY(hipMalloc(dptr, h.size() * sizeof(T)));
    DFFT_HIP_TRY(hipMemcpy(*dptr, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
    return DFFT_OK;
}

// B^ in fp64 on the device: b (host, extended precision rounded once) -> FFT_M with the library's forward transform, on a stream of its
// own, synchronised.  A zero transform in `dtype` warms the four-step tables of that precision, so that no later call builds them.
int build_bhat(BluesteinTables* t, const std::vector<double>& b) {
    const long long M = t->M;
    void*           d64 = nullptr;
    void*           lscr = nullptr;
    void*           warm = nullptr;
    hipStream_t     st = nullptr;
    int             rc = upload(b, &d64);
    auto            cleanup = [&]() {
        if (st) (void)hipStreamDestroy(st);
        if (lscr) (void)hipFree(lscr);
        if (warm) (void)hipFree(warm);
        if (d64 && d64 != t->bhat) (void)hipFree(d64);
    };
    if (rc == DFFT_OK && hipStreamCreateWithFlags(&st, hipStreamNonBlocking) != hipSuccess) rc = fail(DFFT_EHIP, "Bluestein tables: hipStreamCreate");
    if (rc == DFFT_OK && M > 4096 && hipMalloc(&lscr, (size_t)M * 16) != hipSuccess) rc = fail(DFFT_EHIP, "Bluestein tables: scratch");
    if (rc == DFFT_OK && M > 1) rc = fft_m(d64, M, 1, 1, DFFT_F64, DFFT_FORWARD, lscr, st);
    if (rc == DFFT_OK && M > 4096 && t->dtype == DFFT_F32) {
        if (hipMalloc(&warm, (size_t)M * 8) != hipSuccess || hipMemsetAsync(warm, 0, (size_t)M * 8, st) != hipSuccess)
            rc = fail(DFFT_EHIP, "Bluestein tables: warm-up buffer");
        if (rc == DFFT_OK) rc = fft_m(warm, M, 1, 1, DFFT_F32, DFFT_FORWARD, lscr, st);
    }
    if (rc == DFFT_OK && M <= 4096 && M > 1) {
        const void* tw = nullptr;
        rc = get_twiddles((int)M, t->dtype, &tw);  // the fused kernels' and the single-pass passes' table
    }
    if (rc == DFFT_OK && hipStreamSynchronize(st) != hipSuccess) rc = fail(DFFT_EHIP, "Bluestein tables: FFT of the chirp");
    if (rc == DFFT_OK) {
        if (t->dtype == DFFT_F64) {
            t->bhat = d64;
        } else {
            std::vector<double> h(2 * (size_t)M);
            std::vector<float>  f(2 * (size_t)M);
            if (hipMemcpy(h.data(), d64, h.size() * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) {
                rc = fail(DFFT_EHIP, "Bluestein tables: read-back");
            } else {
                for (size_t i = 0; i < h.size(); ++i) f[i] = (float)h[i];
                rc = upload(f, &t->bhat);
            }
        }
    }
    cleanup();
    return rc;
}

template <int N> hipError_t fused_run(const FusedLaunch& F, hipStream_t stream) {
    if constexpr (N >= kFusedMinM) return BsInst<true, N>::run(F, stream);
    else return hipErrorInvalidValue;
}

}  // namespace

BluesteinTables::~BluesteinTables() {
    if (chirp) (void)hipFree(chirp);
    if (bhat) (void)hipFree(bhat);
}

long long bluestein_padded_length(long long n) {
    if (n < 1 || n > kBluesteinMaxLength) return 0;
    if (n == 1) return 1;
    const long long need = 2 * n - 1;
    if (n <= kBluesteinFusedMaxLength) {
        for (int m : tuned_lengths())
            if (m >= need) return m;
        return 0;
    }
    const auto& v = four_step_lengths();
    auto        it = std::lower_bound(v.begin(), v.end(), need);
    return it == v.end() ? 0 : *it;
}

bool bluestein_fused_env() { return env_switch_on("DFFT_BLUESTEIN_FUSED"); }

int bluestein_tables(long long n, int dtype, int dir, BluesteinTablesPtr* out) {
    int dev = 0;
    DFFT_HIP_TRY(hipGetDevice(&dev));
    const long long M = bluestein_padded_length(n);
    if (!M || (dtype != DFFT_F64 && dtype != DFFT_F32) || (dir != DFFT_FORWARD && dir != DFFT_BACKWARD))
        return fail(DFFT_EUNSUPPORTED, "Bluestein tables: length " + std::to_string(n) + " is outside the Bluestein range");
    std::lock_guard<std::mutex> lk(g_bs_mutex);
    const BsKey                 key{dev, n, dtype, dir};
    auto                        it = g_bs.find(key);
    if (it != g_bs.end()) {
        *out = it->second;
        return DFFT_OK;
    }
    auto t = std::make_shared<BluesteinTables>();
    t->dev = dev;
    t->n = n;
    t->M = M;
    t->dtype = dtype;
    t->dir = dir;
    // c_m = exp(-d i pi q / n), q = m^2 mod 2n in 64-bit integers; angle and sincos in extended precision, rounded once
    const long double   pi = 3.141592653589793238462643383279502884L;
    std::vector<double> c(2 * (size_t)n), b(2 * (size_t)M, 0.0);
    const long double   inv_m = 1.0L / (long double)M;
    for (long long m = 0; m < n; ++m) {
        const long long   q = (m * m) % (2 * n);
        const long double a = pi * (long double)q / (long double)n;
        const long double cr = cosl(a), ci = -(long double)dir * sinl(a);
        c[2 * m] = (double)cr;
        c[2 * m + 1] = (double)ci;
        // b_m = b_{M-m} = conj(c_m) / M
        b[2 * m] = (double)(cr * inv_m);
        b[2 * m + 1] = (double)(-ci * inv_m);
        if (m > 0) {
            b[2 * (M - m)] = b[2 * m];
            b[2 * (M - m) + 1] = b[2 * m + 1];
        }
    }
    int rc;
    if (dtype == DFFT_F64) {
        rc = upload(c, &t->chirp);
    } else {
        std::vector<float> f(c.size());
        for (size_t i = 0; i < c.size(); ++i) f[i] = (float)c[i];
        rc = upload(f, &t->chirp);
    }
    if (rc == DFFT_OK) rc = build_bhat(t.get(), b);
    if (rc != DFFT_OK) return rc;
    g_bs[key] = t;
    *out = t;
    return DFFT_OK;
}

// Plan-less calls may still be running on the tables: each owning device is drained before the cache lets go of them (like
// long_scratch_trim); tables a plan holds are not freed here.
void bluestein_trim() {
    std::map<BsKey, BluesteinTablesPtr> old;
    {
        std::lock_guard<std::mutex> lk(g_bs_mutex);
        old.swap(g_bs);
    }
    int        cur = 0;
    const bool have_cur = hipGetDevice(&cur) == hipSuccess;
    int        last = -1;
    for (auto& kv : old) {
        if (kv.first.dev != last && hipSetDevice(kv.first.dev) == hipSuccess) (void)hipDeviceSynchronize();
        last = kv.first.dev;
        kv.second.reset();
    }
    (void)hipGetLastError();
    if (have_cur) (void)hipSetDevice(cur);
}

static size_t per_transform_bytes(const BluesteinTables& T, long long s) {
    return (size_t)T.M * (size_t)s * elem_bytes(T.dtype) * (T.M > 4096 ? 2 : 1);  // padded data (+ long_fft's scratch)
}

// The one-launch column kernel keeps a batch item's point offsets in 32 bits: n * s >= 2^31 runs the multi-pass form (as the real-column
// and r2r rules send that extent to their composed routes).  The decision never looks at the batch, so a scratch size asked for one
// chunk holds for every other; a one-launch call of 2^31 or more rows or column tiles (upwards of 170 GB) is turned down by launch_bluestein.
bool bluestein_runs_fused(long long n, long long s, bool fused) {
    return n == 1 || (fused && n <= kBluesteinFusedMaxLength && (s <= 1 || n * s < (1ll << 31)));
}
static bool runs_fused(const BluesteinTables& T, long long s, bool fused) { return bluestein_runs_fused(T.n, s, fused); }

size_t bluestein_scratch_bytes(const BluesteinTables& T, long long s, long long batch, bool fused, size_t cap) {
    if (runs_fused(T, s, fused) || batch <= 0 || s <= 0) return 0;
    const size_t per = per_transform_bytes(T, s);
    return (size_t)chunk_units(per, batch, cap) * per;
}

int bluestein_fft(const BluesteinTables& T, const void* in, void* out, long long s, long long batch, double scale, bool fused, void* scratch,
                  size_t scratch_bytes, hipStream_t stream) {
    if (batch <= 0 || s <= 0) return DFFT_OK;
    const double sc = scale == 0.0 ? 1.0 : scale;
    const bool   f64 = T.dtype == DFFT_F64;
    if (T.n == 1) {  // X_0 = x_0: a scaled copy
        const long long total = batch * s;
        (void)hipGetLastError();
        if (f64)
            hipLaunchKernelGGL(bluestein_finish_kernel<double2>, dim3(elementwise_grid(total)), dim3(256), 0, stream, (const double2*)in,
                               (double2*)out, (const double2*)T.chirp, 1ll, 1ll, s, total, sc);
        else
            hipLaunchKernelGGL(bluestein_finish_kernel<float2>, dim3(elementwise_grid(total)), dim3(256), 0, stream, (const float2*)in,
                               (float2*)out, (const float2*)T.chirp, 1ll, 1ll, s, total, (float)sc);
        DFFT_HIP_TRY(hipGetLastError());
        return DFFT_OK;
    }
    if (runs_fused(T, s, fused)) {
        FusedLaunch F;
        F.dtype = T.dtype;
        F.n = (int)T.n;
        F.s = s;
        F.batch = batch;
        F.in = in;
        F.out = out;
        F.chirp = T.chirp;
        F.bhat = T.bhat;
        F.scale = sc;
        int rc = get_twiddles((int)T.M, T.dtype, &F.tw);  // cached when the tables were built
        if (rc) return rc;
        hipError_t e = hipErrorInvalidValue;
        switch (T.M) {
#define DFFT_BS_CASE(N, GRP, E, ...) \
    case N: e = fused_run<N>(F, stream); break;
            DFFT_PLAN_TABLE(DFFT_BS_CASE)
#undef DFFT_BS_CASE
            default: break;
        }
        if (e == hipSuccess) return DFFT_OK;
        return fail(e == hipErrorInvalidValue ? DFFT_EUNSUPPORTED : DFFT_EHIP, std::string("Bluestein FFT (fused): ") + hipGetErrorString(e));
    }
    // multi-pass form, batch chunks that fit the scratch
    const size_t per = per_transform_bytes(T, s);
    if (!scratch || scratch_bytes < per) return fail(DFFT_EINVAL, "Bluestein FFT: scratch buffer too small");
    const long long chunk = std::min<long long>(batch, (long long)(scratch_bytes / per));
    const long long M = T.M, n = T.n;
    const size_t    eb = elem_bytes(T.dtype);
    void*           pad = scratch;
    void*           lscr = M > 4096 ? (char*)scratch + (size_t)chunk * M * s * eb : nullptr;
    for (long long b0 = 0; b0 < batch; b0 += chunk) {
        const long long nb = std::min(chunk, batch - b0);
        const char*     ip = (const char*)in + (size_t)b0 * n * s * eb;
        char*           op = (char*)out + (size_t)b0 * n * s * eb;
        const long long tp = nb * M * s, tf = nb * n * s;
        (void)hipGetLastError();
        if (f64)
            hipLaunchKernelGGL(bluestein_pad_kernel<double2>, dim3(elementwise_grid(tp)), dim3(256), 0, stream, (const double2*)ip, (double2*)pad,
                               (const double2*)T.chirp, n, M, s, tp);
        else
            hipLaunchKernelGGL(bluestein_pad_kernel<float2>, dim3(elementwise_grid(tp)), dim3(256), 0, stream, (const float2*)ip, (float2*)pad,
                               (const float2*)T.chirp, n, M, s, tp);
        DFFT_HIP_TRY(hipGetLastError());
        if (int rc = fft_m(pad, M, s, nb, T.dtype, DFFT_FORWARD, lscr, stream)) return rc;
        if (f64)
            hipLaunchKernelGGL(bluestein_mul_kernel<double2>, dim3(elementwise_grid(tp)), dim3(256), 0, stream, (double2*)pad, (const double2*)T.bhat,
                               M, s, tp);
        else
            hipLaunchKernelGGL(bluestein_mul_kernel<float2>, dim3(elementwise_grid(tp)), dim3(256), 0, stream, (float2*)pad, (const float2*)T.bhat,
                               M, s, tp);
        DFFT_HIP_TRY(hipGetLastError());
        if (int rc = fft_m(pad, M, s, nb, T.dtype, DFFT_BACKWARD, lscr, stream)) return rc;
        if (f64)
            hipLaunchKernelGGL(bluestein_finish_kernel<double2>, dim3(elementwise_grid(tf)), dim3(256), 0, stream, (const double2*)pad, (double2*)op,
                               (const double2*)T.chirp, n, M, s, tf, sc);
        else
            hipLaunchKernelGGL(bluestein_finish_kernel<float2>, dim3(elementwise_grid(tf)), dim3(256), 0, stream, (const float2*)pad, (float2*)op,
                               (const float2*)T.chirp, n, M, s, tf, (float)sc);
        DFFT_HIP_TRY(hipGetLastError());
    }
    return DFFT_OK;
}

#endif

}  // namespace dfft
