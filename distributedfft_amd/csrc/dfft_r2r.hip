// dfft_r2r.hip -- real-to-real transforms (DCT-II, DCT-III, DST-II, DST-III; unnormalised, scipy.fft norm=None / FFTW REDFT10, REDFT01,
// RODFT10, RODFT01) along the middle axis of reals [batch][n][s], for ANY n with an n-point complex transform, by the two-for-one method
// of dfft_real_cols.hip / dfft_real_pair.hip: two real sequences a, b -- adjacent columns 2c, 2c + 1 for s > 1, rows 2p, 2p + 1 for s = 1
// -- share ONE n-point complex transform.  Types I and IV are not built.
//
// With w_k = exp(-i pi k / 2n) (the quarter-wave table, R2rTable) and H = ceil(n / 2):
//   DCT-II   v[m] = x[2m] (m < H), v[n-1-m] = x[2m+1];  z = v_a + i v_b;  Z = FFT_n(z);  Zt_k = conj Z[(n-k) mod n];
//            y_a[k] = Re(w_k (Z_k + Zt_k)),  y_b[k] = Im(w_k (Z_k - Zt_k)).
//   DCT-III  P(X)[k] = conj(w_k) (X[k] - i X[n-k]), X[n] := 0;  Z = P(X_a) + i P(X_b);  z = unnormalised inverse FFT_n(Z);
//            y_a[2m] = Re z[m] (m < H), y_a[2m+1] = Re z[n-1-m];  y_b the same of Im z.
//   DST-II   = reverse(DCT-II(x (-1)^j)),  DST-III = (-1)^j DCT-III(reverse(X)): the sign and the reversal live in the load and store
//            address maps (a uniform run-time flag), so the DST kinds add no kernels and no passes.
// Type III of type II is 2n x.  The two sequences of a pair share one transform, so each one's rounding error is bounded relative to the
// pair's combined magnitude, not its own (a column 10^6 times smaller than its partner keeps an error of about 10^6 ulps of its own
// size).  An odd last column or row is paired with zeros and its partner's output is dropped: nothing outside the caller's data is read
// or written.
//
// Forms:
//   * s >= 2, n with a tuned single-pass plan (dfft_plans.h), n * s < 2^31: ONE launch of r2r2_kernel / r2r3_kernel on the column tiles
//     of dfft_real_cols.hip (CB adjacent column pairs of one batch item, at most 128 KiB of exchange tile and 512 threads, so the tile
//     holds all n points of its columns in natural order).  Every row load and store still covers CB adjacent column pairs -- the
//     permutation only reorders which rows a thread touches.  Where s is even and the buffers are aligned to a pair, a column pair is
//     loaded and stored as one two-element value (VEC), otherwise as two reals.  Per-point offsets are 32-bit within a batch item.
//   * s = 1, n with a tuned single-pass plan, odd or even: the same two kernels on the row geometry of dfft_real_pair.hip (one pair of
//     rows per thread group).
//   * every other n (run-time-scheduled, four-step, Bluestein), n * s >= 2^31, instantiations that would keep values in scratch memory
//     (r2r_fused_ok) and DFFT_R2R_FUSED=0: the composed route, per batch chunk of at most max(256 MiB, one item's or pair's) packed
//     pairs -- r2r_pre_kernel (permute / pre-twiddle, pack) into scratch, the n-point transform on the scratch exactly as real_cols /
//     real_pair_rows dispatch it (the C2C row / column launch, long_fft or bluestein_fft), r2r_post_kernel into `out`.
//
// In place (out == in): a fused tile owns its columns (rows) and has loaded ALL of their points before it stores any -- every load
// feeds run_stages (type II) or the exchange tile (type III), and every store follows a group barrier behind that use; tiles of different
// workgroups touch disjoint elements.  On the composed route the pre kernel of a chunk has read all of the chunk's points into scratch
// before the post kernel (stream-ordered behind it) writes them, and chunks are disjoint.  For the same reason neither kernel marks its
// real pointers __restrict__.
//
// Compiled once per instantiation group (-DDFFT_INST_GROUP=g: the fused kernels of the tuned lengths of group g) and once with
// -DDFFT_INST_GROUP=DFFT_NUM_INST_GROUPS (the dispatcher, the table cache and the pre / post kernels).
#include "dfft_fused_host.h"
#include "dfft_bluestein.h"
#include "dfft_long.h"
#include "dfft_r2r.h"

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

// One fused launch.  The address maps of both geometries: point r of sequence a of tile (item, pc) is in[item * istep + 2 pc + r * rs]
// (pc = 0 on the row geometry), its partner b lies `bd` reals further.
struct R2rFusedLaunch {
    int         dtype;
    int         kind;
    long long   s, batch;  // batch: items (columns) or rows (s = 1)
    bool        vec;       // s even, in and out aligned to two reals: a column pair is one two-element load / store
    const void* in;
    void*       out;
    const void* tw;
    const void* wq;
};

// Instantiations that would keep values in scratch memory at every tile width tried (tools/r2r_resources.py,
// profiles/r15/kernel_resources.txt) are not built: their (n, dtype, type, form) runs the composed route.
enum { R2R_FORM_COLS = 0, R2R_FORM_COLS_VEC = 1, R2R_FORM_ROWS = 2 };
constexpr bool r2r_fused_ok(int n, bool f64, bool three, int form) {
    if (f64 && three) {  // 20 ... 824 bytes per lane with the whole register file (one wave per SIMD) already theirs
        if ((n == 100 || n == 384 || n == 400 || n == 3125) && (form == R2R_FORM_COLS || form == R2R_FORM_ROWS)) return false;
        if (n == 1536 && form == R2R_FORM_ROWS) return false;
    }
    if (f64 && !three) {  // 116 and 52 bytes per lane
        if (n == 2048 && form == R2R_FORM_COLS) return false;
        if (n == 3125 && form == R2R_FORM_ROWS) return false;
    }
    if (!f64 && three && n == 3125 && form == R2R_FORM_ROWS) return false;  // 628 bytes per lane
    return true;
}

// the family (dfft_fused_host.h); run<N>: defined in the translation unit of N's group only
struct R2rTag {
    using Launch = R2rFusedLaunch;
    static constexpr bool ok(int n, bool f64, bool three, int form) { return r2r_fused_ok(n, f64, three, form); }
    template <int N> static hipError_t run(const Launch& F, hipStream_t stream);
};

#if DFFT_INST_GROUP < DFFT_NUM_INST_GROUPS

// Column tiles as dfft_real_cols.hip sizes them: the C2C column kernel's width, halved until the tile holds at most 128 KiB (the split
// step needs all n points of its columns in the exchange tile at once) and the workgroup at most 512 threads, 256 for the lengths
// that kept values in scratch memory at 512.
template <class V, class P, bool THREE> constexpr int r2r_max_threads() {
    constexpr bool f64 = sizeof(V) == 16;
    constexpr int  N = P::N;
    if (f64 ? (N == 1024 || N == 4096) : (N == 400 || N == 640 || N == 1280 || N == 1536 || N == 3125 || N == 4096)) return 256;
    // the type III kernels of these kept 20 ... 308 bytes per lane in scratch at 512 threads
    if (THREE && (f64 ? (N == 768 || N == 1000 || N == 2048 || N == 2187) : (N == 1024 || N == 2048))) return 256;
    return 512;
}
template <class V, class P, bool THREE> constexpr int r2r_cols_per_tile() {
    int cb = cols_per_tile<V, P>();
    while (cb > 1 && ((long long)P::N * cb * (long long)sizeof(V) > 128 * 1024 || cb * P::T > r2r_max_threads<V, P, THREE>())) cb /= 2;
    return cb;
}
template <class V, class P, bool THREE> struct R2rColsGeom {
    static constexpr bool ROWS = false;
    static constexpr int  CB = r2r_cols_per_tile<V, P, THREE>();
    static constexpr int  G = ConstMax1<256 / (CB * P::T)>::value;
    using KG = KernelGeom<V, P, CB, G, TuneDefault>;
    static_assert(KG::PH == 1, "the split step needs the whole tile in the LDS");
    static constexpr int    SPLIT = (KG::PAD ? P::N + P::N / 8 : P::N) * CB;  // > lds_index<CB, PAD>(N - 1, CB - 1)
    static constexpr int    EXR = ((KG::LDS_ELEMS > SPLIT ? KG::LDS_ELEMS : SPLIT) + 1) / 2 * 2;
    static constexpr size_t LDS_BYTES = (size_t)EXR * G * sizeof(V) + KG::TW_BYTES;
};
// Row tiles as dfft_real_pair.hip has them: one pair of rows per thread group, about 256 threads per workgroup
template <class V, class P, bool THREE> struct R2rRowsGeom {
    static constexpr bool ROWS = true;
    static constexpr int  CB = 1;
    static constexpr int  G = ConstMax1<256 / P::T>::value;
    using KG = KernelGeom<V, P, 1, G, TuneDefault>;
    static_assert(KG::PH == 1, "the split step needs the whole tile in the LDS");
    static constexpr int    SPLIT = KG::PAD ? P::N + P::N / 8 : P::N;
    static constexpr int    EXR = ((KG::LDS_ELEMS > SPLIT ? KG::LDS_ELEMS : SPLIT) + 1) / 2 * 2;
    static constexpr size_t LDS_BYTES = (size_t)EXR * G * sizeof(V) + KG::TW_BYTES;
};

// What a kernel needs besides the pointers (one by-value argument)
struct R2rTileArgs {
    long long istep;        // reals from one tile owner (batch item / row pair) to the next
    long long s;            // columns: reals per row;  rows: the number of rows
    unsigned  rs, bd;       // reals from one point to the next, and from sequence a to sequence b
    unsigned  tiles, tiles_per_b;
    int       dst;          // 0: DCT, 1: DST
};

// row of the caller's axis that position m of the permuted sequence v holds: 2m for m < H, 2 (n-1-m) + 1 above
template <int N> __device__ __forceinline__ int r2r_perm(int m) { return m < (N + 1) / 2 ? 2 * m : 2 * (N - 1 - m) + 1; }

// Types II (DCT-II, DST-II).  Tile t = (owner b, block of CB column pairs); VEC (columns only): column pair pc is the two-element value
// pc of a row of s / 2.
template <class V, class P, class GEO, bool VEC>
__global__ void __attribute__((amdgpu_flat_work_group_size(1, GEO::KG::THREADS)))
r2r2_kernel(const typename real_of<V>::type* in, typename real_of<V>::type* out, const typename VecTraits<V>::W* __restrict__ tw,
            const V* __restrict__ wq, const R2rTileArgs A) {
    using KG = typename GEO::KG;
    using W = typename VecTraits<V>::W;
    using RT = typename real_of<V>::type;
    constexpr int  E = P::E, T = P::T, N = P::N, G = GEO::G, GT = KG::GT, CB = GEO::CB, H = (N + 1) / 2;
    constexpr bool TWPOW = KG::TWMODE == TW_REG;
    static_assert(!(VEC && GEO::ROWS), "rows have no two-element access");
    extern __shared__ __attribute__((aligned(16))) char dfft_smem[];
    const int g = threadIdx.x / GT;
    const int tid = (int)threadIdx.x - g * GT;
    const int c = tid % CB;
    const int j = tile_j<CB, KG::NW>(tid);
    V*        lds = reinterpret_cast<V*>(dfft_smem + KG::TW_BYTES) + g * GEO::EXR;
    W         twreg[KG::TWMODE == TW_REG && KG::TWN > 0 ? KG::TWN : 1];
    const W*  twr = stage_twiddles<V, P, +1, KG>(twreg, reinterpret_cast<W*>(dfft_smem), tw, j);
    const long long sp = GEO::ROWS ? 1 : (A.s + 1) / 2;
    const bool      dst = A.dst != 0;
    for (unsigned r0 = blockIdx.x * G; r0 < A.tiles; r0 += gridDim.x * G) {
        const unsigned  t = r0 + g;
        const unsigned  b = t < A.tiles ? t / A.tiles_per_b : 0u, cb = t < A.tiles ? t - b * A.tiles_per_b : 0u;
        const long long pc = (long long)cb * CB + c;
        const bool      va = t < A.tiles && pc < sp;
        const bool      vb = va && (GEO::ROWS ? 2ll * b + 1 < A.s : 2 * pc + 1 < A.s);
        const long long base = (long long)b * A.istep + (GEO::ROWS ? 0 : 2 * pc);
        // per-point offsets in 32 bits from the tile's base pointer (n * s < 2^31, checked on the host)
        V v[E];
        if constexpr (VEC) {
            const V*       ip = reinterpret_cast<const V*>(in) + (va ? base / 2 : 0);
            const unsigned uh = A.rs / 2;
#pragma unroll
            for (int k = 0; k < E; ++k) {
                const int m = j + T * k;
                V         x = va ? ip[(unsigned)r2r_perm<N>(m) * uh] : V{0, 0};
                if (dst && m >= H) x = V{-x.x, -x.y};
                v[k] = x;
            }
        } else {
            const RT* ip = in + (va ? base : 0);
#pragma unroll
            for (int k = 0; k < E; ++k) {
                const int      m = j + T * k;
                const unsigned o = (unsigned)r2r_perm<N>(m) * A.rs;
                V              x = V{va ? ip[o] : (RT)0, vb ? ip[o + A.bd] : (RT)0};
                if (dst && m >= H) x = V{-x.x, -x.y};
                v[k] = x;
            }
        }
        run_stages<V, P, 0, +1, CB, KG::PAD, KG::WAVE_LOCAL, KG::TWMODE, TWPOW, KG::PH, 1, KG::NW, KG::LOCALX>(v, twr, lds, j, c);
        group_sync<KG::WAVE_LOCAL>();
#pragma unroll
        for (int k = 0; k < E; ++k) lds[lds_index<CB, KG::PAD>(j + T * k, c)] = v[k];
        group_sync<KG::WAVE_LOCAL>();
        if (va) {
#pragma unroll
            for (int k = 0; k < E; ++k) {
                const int kk = j + T * k, km = kk == 0 ? 0 : N - kk;
                const V   zm = lds[lds_index<CB, KG::PAD>(km, c)];
                const V   w = wq[kk];
                // y_a = Re(w (Z + conj Zm)), y_b = Im(w (Z - conj Zm))
                const RT       ya = w.x * (v[k].x + zm.x) - w.y * (v[k].y - zm.y);
                const RT       yb = w.x * (v[k].y + zm.y) + w.y * (v[k].x - zm.x);
                const unsigned row = (unsigned)(dst ? N - 1 - kk : kk);
                if constexpr (VEC) {
                    reinterpret_cast<V*>(out)[base / 2 + row * (A.rs / 2)] = V{ya, yb};
                } else {
                    RT* op = out + base;
                    op[row * A.rs] = ya;
                    if (vb) op[row * A.rs + A.bd] = yb;
                }
            }
        }
        group_sync<KG::WAVE_LOCAL>();  // the next tile's exchanges reuse the tile
    }
}

// Types III (DCT-III, DST-III)
template <class V, class P, class GEO, bool VEC>
__global__ void __attribute__((amdgpu_flat_work_group_size(1, GEO::KG::THREADS)))
r2r3_kernel(const typename real_of<V>::type* in, typename real_of<V>::type* out, const typename VecTraits<V>::W* __restrict__ tw,
            const V* __restrict__ wq, const R2rTileArgs A) {
    using KG = typename GEO::KG;
    using W = typename VecTraits<V>::W;
    using RT = typename real_of<V>::type;
    constexpr int  E = P::E, T = P::T, N = P::N, G = GEO::G, GT = KG::GT, CB = GEO::CB, H = (N + 1) / 2;
    constexpr bool TWPOW = KG::TWMODE == TW_REG;
    static_assert(!(VEC && GEO::ROWS), "rows have no two-element access");
    extern __shared__ __attribute__((aligned(16))) char dfft_smem[];
    const int g = threadIdx.x / GT;
    const int tid = (int)threadIdx.x - g * GT;
    const int c = tid % CB;
    const int j = tile_j<CB, KG::NW>(tid);
    V*        lds = reinterpret_cast<V*>(dfft_smem + KG::TW_BYTES) + g * GEO::EXR;
    W         twreg[KG::TWMODE == TW_REG && KG::TWN > 0 ? KG::TWN : 1];
    const W*  twr = stage_twiddles<V, P, -1, KG>(twreg, reinterpret_cast<W*>(dfft_smem), tw, j);
    const long long sp = GEO::ROWS ? 1 : (A.s + 1) / 2;
    const bool      dst = A.dst != 0;
    for (unsigned r0 = blockIdx.x * G; r0 < A.tiles; r0 += gridDim.x * G) {
        const unsigned  t = r0 + g;
        const unsigned  b = t < A.tiles ? t / A.tiles_per_b : 0u, cb = t < A.tiles ? t - b * A.tiles_per_b : 0u;
        const long long pc = (long long)cb * CB + c;
        const bool      va = t < A.tiles && pc < sp;
        const bool      vb = va && (GEO::ROWS ? 2ll * b + 1 < A.s : 2 * pc + 1 < A.s);
        const long long base = (long long)b * A.istep + (GEO::ROWS ? 0 : 2 * pc);
        V               v[E];
        // X_a[kk] + i X_b[kk] (DST: the reversed sequence) into the tile in natural order
        if constexpr (VEC) {
            const V*       ip = reinterpret_cast<const V*>(in) + (va ? base / 2 : 0);
            const unsigned uh = A.rs / 2;
#pragma unroll
            for (int k = 0; k < E; ++k) {
                const int kk = j + T * k;
                v[k] = va ? ip[(unsigned)(dst ? N - 1 - kk : kk) * uh] : V{0, 0};
            }
        } else {
            const RT* ip = in + (va ? base : 0);
#pragma unroll
            for (int k = 0; k < E; ++k) {
                const int      kk = j + T * k;
                const unsigned o = (unsigned)(dst ? N - 1 - kk : kk) * A.rs;
                v[k] = V{va ? ip[o] : (RT)0, vb ? ip[o + A.bd] : (RT)0};
            }
        }
        group_sync<KG::WAVE_LOCAL>();  // the previous tile's stages are done with the tile
#pragma unroll
        for (int k = 0; k < E; ++k) lds[lds_index<CB, KG::PAD>(j + T * k, c)] = v[k];
        group_sync<KG::WAVE_LOCAL>();
        // Z[kk] = P(X_a)[kk] + i P(X_b)[kk],  P(X)[k] = conj(w_k) (X[k] - i X[n-k]),  X[n] = 0
#pragma unroll
        for (int k = 0; k < E; ++k) {
            const int kk = j + T * k;
            const V   xm = lds[lds_index<CB, KG::PAD>(kk == 0 ? 0 : N - kk, c)];
            const V   w = wq[kk];
            const RT  p = v[k].x + (kk == 0 ? (RT)0 : xm.y), q = (kk == 0 ? (RT)0 : xm.x) - v[k].y;
            v[k] = V{w.x * p - w.y * q, -w.y * p - w.x * q};
        }
        group_sync<KG::WAVE_LOCAL>();  // every partner is read before the stages reuse the tile
        run_stages<V, P, 0, -1, CB, KG::PAD, KG::WAVE_LOCAL, KG::TWMODE, TWPOW, KG::PH, 1, KG::NW, KG::LOCALX>(v, twr, lds, j, c);
        if (va) {
#pragma unroll
            for (int k = 0; k < E; ++k) {
                const int      m = j + T * k;
                const unsigned row = (unsigned)r2r_perm<N>(m);
                V              y = v[k];
                if (dst && m >= H) y = V{-y.x, -y.y};
                if constexpr (VEC) {
                    reinterpret_cast<V*>(out)[base / 2 + row * (A.rs / 2)] = y;
                } else {
                    RT* op = out + base;
                    op[row * A.rs] = y.x;
                    if (vb) op[row * A.rs + A.bd] = y.y;
                }
            }
        }
    }
}

template <class V, class P, class GEO, bool VEC, bool THREE> hipError_t launch_r2r_plan(const R2rFusedLaunch& F, hipStream_t stream) {
    using W = typename VecTraits<V>::W;
    using RT = typename real_of<V>::type;
    constexpr int           N = P::N;
    static std::atomic<int> blocks_per_cu[kMaxDevices];
    constexpr bool          three = THREE;
    const void*             kern = nullptr;
    if constexpr (three) kern = reinterpret_cast<const void*>(r2r3_kernel<V, P, GEO, VEC>);
    else kern = reinterpret_cast<const void*>(r2r2_kernel<V, P, GEO, VEC>);
    hipError_t              e;
    const int               bpc = resident_blocks_per_cu(kern, GEO::KG::THREADS, GEO::LDS_BYTES, blocks_per_cu, &e);
    if (bpc == 0) return e;
    // owners: batch items of [n][s] (columns), or pairs of rows (two rows of n reals each)
    const long long owners = GEO::ROWS ? (F.batch + 1) / 2 : F.batch;
    const long long per_b = GEO::ROWS ? 1 : ((F.s + 1) / 2 + GEO::CB - 1) / GEO::CB;
    const long long max_b = std::max(1ll, ((1ll << 30) - 1) / per_b);  // tile indices stay below 2^30 per launch
    const long long step = GEO::ROWS ? 2ll * N : (long long)N * F.s;
    (void)hipGetLastError();
    for (long long b0 = 0; b0 < owners; b0 += max_b) {
        const long long nb = std::min(max_b, owners - b0), tiles = nb * per_b;
        const long long grid = std::max(1ll, persistent_grid(device_info().cus, bpc, (tiles + GEO::G - 1) / GEO::G));
        R2rTileArgs A;
        A.istep = step;
        A.s = GEO::ROWS ? F.batch - 2 * b0 : F.s;
        A.rs = GEO::ROWS ? 1u : (unsigned)F.s;
        A.bd = GEO::ROWS ? (unsigned)N : 1u;
        A.tiles = (unsigned)tiles;
        A.tiles_per_b = (unsigned)per_b;
        A.dst = (F.kind == R2R_DST2 || F.kind == R2R_DST3) ? 1 : 0;
        const RT* ip = (const RT*)F.in + b0 * step;
        RT*       op = (RT*)F.out + b0 * step;
        if constexpr (three)
            hipLaunchKernelGGL((r2r3_kernel<V, P, GEO, VEC>), dim3((unsigned)grid), dim3(GEO::KG::THREADS), GEO::LDS_BYTES, stream, ip, op, (const W*)F.tw,
                               (const V*)F.wq, A);
        else
            hipLaunchKernelGGL((r2r2_kernel<V, P, GEO, VEC>), dim3((unsigned)grid), dim3(GEO::KG::THREADS), GEO::LDS_BYTES, stream, ip, op, (const W*)F.tw,
                               (const V*)F.wq, A);
        e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

template <class V, int N, bool THREE> hipError_t r2r_run_typed(const R2rFusedLaunch& F, hipStream_t stream) {
    using P = typename PlanFor<N>::type;
    constexpr bool f64 = sizeof(V) == 16;
    if (F.s == 1) {
        if constexpr (r2r_fused_ok(N, f64, THREE, R2R_FORM_ROWS)) return launch_r2r_plan<V, P, R2rRowsGeom<V, P, THREE>, false, THREE>(F, stream);
    } else if (F.vec) {
        if constexpr (r2r_fused_ok(N, f64, THREE, R2R_FORM_COLS_VEC)) return launch_r2r_plan<V, P, R2rColsGeom<V, P, THREE>, true, THREE>(F, stream);
    } else {
        if constexpr (r2r_fused_ok(N, f64, THREE, R2R_FORM_COLS)) return launch_r2r_plan<V, P, R2rColsGeom<V, P, THREE>, false, THREE>(F, stream);
    }
    return hipErrorInvalidValue;  // not built (r2r_fused_ok): the dispatcher does not come here
}
template <int N> hipError_t R2rTag::run(const R2rFusedLaunch& F, hipStream_t stream) {
    const bool three = F.kind == R2R_DCT3 || F.kind == R2R_DST3;
    if (F.dtype == F64) return three ? r2r_run_typed<double2, N, true>(F, stream) : r2r_run_typed<double2, N, false>(F, stream);
    if (F.dtype == F32) return three ? r2r_run_typed<float2, N, true>(F, stream) : r2r_run_typed<float2, N, false>(F, stream);
    return hipErrorInvalidValue;
}
DFFT_FUSED_INSTANTIATE(R2rTag)

#else  // the dispatcher, the table cache, and the kernels of the composed route

// Address map of the composed route's kernels: packed pair (u, k, pc) of z [units][n][sp] <-> reals in[u * istep + 2 pc + row * rs]
// (+ bd for sequence b), u = batch item (columns) or row pair (rows, sp = 1); lim = s (columns) or the number of rows of the chunk.
struct R2rMap {
    long long n, sp, total;  // total = units * n * sp
    long long istep, rs, bd, lim;
    int       rows, vec, three, dst;
};

__device__ __forceinline__ long long r2r_perm_rt(long long m, long long n) { return m < (n + 1) / 2 ? 2 * m : 2 * (n - 1 - m) + 1; }

// type II: z[u][m][pc] = (+-) (x_a[perm m] + i x_b[perm m]);  type III: z[u][k][pc] = P(X_a)[k] + i P(X_b)[k]
template <class V>
__global__ void __launch_bounds__(256) r2r_pre_kernel(const typename real_of<V>::type* in, V* __restrict__ z, const V* __restrict__ wq, const R2rMap M) {
    using RT = typename real_of<V>::type;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < M.total; e += (long long)gridDim.x * 256) {
        const long long r = e / M.sp, pc = e - r * M.sp;
        const long long u = r / M.n, k = r - u * M.n;
        const bool      vb = M.rows ? 2 * u + 1 < M.lim : 2 * pc + 1 < M.lim;
        const long long base = u * M.istep + (M.rows ? 0 : 2 * pc);
        auto            pair_at = [&](long long row) -> V {
            if (M.vec) return reinterpret_cast<const V*>(in)[(base + row * M.rs) / 2];  // 16-byte (fp64) / 8-byte (fp32) loads
            const RT* ip = in + base + row * M.rs;
            return V{ip[0], vb ? ip[M.bd] : (RT)0};
        };
        if (!M.three) {
            V x = pair_at(r2r_perm_rt(k, M.n));
            if (M.dst && k >= (M.n + 1) / 2) x = V{-x.x, -x.y};
            z[e] = x;
        } else {
            const V  x = pair_at(M.dst ? M.n - 1 - k : k);
            const V  xm = k == 0 ? V{0, 0} : pair_at(M.dst ? k - 1 : M.n - k);
            const V  w = wq[k];
            const RT p = x.x + xm.y, q = xm.x - x.y;
            z[e] = V{w.x * p - w.y * q, -w.y * p - w.x * q};
        }
    }
}

// type II: y[k] from Z[k] and Z[n-k];  type III: y[perm m] = (+-) z[m]
template <class V>
__global__ void __launch_bounds__(256) r2r_post_kernel(const V* __restrict__ z, typename real_of<V>::type* out, const V* __restrict__ wq, const R2rMap M) {
    using RT = typename real_of<V>::type;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < M.total; e += (long long)gridDim.x * 256) {
        const long long r = e / M.sp, pc = e - r * M.sp;
        const long long u = r / M.n, k = r - u * M.n;
        const bool      vb = M.rows ? 2 * u + 1 < M.lim : 2 * pc + 1 < M.lim;
        const long long base = u * M.istep + (M.rows ? 0 : 2 * pc);
        long long       row;
        V               y;
        if (!M.three) {
            const V zk = z[e], zm = z[(u * M.n + (k == 0 ? 0 : M.n - k)) * M.sp + pc];
            const V w = wq[k];
            y = V{w.x * (zk.x + zm.x) - w.y * (zk.y - zm.y), w.x * (zk.y + zm.y) + w.y * (zk.x - zm.x)};
            row = M.dst ? M.n - 1 - k : k;
        } else {
            y = z[e];
            if (M.dst && k >= (M.n + 1) / 2) y = V{-y.x, -y.y};
            row = r2r_perm_rt(k, M.n);
        }
        if (M.vec) {
            reinterpret_cast<V*>(out)[(base + row * M.rs) / 2] = y;
        } else {
            RT* op = out + base + row * M.rs;
            op[0] = y.x;
            if (vb) op[M.bd] = y.y;
        }
    }
}

namespace {

bool tuned_length(long long n, int dtype, bool three, int form) { return tuned_built<R2rTag>(n, dtype == F64, three, form); }

// units (batch items, or row pairs at s = 1) and packed pairs per row of a unit
long long r2r_units(long long s, long long batch) { return s == 1 ? (batch + 1) / 2 : batch; }
long long r2r_sp(long long s) { return s == 1 ? 1 : (s + 1) / 2; }

// units per chunk of the composed route (their packed pairs within max(256 MiB, one unit's)), and the scratch such a chunk needs
long long r2r_chunk_units(long long n, long long sp, int dtype, long long units, size_t cap) {
    const size_t zb = (size_t)n * sp * elem_bytes(dtype);
    return chunk_units(zb, units, cap);
}
size_t chunk_bytes(long long n, long long sp, int dtype, long long nu, const BluesteinTables* T, bool bs_fused, size_t cap) {
    const size_t zb = (size_t)nu * n * sp * elem_bytes(dtype);
    if (T) return zb + bluestein_scratch_bytes(*T, sp, nu, bs_fused, cap);
    return n > 4096 ? 2 * zb : zb;  // four-step: long_fft's scratch as large as its data
}

// n-point transforms down the sp columns of the nu units of z [nu][n][sp], in place
int r2r_fft(void* z, long long n, long long sp, long long nu, int dtype, int dir, const BluesteinTables* T, bool bs_fused, void* inner,
            size_t inner_bytes, hipStream_t stream) {
    if (T) return bluestein_fft(*T, z, z, sp, nu, 1.0, bs_fused, inner, inner_bytes, stream);
    if (n > 4096) return long_fft(z, z, n, sp, nu, dtype, dir, 1.0, inner, stream);
    // single-pass lengths: the entry points' own launches (they take no scratch for n <= 4096)
    return sp == 1 ? dfft_fft1d_rows(z, z, n, nu, dtype, dir, stream) : dfft_fft1d_cols(z, z, n, sp, nu, dtype, dir, stream);
}

template <class V>
int r2r_chunk(const R2rLaunch& L, const R2rTable& Wt, long long u0, long long nu, const BluesteinTables* T, bool bs_fused, void* z, void* inner,
              size_t inner_bytes, hipStream_t stream) {
    using RT = typename real_of<V>::type;
    const bool rows = L.s == 1;
    R2rMap     M;
    std::memset(&M, 0, sizeof(M));
    M.n = L.n;
    M.sp = r2r_sp(L.s);
    M.total = nu * L.n * M.sp;
    M.istep = rows ? 2 * L.n : L.n * L.s;
    M.rs = rows ? 1 : L.s;
    M.bd = rows ? L.n : 1;
    M.lim = rows ? L.batch - 2 * u0 : L.s;
    M.rows = rows ? 1 : 0;
    M.three = (L.kind == R2R_DCT3 || L.kind == R2R_DST3) ? 1 : 0;
    M.dst = (L.kind == R2R_DST2 || L.kind == R2R_DST3) ? 1 : 0;
    M.vec = (!rows && L.s % 2 == 0 && (uintptr_t)L.in % sizeof(V) == 0 && (uintptr_t)L.out % sizeof(V) == 0) ? 1 : 0;
    const RT* in = (const RT*)L.in + u0 * M.istep;
    RT*       out = (RT*)L.out + u0 * M.istep;
    (void)hipGetLastError();
    hipLaunchKernelGGL(r2r_pre_kernel<V>, dim3(elementwise_grid(M.total)), dim3(256), 0, stream, in, (V*)z, (const V*)Wt.w, M);
    DFFT_HIP_TRY(hipGetLastError());
    if (int rc = r2r_fft(z, L.n, M.sp, nu, L.dtype, M.three ? -1 : +1, T, bs_fused, inner, inner_bytes, stream)) return rc;
    hipLaunchKernelGGL(r2r_post_kernel<V>, dim3(elementwise_grid(M.total)), dim3(256), 0, stream, (const V*)z, out, (const V*)Wt.w, M);
    DFFT_HIP_TRY(hipGetLastError());
    return DFFT_OK;
}

struct R2rKey {
    int       dev;
    long long n;
    int       dtype;
    bool      operator<(const R2rKey& o) const { return std::tie(dev, n, dtype) < std::tie(o.dev, o.n, o.dtype); }
};
std::mutex                    g_r2r_mutex;
std::map<R2rKey, R2rTablePtr> g_r2r;

}  // namespace

R2rTable::~R2rTable() {
    if (w) (void)hipFree(w);
}

int r2r_table(long long n, int dtype, R2rTablePtr* out) {
    int dev = 0;
    DFFT_HIP_TRY(hipGetDevice(&dev));
    if (n < 1 || (dtype != F64 && dtype != F32)) return fail(DFFT_EINVAL, "r2r table: bad arguments");
    std::lock_guard<std::mutex> lk(g_r2r_mutex);
    const R2rKey                key{dev, n, dtype};
    auto                        it = g_r2r.find(key);
    if (it != g_r2r.end()) {
        *out = it->second;
        return DFFT_OK;
    }
    auto t = std::make_shared<R2rTable>();
    t->dev = dev;
    t->n = n;
    t->dtype = dtype;
    // w_k = exp(-i pi k / 2n): angle and sincos in extended precision, rounded once
    const long double   pi = 3.141592653589793238462643383279502884L;
    std::vector<double> w(2 * (size_t)n);
    for (long long k = 0; k < n; ++k) {
        const long double a = pi * (long double)k / (long double)(2 * n);
        w[2 * k] = (double)cosl(a);
        w[2 * k + 1] = (double)-sinl(a);
    }
    if (dtype == F64) {
        DFFT_HIP_TRY(hipMalloc(&t->w, w.size() * sizeof(double)));
        DFFT_HIP_TRY(hipMemcpy(t->w, w.data(), w.size() * sizeof(double), hipMemcpyHostToDevice));
    } else {
        std::vector<float> f(w.size());
        for (size_t i = 0; i < w.size(); ++i) f[i] = (float)w[i];
        DFFT_HIP_TRY(hipMalloc(&t->w, f.size() * sizeof(float)));
        DFFT_HIP_TRY(hipMemcpy(t->w, f.data(), f.size() * sizeof(float), hipMemcpyHostToDevice));
    }
    g_r2r[key] = t;
    *out = t;
    return DFFT_OK;
}

// Plan-less calls may still be running on the tables: each owning device is drained before the cache lets go of them (bluestein_trim)
void r2r_trim() {
    std::map<R2rKey, R2rTablePtr> old;
    {
        std::lock_guard<std::mutex> lk(g_r2r_mutex);
        old.swap(g_r2r);
    }
    if (old.empty()) return;
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

bool r2r_fused_env() { return env_switch_on("DFFT_R2R_FUSED"); }

// Fused lengths that run the composed route because it measured at least as fast (fused / composed time >= 1.0,
// profiles/r15/README.md).  None recorded: not measured yet.
static bool composed_faster(long long n, long long s, int dtype) {
    (void)n;
    (void)s;
    (void)dtype;
    return false;
}

bool r2r_fused(long long n, long long s, int dtype, int kind, bool vec) {
    const bool three = kind == R2R_DCT3 || kind == R2R_DST3;
    const int  form = s == 1 ? R2R_FORM_ROWS : (vec ? R2R_FORM_COLS_VEC : R2R_FORM_COLS);
    return s >= 1 && tuned_length(n, dtype, three, form) && (s == 1 || n * s < (1ll << 31)) && !composed_faster(n, s, dtype);
}
bool r2r_vec(const void* in, const void* out, long long s, int dtype) {
    return s > 1 && s % 2 == 0 && (uintptr_t)in % elem_bytes(dtype) == 0 && (uintptr_t)out % elem_bytes(dtype) == 0;
}

size_t r2r_scratch_bytes(const R2rLaunch& L, bool fused_on, const BluesteinTables* T, bool bluestein_fused, size_t cap) {
    const long long n = L.n, s = L.s, batch = L.batch;
    const int       dtype = L.dtype;
    if (n < 1 || s < 1 || batch <= 0 || (fused_on && r2r_fused(n, s, dtype, L.kind, r2r_vec(L.in, L.out, s, dtype)))) return 0;
    const long long sp = r2r_sp(s);
    return chunk_bytes(n, sp, dtype, r2r_chunk_units(n, sp, dtype, r2r_units(s, batch), cap), T, bluestein_fused, cap);
}

int r2r(const R2rLaunch& L, const R2rTable& Wt, bool fused_on, const BluesteinTables* T, bool bluestein_fused, size_t cap, void* scratch, size_t scratch_bytes,
        hipStream_t stream) {
    if (L.n < 1 || L.s < 1 || L.batch < 0 || L.kind < R2R_DCT2 || L.kind > R2R_DST3 || (L.dtype != F64 && L.dtype != F32) || !L.in || !L.out)
        return fail(DFFT_EINVAL, "r2r: bad arguments");
    if (L.batch == 0) return DFFT_OK;
    const bool three = L.kind == R2R_DCT3 || L.kind == R2R_DST3;
    if (Wt.n != L.n || Wt.dtype != L.dtype || !Wt.w) return fail(DFFT_EINVAL, "r2r: quarter-wave table of another transform");
    if (T && (T->n != L.n || T->dtype != L.dtype || T->dir != (three ? -1 : 1))) return fail(DFFT_EINVAL, "r2r: Bluestein tables of another transform");
    if (fused_on && r2r_fused(L.n, L.s, L.dtype, L.kind, r2r_vec(L.in, L.out, L.s, L.dtype))) {
        R2rFusedLaunch F;
        std::memset(&F, 0, sizeof(F));
        F.dtype = L.dtype;
        F.kind = L.kind;
        F.s = L.s;
        F.batch = L.batch;
        F.in = L.in;
        F.out = L.out;
        F.wq = Wt.w;
        F.vec = r2r_vec(L.in, L.out, L.s, L.dtype);
        if (int rc = get_twiddles((int)L.n, L.dtype, &F.tw)) return rc;
        const hipError_t e = run_tuned<R2rTag>(L.n, F, stream);
        if (e == hipSuccess) return DFFT_OK;
        return fail(DFFT_EHIP, std::string(three ? "r2r type III (fused): " : "r2r type II (fused): ") + hipGetErrorString(e));
    }
    if (!T && L.n > 4096) {
        int a, b;
        if (!long_split(L.n, &a, &b)) return fail(DFFT_EINVAL, "r2r: length " + std::to_string(L.n) + " needs Bluestein tables");
    }
    // batch chunks whose packed pairs and transform scratch fit the scratch buffer
    const long long sp = r2r_sp(L.s), units = r2r_units(L.s, L.batch);
    long long       nu = r2r_chunk_units(L.n, sp, L.dtype, units, cap);
    while (nu > 1 && chunk_bytes(L.n, sp, L.dtype, nu, T, bluestein_fused, cap) > scratch_bytes) nu = (nu + 1) / 2;
    if (!scratch || chunk_bytes(L.n, sp, L.dtype, nu, T, bluestein_fused, cap) > scratch_bytes) return fail(DFFT_EINVAL, "r2r: scratch buffer too small");
    const size_t zb = (size_t)nu * L.n * sp * elem_bytes(L.dtype);
    void*        inner = (char*)scratch + zb;
    const size_t inner_bytes = scratch_bytes - zb;
    for (long long u0 = 0; u0 < units; u0 += nu) {
        const long long m = std::min(nu, units - u0);
        const int       rc = L.dtype == F64 ? r2r_chunk<double2>(L, Wt, u0, m, T, bluestein_fused, scratch, inner, inner_bytes, stream)
                                            : r2r_chunk<float2>(L, Wt, u0, m, T, bluestein_fused, scratch, inner, inner_bytes, stream);
        if (rc) return rc;
    }
    return DFFT_OK;
}

#endif

}  // namespace dfft
