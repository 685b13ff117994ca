// dfft_csd.hip -- framed (Welch) 1-D real cross-spectrum: two real fields x, g [rows][n], every row cut into whole frames of m = 2 M reals
// that advance by `hop` (no padding, no centring: frame f is the samples [f hop, f hop + m)), each frame multiplied by win[m],
//     out[r][k] = scale sum_f conj(rfft(win x[r, f hop : f hop + m])[k]) rfft(win g[r, f hop : f hop + m])[k],   k = 0 ... M,
// out [rows][M + 1], for M a single-pass length (real form 1, m <= 8192): the sum that Welch power spectral densities, cross-spectral
// densities and coherences average.  g == x is the auto-spectrum sum |X|^2.  Per-frame detrending, median averaging, two-sided
// output, padding, frames beyond 8192 points and a backward form are not built.
//
// Fused form, rcsd_frames_kernel (M with a tuned plan of dfft_plans.h): the frame loader of stft_frames_kernel (dfft_stft.hip) in
// front of the split / conjugate-multiply / accumulate loop of rxspec_rows_kernel (dfft_xspec.hip).  The frames of a row are cut into
// `slices` contiguous ranges (rcsd_slices: fixed constants, never the device); ONE thread group, with the geometry of the convolution
// kernel (RconvGeom, dfft_rconv_impl.h), owns one (slice, row) item.  Per frame of its slice it loads the m reals of x at
// row n + f hop (64-bit bases) as the M complex values z[j] = x[2j] + i x[2j+1] -- frames are always whole, so nothing is clamped or
// mirrored -- multiplies by the window (in registers under the TWH_REG rule, read per use otherwise), runs the M-point stages
// (run_stages) and with ONE LDS exchange for Z[M-k] forms 2 X[k] into registers; the same for g; and accumulates conj(2 X[k]) 2 G[k]
// in the working precision -- E accumulators per thread, plus the Nyquist accumulator in the thread of bin 0.  Overlapping frames of a
// row are consecutive trips of one thread group: a row comes from HBM once and its other m / hop - 1 readings are L2 hits.  After
// its frames the group stores its M + 1 sums times scale / 4, the imaginary parts of bins 0 and M as exact zeros: straight to `out` for
// one slice, else to partial[slice][row][.] in the scratch buffer, which slice_reduce (dfft_rows_common.hip) sums in slice order.  No atomics: the
// result is the same bits from call to call.  No spectrogram and no framed copy ever exists in memory.
//
// Thread groups of one workgroup take consecutive items; all of them run the trip count of the longest slice (the exchanges of a
// group wider than a wavefront are workgroup barriers), frames beyond a group's own count -- and the groups of a ragged last workgroup
// -- load zeros.
//
// Composed form (every other accepted M, the instantiations rcsd_fused_ok leaves out, DFFT_RCSD_FUSED=0): per chunk of consecutive
// (row, frame) items of at most max(256 MiB, one frame's) scratch -- the STFT's frame kernel (dfft_stft.hip) into bins (g == x: into
// squared moduli) where it is built, else rcsd_gather_kernel and launch_real_rows forward, on both fields; rcsd_mac_kernel: one thread per (row, bin) adds the chunk's frames of its row to `out` in frame order and, behind the row's last frame,
// multiplies by scale.  The additions of a bin are the same whatever the chunking.  Deterministic as well.
//
// Compiled once per instantiation group (-DDFFT_INST_GROUP=g: the fused kernels of the tuned lengths of group g) and once with
// -DDFFT_INST_GROUP=DFFT_NUM_INST_GROUPS (the dispatcher, the reduction and the kernels of the composed form).
#include "dfft_csd.h"
#include "dfft_fused_host.h"
#include "dfft_rows_common.h"
#include "dfft_stft.h"

#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <cstring>
#include <type_traits>

#ifndef DFFT_INST_GROUP
#error "compile with -DDFFT_INST_GROUP=<g>"
#endif

namespace dfft {

// One fused launch
struct RcsdFusedLaunch {
    int         dtype;
    long long   n, m, hop, frames, rows, slices;
    double      scale;
    bool        vec, autos;
    const void* x;
    const void* g;
    void*       dest;  // [slices][rows][m/2 + 1]: `out` for one slice, else the partial sums
    const void* win;
    const void* tw;    // e^{-2 pi i k / M}
    const void* twh;   // e^{-2 pi i k / m}
};

// (M, dtype) whose instantiations would keep values in scratch memory (tools/fused_resources.py rcsd, profiles/2026-10-20_rcsd1d/
// kernel_resources.txt) are not built: they run the composed form.  The kernel reads or holds the window pairs of a thread next to
// everything rxspec_rows_kernel holds, so the list is longer than rxspec_fused_ok's.
constexpr bool rcsd_fused_ok(int M, bool f64, bool autos) {
    if (M == 3125) return false;
    // The auto-spectrum kernel (one transform, no copy of the bins, real accumulators) has room where the cross kernel has none: of the
    // lengths below only 1280, 1536 and 2401 points in fp64 go into scratch (12 ... 204 bytes per lane)
    if (autos) return !(f64 && (M == 1280 || M == 1536 || M == 2401));
    // 1024 points in fp32, cross: measured 2.58 ms against the composed form's 2.62 ms (4096 rows of 65536, hop 1024), inside the two
    // spreads -- not kept
    if (M == 1024 && !f64) return false;         // 25 points per thread: the forward kernel's exclusion, and three live arrays here
    if (M == 1536 && f64) return false;  // 24 points: the forward kernel's exclusion
    // 20, 24 and (2401) 7 points per thread in fp64: the exclusions of rxspec_fused_ok ...
    if (f64 && (M == 200 || M == 384 || M == 400 || M == 640 || M == 1280 || M == 2401)) return false;
    // ... and with the window the shorter 20- and 24-point lengths as well: 80 ... 428 bytes per lane
    if (f64 && (M == 48 || M == 80 || M == 96 || M == 100 || M == 160 || M == 192 || M == 320)) return false;
    // 4096 points in fp64, 16 points per thread: 252 ... 380 bytes per lane, and 228 with the accumulators in LDS slots as in
    // rxspec_rows_kernel
    if (f64 && M == 4096) return false;
    return true;
}

// the family (dfft_fused_host.h); run<M>: defined in the translation unit of M's group only
struct RcsdTag {
    using Launch = RcsdFusedLaunch;
    static constexpr bool ok(int M, bool f64, bool autos) { return rcsd_fused_ok(M, f64, autos); }
    template <int M> static hipError_t run(const Launch& F, hipStream_t stream);
};

#if DFFT_INST_GROUP < DFFT_NUM_INST_GROUPS

// The whole frame at `ip` (m reals; nothing is read of a frame that is not `live`) times the window, as the M complex values of a
// thread group
template <class V, class P, bool VEC, bool WIN_REG>
__device__ __forceinline__ void rcsd_load(V (&v)[P::E], const typename real_of<V>::type* ip, bool live, const V (&wn)[WIN_REG ? P::E : 1],
                                          const typename real_of<V>::type* __restrict__ win, int j) {
    using RT = typename real_of<V>::type;
    constexpr int E = P::E, T = P::T;
    // fp64 with the window read per use: the window comes in behind the frame, four values at a time -- the compiler would otherwise hold
    // the 2 E window values next to the E loaded ones, and the 16-point kernels of 1024 and 2048 points went 28 ... 124 bytes per lane
    // into scratch.  This rests on how the compiler schedules, and the kernels have no registers to spare: after any change of the
    // toolchain run tools/fused_resources.py rcsd again (tests/test_rcsd1d_host.py holds the inventory to zero scratch) and route what spills.
    constexpr bool STAGED = !WIN_REG && sizeof(V) == 16;
#pragma unroll
    for (int k = 0; k < E; ++k) {
        const int kk = j + T * k;
        V         a{(RT)0, (RT)0};
        if (live) {
            if constexpr (VEC) a = reinterpret_cast<const V*>(ip)[kk];  // n and hop even, the field aligned to two reals
            else a = V{ip[2 * kk], ip[2 * kk + 1]};
        }
        if constexpr (STAGED) {
            v[k] = a;
        } else {
            const V w2 = WIN_REG ? wn[WIN_REG ? k : 0] : V{win[2 * kk], win[2 * kk + 1]};
            v[k] = V{a.x * w2.x, a.y * w2.y};
        }
    }
    if constexpr (STAGED) {
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int k = 0; k < E; ++k) {
            const int kk = j + T * k;
            v[k] = V{v[k].x * win[2 * kk], v[k].y * win[2 * kk + 1]};
            if (k % 4 == 3) __builtin_amdgcn_sched_barrier(0);
        }
    }
}

// AUTO: g is x.  One transform per frame, no copy of the first field's bins and real accumulators only: about a third fewer live
// registers than the cross form.
template <class V, class P, bool VEC, bool AUTO>
__global__ void __attribute__((amdgpu_flat_work_group_size(1, RconvGeom<V, P>::KG::THREADS)))
rcsd_frames_kernel(const typename real_of<V>::type* x, const typename real_of<V>::type* g, V* __restrict__ dest,
                   const typename real_of<V>::type* __restrict__ win, const typename VecTraits<V>::W* __restrict__ tw,
                   const typename VecTraits<V>::W* __restrict__ twh, unsigned items, unsigned rows, unsigned slices, unsigned frames, long long n,
                   long long hop, int cross, double scale) {
    using RG = RconvGeom<V, P>;
    using KG = typename RG::KG;
    using W = typename VecTraits<V>::W;
    using RT = typename real_of<V>::type;
    constexpr int  E = P::E, T = P::T, M = P::N, G = RG::G, GT = KG::GT;
    constexpr bool WIN_REG = RG::TWH_REG;  // a thread's 2 E window values take the registers its E pairing twiddles take
    extern __shared__ __attribute__((aligned(16))) char dfft_smem[];
    const int grp = threadIdx.x / GT;
    const int j = tile_j<1, KG::NW>((int)threadIdx.x - grp * GT);
    V*        lds = reinterpret_cast<V*>(dfft_smem + KG::TW_BYTES) + grp * RG::EXR;
    W         twreg[KG::TWMODE == TW_REG && KG::TWN > 0 ? KG::TWN : 1];
    const W*  twr = stage_twiddles<V, P, +1, KG>(twreg, reinterpret_cast<W*>(dfft_smem), tw, j);
    W         wh[RG::TWH_REG ? E : 1];
    if constexpr (RG::TWH_REG) {
#pragma unroll
        for (int k = 0; k < E; ++k) wh[k] = twh[j + T * k];
    }
    V wn[WIN_REG ? E : 1];  // (win[2 jj], win[2 jj + 1]) of the thread's values jj = j + T k
    if constexpr (WIN_REG) {
#pragma unroll
        for (int k = 0; k < E; ++k) wn[k] = V{win[2 * (j + T * k)], win[2 * (j + T * k) + 1]};
    }
    const RT sc = (RT)(0.25 * scale);
    // slice s holds frames [s per + min(s, rem), ...) of its row: per frames, one more in the first rem slices
    const unsigned per = frames / slices, rem = frames % slices, trips = per + (rem ? 1u : 0u);
    for (unsigned i0 = blockIdx.x * G; i0 < items; i0 += gridDim.x * G) {
        const unsigned item = i0 + grp;  // slice * rows + row
        const bool     valid = item < items;
        const unsigned s = valid ? item / rows : 0u, row = valid ? item - s * rows : 0u;
        const unsigned f0 = s * per + (s < rem ? s : rem), count = valid ? per + (s < rem ? 1u : 0u) : 0u;
        using ACC = typename std::conditional<AUTO, RT, V>::type;
        ACC            acc[E];
        RT             accn = (RT)0;
#pragma unroll
        for (int k = 0; k < E; ++k) acc[k] = ACC{};
        for (unsigned i = 0; i < trips; ++i) {
            const bool      live = i < count;  // f0 + i < frames: the whole frame lies inside the row
            const long long base = live ? (long long)row * n + (long long)(f0 + i) * hop : 0ll;  // 64-bit bases
            V               v[E];
            rcsd_load<V, P, VEC, WIN_REG>(v, x + base, live, wn, win, j);
            const RT xn = rrow_bins<V, P, RG>(v, twr, lds, wh, twh, j);
            if constexpr (AUTO) {  // |2 X|^2: the imaginary parts are never formed
#pragma unroll
                for (int k = 0; k < E; ++k) acc[k] += v[k].x * v[k].x + v[k].y * v[k].y;
                accn += xn * xn;
            } else {
                RT gn = xn;
                V  xr[E];
#pragma unroll
                for (int k = 0; k < E; ++k) xr[k] = v[k];
                if (cross) {  // always: a branch the compiler cannot see through keeps the second field's loads and transform behind the
                              // first one's (merged, the 16- to 24-point kernels go 120 ... 468 bytes per lane into scratch)
                    rcsd_load<V, P, VEC, WIN_REG>(v, g + base, live, wn, win, j);
                    gn = rrow_bins<V, P, RG>(v, twr, lds, wh, twh, j);
                }
#pragma unroll
                for (int k = 0; k < E; ++k) {  // conj(X) G
                    acc[k].x += xr[k].x * v[k].x + xr[k].y * v[k].y;
                    acc[k].y += xr[k].x * v[k].y - xr[k].y * v[k].x;
                }
                accn += xn * gn;
            }
        }
        if (valid) {
            V* op = dest + (size_t)item * (M + 1);
#pragma unroll
            for (int k = 0; k < E; ++k) {
                const int kk = j + T * k;
                if constexpr (AUTO) op[kk] = V{acc[k] * sc, (RT)0};
                else op[kk] = V{acc[k].x * sc, kk == 0 ? (RT)0 : acc[k].y * sc};
                if (kk == 0) op[M] = V{accn * sc, (RT)0};
            }
        }
    }
}

template <class V, class P, bool VEC, bool AUTO> hipError_t launch_rcsd_plan(const RcsdFusedLaunch& F, hipStream_t stream) {
    using RG = RconvGeom<V, P>;
    using W = typename VecTraits<V>::W;
    using RT = typename real_of<V>::type;
    constexpr size_t        LDS_BYTES = RG::LDS_BYTES;
    auto                    kern = rcsd_frames_kernel<V, P, VEC, AUTO>;
    static std::atomic<int> blocks_per_cu[kMaxDevices];
    hipError_t              e;
    const int               bpc = resident_blocks_per_cu(reinterpret_cast<const void*>(kern), RG::KG::THREADS, LDS_BYTES, blocks_per_cu, &e);
    if (bpc == 0) return e;
    const long long items = F.rows * F.slices;
    const long long grid = persistent_grid(device_info().cus, bpc, (items + RG::G - 1) / RG::G);
    if (grid < 1) return hipSuccess;
    (void)hipGetLastError();
    hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(RG::KG::THREADS), LDS_BYTES, stream, (const RT*)F.x, (const RT*)F.g, (V*)F.dest, (const RT*)F.win,
                       (const W*)F.tw, (const W*)F.twh, (unsigned)items, (unsigned)F.rows, (unsigned)F.slices, (unsigned)F.frames, F.n, F.hop, F.autos ? 0 : 1, F.scale);
    return hipGetLastError();
}

template <class V, int M> hipError_t rcsd_run_typed(const RcsdFusedLaunch& F, hipStream_t stream) {
    using P = typename PlanFor<M>::type;
    if constexpr (rcsd_fused_ok(M, sizeof(V) == 16, true)) {
        if (F.autos) return F.vec ? launch_rcsd_plan<V, P, true, true>(F, stream) : launch_rcsd_plan<V, P, false, true>(F, stream);
    }
    if constexpr (rcsd_fused_ok(M, sizeof(V) == 16, false)) {
        if (!F.autos) return F.vec ? launch_rcsd_plan<V, P, true, false>(F, stream) : launch_rcsd_plan<V, P, false, false>(F, stream);
    }
    return hipErrorInvalidValue;  // not built (rcsd_fused_ok): the dispatcher does not come here
}
template <int M> hipError_t RcsdTag::run(const RcsdFusedLaunch& F, hipStream_t stream) {
    if (F.dtype == F64) return rcsd_run_typed<double2, M>(F, stream);
    if (F.dtype == F32) return rcsd_run_typed<float2, M>(F, stream);
    return hipErrorInvalidValue;
}
DFFT_FUSED_INSTANTIATE(RcsdTag)

#else  // the dispatcher and the kernels of the composed form

// item it0 + t = (row, f): row = item / frames, f = item % frames.  Windowed frames: p[t][i] = in[row n + f hop + i] win[i]
template <class RT>
__global__ void __launch_bounds__(256) rcsd_gather_kernel(const RT* __restrict__ in, RT* __restrict__ p, const RT* __restrict__ win, long long n, long long m,
                                                          long long hop, long long frames, long long it0, long long total) {
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
        const long long t = e / m, i = e - t * m;
        const long long row = (it0 + t) / frames, f = (it0 + t) - row * frames;
        p[e] = in[row * n + f * hop + i] * win[i];
    }
}
// The chunk holds the bins xb, gb [ni][nb] of the items [it0, it0 + ni), which touch the rows [r0, r0 + nr).  out[r][k] (+)= the sum,
// in frame order, of conj(xb[t][k]) gb[t][k] over the chunk's frames of row r: a row whose frame 0 lies in the chunk starts its sum,
// and a row whose last frame does is multiplied by scale behind it.  autos: gb is xb, and the sum is of |xb|^2 with exact-zero
// imaginary parts.
template <class V>
__global__ void __launch_bounds__(256) rcsd_mac_kernel(const V* xb, const V* gb, V* __restrict__ out, long long nb, long long frames, long long it0,
                                                       long long ni, long long r0, long long nr, double scale, int autos, int power) {
    using RT = typename real_of<V>::type;
    const long long total = nr * nb;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
        const long long rl = e / nb, k = e - rl * nb, r = r0 + rl;
        const long long lo = it0 > r * frames ? it0 : r * frames, hi = it0 + ni < (r + 1) * frames ? it0 + ni : (r + 1) * frames;  // the row's items of the chunk
        V               acc = lo == r * frames ? V{0, 0} : out[r * nb + k];
        for (long long it = lo; it < hi; ++it) {
            if (power) {  // xb holds |bins|^2, reals
                acc.x += reinterpret_cast<const RT*>(xb)[(it - it0) * nb + k];
                continue;
            }
            const V a = xb[(it - it0) * nb + k];
            if (autos) {
                acc.x += a.x * a.x + a.y * a.y;
            } else {
                const V b = gb[(it - it0) * nb + k];
                acc.x += a.x * b.x + a.y * b.y;
                acc.y += a.x * b.y - a.y * b.x;
            }
        }
        if (k == 0 || k == nb - 1) acc.y = (RT)0;  // DC and Nyquist
        if (hi == (r + 1) * frames) acc = V{acc.x * (RT)scale, acc.y * (RT)scale};
        out[r * nb + k] = acc;
    }
}
namespace {

// the cut into slices (slice_count; 512 workgroups per part: 2048 measured): the target item count takes at most 32 thread
// groups of a workgroup, and a slice holds at least 8 frames (it costs M + 1 stored and re-read bins)
constexpr long long kRcsdMaxGroupFactor = 32;
constexpr long long kRcsdMinFrames = 8;

bool shape_ok(const RcsdLaunch& L) {
    return (L.dtype == F64 || L.dtype == F32) && L.n >= 1 && L.m >= 2 && L.m <= L.n && L.hop >= 1 && L.rows >= 1 && L.frames >= 1 &&
           real_length_supported(L.m) && rcsd_items_ok(L.rows, L.frames) && L.frames == stft_frames(L.n, L.m, L.hop, 0);
}

// one item (frame of a row) of the composed form: its m/2 + 1 bins of either field and its m windowed reals (shared by the two fields)
size_t item_bytes(long long m, int dtype) { return 2 * (size_t)(m / 2 + 1) * elem_bytes(dtype) + (size_t)m * (elem_bytes(dtype) / 2); }
// items of a chunk: what fits 256 MiB, or DFFT_RCSD_CHUNK_BYTES
long long chunk_items(long long m, int dtype, long long items) { return chunk_units(item_bytes(m, dtype), items, chunk_cap_env("DFFT_RCSD_CHUNK_BYTES")); }

template <class V>
hipError_t gather_and_transform(const RcsdLaunch& L, const void* field, long long it0, long long ni, void* fr, V* bins, hipStream_t stream) {
    using RT = typename real_of<V>::type;
    (void)hipGetLastError();
    hipLaunchKernelGGL(rcsd_gather_kernel<RT>, dim3(elementwise_grid(ni * L.m)), dim3(256), 0, stream, (const RT*)field, (RT*)fr, (const RT*)L.win, L.n, L.m,
                       L.hop, L.frames, it0, ni * L.m);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return launch_real_rows(contiguous_real_rows(L.dtype, L.m, ni, +1, 1.0, fr, bins), stream);
}

// The bins (auto-spectrum: their squared moduli) of the items [it0, it0 + ni) of one field through the one-launch frame kernel of the
// STFT (dfft_stft.hip), which reads the frames straight from the rows: no framed copy.  The items are whole rows, or frames of one row.
int frames_by_stft(const RcsdLaunch& L, const void* field, long long it0, long long ni, void* bins, bool power, hipStream_t stream) {
    const long long r0 = it0 / L.frames, f0 = it0 - r0 * L.frames;
    const bool      piece = f0 != 0 || ni % L.frames != 0;
    StftLaunch      S;
    std::memset(&S, 0, sizeof(S));
    S.dtype = L.dtype;
    S.pad_mode = STFT_PAD_ZERO;
    S.out_kind = power ? STFT_OUT_POWER : STFT_OUT_COMPLEX;
    S.m = L.m;
    S.hop = L.hop;
    S.pad = 0;
    S.n = piece ? (ni - 1) * L.hop + L.m : L.n;
    S.frames = piece ? ni : L.frames;
    S.rows = piece ? 1 : ni / L.frames;
    S.scale = 1.0;
    S.in = (const char*)field + (size_t)(r0 * L.n + f0 * L.hop) * (elem_bytes(L.dtype) / 2);
    S.out = bins;
    S.win = L.win;
    return stft(S, true, nullptr, 0, stream);
}

// by_stft: the chunk is whole rows or frames of one row, and the STFT's frame kernel is built for (m/2, dtype)
template <class V> int rcsd_chunk(const RcsdLaunch& L, long long it0, long long ni, bool by_stft, void* scratch, hipStream_t stream) {
    const long long nb = L.m / 2 + 1;
    const bool      autos = L.x == L.g, power = by_stft && autos;
    V*              xb = (V*)scratch;           // [ni][nb] (power: as many reals)
    V*              gb = xb + ni * nb;          // [ni][nb]
    void*           fr = (void*)(gb + ni * nb);  // [ni][m] reals, behind a multiple of sizeof(V) bytes
    if (by_stft) {
        if (int rc = frames_by_stft(L, L.x, it0, ni, xb, power, stream)) return rc;
        if (!autos)
            if (int rc = frames_by_stft(L, L.g, it0, ni, gb, false, stream)) return rc;
    } else {
        hipError_t e = gather_and_transform<V>(L, L.x, it0, ni, fr, xb, stream);
        if (e == hipSuccess && !autos) e = gather_and_transform<V>(L, L.g, it0, ni, fr, gb, stream);
        if (e != hipSuccess) return fail(DFFT_EHIP, std::string("rcsd (gather, R2C rows): ") + hipGetErrorString(e));
    }
    const long long r0 = it0 / L.frames, nr = (it0 + ni - 1) / L.frames - r0 + 1;
    hipLaunchKernelGGL(rcsd_mac_kernel<V>, dim3(elementwise_grid(nr * nb)), dim3(256), 0, stream, (const V*)xb, (const V*)(autos ? xb : gb), (V*)L.out, nb, L.frames,
                       it0, ni, r0, nr, L.scale, autos ? 1 : 0, power ? 1 : 0);
    DFFT_HIP_TRY(hipGetLastError());
    return DFFT_OK;
}

}  // namespace

bool rcsd_fused_env() { return env_switch_on("DFFT_RCSD_FUSED"); }

bool rcsd_vec(const void* x, const void* g, long long n, long long hop, int dtype) {
    return n % 2 == 0 && hop % 2 == 0 && (uintptr_t)x % elem_bytes(dtype) == 0 && (uintptr_t)g % elem_bytes(dtype) == 0;
}

bool rcsd_fused(long long m, int dtype, bool autos) {
    if ((dtype != F64 && dtype != F32) || m < 4 || m % 2 || !real_length_supported(m)) return false;
    return tuned_built<RcsdTag>(m / 2, dtype == F64, autos);
}

long long rcsd_slices(long long m, long long rows, long long frames, int dtype) {
    if (m < 2 || !real_length_supported(m) || rows < 1 || frames < 1 || (dtype != F64 && dtype != F32) || !rcsd_items_ok(rows, frames)) return 0;
    return slice_count(groups_per_workgroup(m / 2), kRcsdMaxGroupFactor, rows, frames, kRcsdMinFrames);
}

size_t rcsd_scratch_bytes(const RcsdLaunch& L, bool fused_on) {
    if (!shape_ok(L)) return 0;
    if (fused_on && rcsd_fused(L.m, L.dtype, L.x == L.g)) {
        const long long slices = rcsd_slices(L.m, L.rows, L.frames, L.dtype);
        return slices > 1 ? (size_t)slices * L.rows * (L.m / 2 + 1) * elem_bytes(L.dtype) : 0;
    }
    // rows * frames stays below 2^62
    return (size_t)chunk_items(L.m, L.dtype, L.rows * L.frames) * item_bytes(L.m, L.dtype);
}

int rcsd(const RcsdLaunch& L, bool fused_on, void* scratch, size_t scratch_bytes, hipStream_t stream) {
    if (!shape_ok(L) || !L.x || !L.g || !L.out || !L.win) return fail(DFFT_EINVAL, "rcsd: bad arguments");
    const long long nb = L.m / 2 + 1;
    if (fused_on && rcsd_fused(L.m, L.dtype, L.x == L.g)) {
        const long long slices = rcsd_slices(L.m, L.rows, L.frames, L.dtype);
        const size_t    need = slices > 1 ? (size_t)slices * L.rows * nb * elem_bytes(L.dtype) : 0;
        if (need && (!scratch || scratch_bytes < need)) return fail(DFFT_EINVAL, "rcsd: scratch buffer too small");
        RcsdFusedLaunch F;
        std::memset(&F, 0, sizeof(F));
        F.dtype = L.dtype;
        F.n = L.n;
        F.m = L.m;
        F.hop = L.hop;
        F.frames = L.frames;
        F.rows = L.rows;
        F.slices = slices;
        F.scale = L.scale;
        F.vec = rcsd_vec(L.x, L.g, L.n, L.hop, L.dtype);
        F.autos = L.x == L.g;
        F.x = L.x;
        F.g = L.g;
        F.dest = slices > 1 ? scratch : L.out;
        F.win = L.win;
        if (int rc = get_twiddles((int)(L.m / 2), L.dtype, &F.tw)) return rc;
        if (int rc = get_twiddles((int)L.m, L.dtype, &F.twh)) return rc;
        const hipError_t e = run_tuned<RcsdTag>(L.m / 2, F, stream);
        if (e != hipSuccess) return fail(DFFT_EHIP, std::string("rcsd (fused): ") + hipGetErrorString(e));
        return slices > 1 ? slice_reduce(scratch, L.out, L.rows * nb, slices, L.dtype, stream) : DFFT_OK;
    }
    // chunks of consecutive (row, frame) items whose windowed frames and bins fit the scratch buffer: the frames of a row are added in
    // ascending order whatever the cut
    const size_t    ib = item_bytes(L.m, L.dtype);
    const long long items = L.rows * L.frames;
    long long       ni = fit_chunk_to_lease("rcsd", chunk_items(L.m, L.dtype, items), ib, scratch, scratch_bytes);
    if (ni < 1) return DFFT_EINVAL;
    // Where the STFT's one-launch frame kernel is built for (m/2, dtype) it forms the chunk's bins straight from the rows; the chunks
    // are then whole rows, or -- a row with more frames than a chunk holds -- runs of frames of one row.  No windowed frames are kept
    // then (and the auto-spectrum keeps squared moduli, not bins), so the same lease holds more items.
    const bool by_stft = stft_fused_env() && stft_fused(L.m, L.dtype);
    if (by_stft) {
        const size_t held = L.x == L.g ? (size_t)nb * (elem_bytes(L.dtype) / 2) : 2 * (size_t)nb * elem_bytes(L.dtype);
        ni = std::min(items, (long long)((size_t)ni * ib / held));
    }
    for (long long i0 = 0; i0 < items;) {
        long long k = std::min(ni, items - i0);
        if (by_stft) {
            const long long f0 = i0 % L.frames;
            k = f0 == 0 && k >= L.frames ? k / L.frames * L.frames : std::min(k, L.frames - f0);
        }
        const int rc = L.dtype == F64 ? rcsd_chunk<double2>(L, i0, k, by_stft, scratch, stream) : rcsd_chunk<float2>(L, i0, k, by_stft, scratch, stream);
        if (rc) return rc;
        i0 += k;
    }
    return DFFT_OK;
}

#endif

}  // namespace dfft
