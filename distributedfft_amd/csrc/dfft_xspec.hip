// dfft_xspec.hip -- batched 1-D real cross-spectrum: two real fields x, g [batch][channels][n], every row zero-padded to m = 2 M,
//     S[c, k] = sum_b conj(rfft(x[b, c, :], m)[k]) rfft(g[b, c, :], m)[k],        k = 0 ... M,   out [channels][M + 1], unnormalised,
// for M a single-pass length (real form 1, m <= 8192): the filter gradient of dfft_rconv1d (the input gradient is dfft_rconv1d itself with
// the conjugated filter), and the Welch / cross-spectral-density / matched-filter accumulation.  g == x is the auto-spectrum sum |X|^2.
//
// Fused form, rxspec_rows_kernel (M with a tuned plan of dfft_plans.h): each row of either field is read once and nothing is written
// per row.  The batch is cut into `slices` contiguous ranges (rxspec_slices: fixed constants, never the device); ONE thread group, with the
// geometry of the convolution kernel (RconvGeom, dfft_rconv_impl.h), owns one (slice, channel) item.  Per row of its slice it loads
// x[b, c, :] as the M complex values z[j] = x[2j] + i x[2j+1], zeros beyond n, runs the M-point stages (run_stages), and with ONE LDS
// exchange for Z[M-k] forms, W = e^{-2 pi i / m},
//     2 X[k] = (Z[k] + conj Z[M-k]) - i (Z[k] - conj Z[M-k]) W^k
// into registers; the same for g[b, c, :]; and accumulates conj(2 X[k]) 2 G[k] in the working precision -- E accumulators per thread,
// each thread its own bins only (no partner product as in the convolution kernel: nothing is merged back).  Bin 0 pairs with itself
// through Z[M] = Z[0]: X[0] = Re Z[0] + Im Z[0], and the thread that holds it also keeps the Nyquist bin X[M] = Re Z[0] - Im Z[0].
// For even M the bin k = M/2 pairs with itself and the general formula holds.  After its rows the group stores its M + 1 sums times
// 1/4, the imaginary parts of bins 0 and M as exact zeros: straight to `out` for one slice, else to partial[slice][channel][.] in the
// scratch buffer, which slice_reduce (dfft_rows_common.hip) sums in slice order.  No atomics: the result is the same bits from call to call.
// The auto-spectrum skips the second transform and adds |2 X[k]|^2 to the real parts alone (x_r g_i - x_i g_r of equal operands is not
// an exact zero once the compiler contracts it into a multiply-add).
//
// Thread groups of one workgroup take consecutive items; all of them run the trip count of the longest slice (the exchanges of a
// group wider than a wavefront are workgroup barriers), rows beyond a group's own count -- and the groups of a ragged last workgroup --
// load zeros.
//
// Composed form (every other accepted M, the instantiations rxspec_fused_ok leaves out, DFFT_RXSPEC_FUSED=0): per chunk of rows of at
// most max(256 MiB, one row's) scratch -- pad_rows (dfft_rows_common.hip) and launch_real_rows forward on both fields, rxspec_mac_kernel: one thread
// per (channel, bin) adds the chunk's rows of its channel to `out` in row order.  Deterministic as well.
//
// Compiled once per instantiation group (-DDFFT_INST_GROUP=g: the fused kernels of the tuned lengths of group g) and once with
// -DDFFT_INST_GROUP=DFFT_NUM_INST_GROUPS (the dispatcher and the accumulating kernel of the composed form).
#include "dfft_fused_host.h"
#include "dfft_rows_common.h"
#include "dfft_xspec.h"

#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <cstring>

#ifndef DFFT_INST_GROUP
#error "compile with -DDFFT_INST_GROUP=<g>"
#endif

namespace dfft {

// One fused launch
struct RxspecFusedLaunch {
    int         dtype;
    long long   n, m, channels, batch, slices;
    bool        vec, autos;
    const void* x;
    const void* g;
    void*       dest;  // [slices][channels][m/2 + 1]: `out` for one slice, else the partial sums
    const void* tw;    // e^{-2 pi i k / M}
    const void* twh;   // e^{-2 pi i k / m}
};

// (M, dtype) whose instantiations would keep values in scratch memory (tools/fused_resources.py rxspec, profiles/2026-10-20_rxspec1d/
// kernel_resources.txt) or measured slower than the composed form are not built: they run the composed form.
constexpr bool rxspec_fused_ok(int M, bool f64) {
    if (M == 3125) return false;         // 25 points per thread: the forward kernel's exclusion, and three live arrays here
    if (M == 1536 && f64) return false;  // 24 points: the forward kernel's exclusion
    // 20, 24 and (2401) 7 points per thread in fp64: 12 ... 228 bytes per lane, per-real accesses always, two-real ones mostly
    if (f64 && (M == 200 || M == 384 || M == 400 || M == 640 || M == 1280 || M == 2401)) return false;
    return true;
}

// (M, dtype) whose E accumulators per thread live in LDS slots of the thread's own behind the exchange tiles (no barrier: nobody else
// touches them) instead of registers: 4096 points in fp64, 16 points per thread, went 36 bytes per lane into scratch with per-real
// accesses otherwise, and its 72 KiB tile allows one workgroup per CU by registers already, so the 64 KiB of slots cost no residency.
constexpr bool rxspec_acc_lds(int M, bool f64) { return M == 4096 && f64; }

// the family (dfft_fused_host.h); run<M>: defined in the translation unit of M's group only
struct RxspecTag {
    using Launch = RxspecFusedLaunch;
    static constexpr bool ok(int M, bool f64) { return rxspec_fused_ok(M, f64); }
    template <int M> static hipError_t run(const Launch& F, hipStream_t stream);
};

#if DFFT_INST_GROUP < DFFT_NUM_INST_GROUPS

template <class V, class P, bool VEC>
__global__ void __attribute__((amdgpu_flat_work_group_size(1, RconvGeom<V, P>::KG::THREADS)))
rxspec_rows_kernel(const typename real_of<V>::type* x, const typename real_of<V>::type* g, V* __restrict__ dest,
                   const typename VecTraits<V>::W* __restrict__ tw, const typename VecTraits<V>::W* __restrict__ twh, unsigned items, unsigned channels,
                   unsigned slices, unsigned batch, int n, int autos) {
    using RG = RconvGeom<V, P>;
    using KG = typename RG::KG;
    using W = typename VecTraits<V>::W;
    using RT = typename real_of<V>::type;
    constexpr int  E = P::E, T = P::T, M = P::N, G = RG::G, GT = KG::GT;
    constexpr bool ACC_LDS = rxspec_acc_lds(M, sizeof(V) == 16);
    extern __shared__ __attribute__((aligned(16))) char dfft_smem[];
    const int grp = threadIdx.x / GT;
    const int j = tile_j<1, KG::NW>((int)threadIdx.x - grp * GT);
    V*        lds = reinterpret_cast<V*>(dfft_smem + KG::TW_BYTES) + grp * RG::EXR;
    V*        accl = reinterpret_cast<V*>(dfft_smem + KG::TW_BYTES) + G * RG::EXR + grp * M;  // ACC_LDS: slot j + T k is this thread's
    W         twreg[KG::TWMODE == TW_REG && KG::TWN > 0 ? KG::TWN : 1];
    const W*  twr = stage_twiddles<V, P, +1, KG>(twreg, reinterpret_cast<W*>(dfft_smem), tw, j);
    W         wh[RG::TWH_REG ? E : 1];
    if constexpr (RG::TWH_REG) {
#pragma unroll
        for (int k = 0; k < E; ++k) wh[k] = twh[j + T * k];
    }
    // slice s holds rows [s per + min(s, rem), ...) of the batch: per rows, one more in the first rem slices
    const unsigned per = batch / slices, rem = batch % slices, trips = per + (rem ? 1u : 0u);
    for (unsigned i0 = blockIdx.x * G; i0 < items; i0 += gridDim.x * G) {
        const unsigned item = i0 + grp;  // slice * channels + channel
        const bool     valid = item < items;
        const unsigned s = valid ? item / channels : 0u, c = valid ? item - s * channels : 0u;
        const unsigned b0 = s * per + (s < rem ? s : rem), count = valid ? per + (s < rem ? 1u : 0u) : 0u;
        V              acc[ACC_LDS ? 1 : E];
        RT             accn = (RT)0;
#pragma unroll
        for (int k = 0; k < E; ++k) {
            if constexpr (ACC_LDS) accl[j + T * k] = V{0, 0};
            else acc[k] = V{0, 0};
        }
        for (unsigned i = 0; i < trips; ++i) {
            const bool      live = i < count;
            const long long base = live ? ((long long)(b0 + i) * channels + c) * n : 0ll;  // 64-bit row bases
            V               v[E];
            rrow_load<V, P, VEC>(v, x + base, live, n, j);
            const RT xn = rrow_bins<V, P, RG>(v, twr, lds, wh, twh, j);
            RT       gn = xn;
            V        xr[E];
#pragma unroll
            for (int k = 0; k < E; ++k) xr[k] = v[k];
            if (!autos) {  // (the same in every thread of the launch)
                rrow_load<V, P, VEC>(v, g + base, live, n, j);
                gn = rrow_bins<V, P, RG>(v, twr, lds, wh, twh, j);
            }
#pragma unroll
            for (int k = 0; k < E; ++k) {  // conj(X) G; the auto-spectrum's imaginary parts stay exact zeros
                const RT re = xr[k].x * v[k].x + xr[k].y * v[k].y, im = xr[k].x * v[k].y - xr[k].y * v[k].x;
                if constexpr (ACC_LDS) {
                    const V a = accl[j + T * k];
                    accl[j + T * k] = V{a.x + re, a.y + (autos ? (RT)0 : im)};
                } else {
                    acc[k].x += re;
                    acc[k].y += autos ? (RT)0 : im;
                }
            }
            accn += xn * gn;
        }
        if (valid) {
            V* op = dest + (size_t)item * (M + 1);
#pragma unroll
            for (int k = 0; k < E; ++k) {
                const int kk = j + T * k;
                const V   a = ACC_LDS ? accl[kk] : acc[ACC_LDS ? 0 : k];
                op[kk] = V{a.x * (RT)0.25, kk == 0 ? (RT)0 : a.y * (RT)0.25};
                if (kk == 0) op[M] = V{accn * (RT)0.25, (RT)0};
            }
        }
    }
}

template <class V, class P, bool VEC> hipError_t launch_rxspec_plan(const RxspecFusedLaunch& F, hipStream_t stream) {
    using RG = RconvGeom<V, P>;
    using W = typename VecTraits<V>::W;
    using RT = typename real_of<V>::type;
    constexpr size_t        LDS_BYTES = RG::LDS_BYTES + (rxspec_acc_lds(P::N, sizeof(V) == 16) ? (size_t)RG::G * P::N * sizeof(V) : 0);
    static_assert(LDS_BYTES <= 160 * 1024, "the accumulator slots do not fit the LDS of a CU");
    auto                    kern = rxspec_rows_kernel<V, P, VEC>;
    static std::atomic<int> blocks_per_cu[kMaxDevices];
    hipError_t              e;
    const int               bpc = resident_blocks_per_cu(reinterpret_cast<const void*>(kern), RG::KG::THREADS, LDS_BYTES, blocks_per_cu, &e);
    if (bpc == 0) return e;
    const long long items = F.channels * F.slices;
    const long long grid = persistent_grid(device_info().cus, bpc, (items + RG::G - 1) / RG::G);
    if (grid < 1) return hipSuccess;
    (void)hipGetLastError();
    hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(RG::KG::THREADS), LDS_BYTES, stream, (const RT*)F.x, (const RT*)F.g, (V*)F.dest, (const W*)F.tw,
                       (const W*)F.twh, (unsigned)items, (unsigned)F.channels, (unsigned)F.slices, (unsigned)F.batch, (int)F.n, F.autos ? 1 : 0);
    return hipGetLastError();
}

template <class V, int M> hipError_t rxspec_run_typed(const RxspecFusedLaunch& F, hipStream_t stream) {
    using P = typename PlanFor<M>::type;
    if constexpr (rxspec_fused_ok(M, sizeof(V) == 16)) return F.vec ? launch_rxspec_plan<V, P, true>(F, stream) : launch_rxspec_plan<V, P, false>(F, stream);
    return hipErrorInvalidValue;  // not built (rxspec_fused_ok): the dispatcher does not come here
}
template <int M> hipError_t RxspecTag::run(const RxspecFusedLaunch& F, hipStream_t stream) {
    if (F.dtype == F64) return rxspec_run_typed<double2, M>(F, stream);
    if (F.dtype == F32) return rxspec_run_typed<float2, M>(F, stream);
    return hipErrorInvalidValue;
}
DFFT_FUSED_INSTANTIATE(RxspecTag)

#else  // the dispatcher and the accumulating kernel of the composed form

// out[c][k] (+)= sum over the chunk's rows r of channel c, in row order, of conj(xb[r][k]) gb[r][k]; `first`: the chunk starts the sum.
// Row r of the chunk is row row0 + r of the fields.  autos: gb is xb, and the sum is of |xb|^2 with exact-zero imaginary parts.
template <class V>
__global__ void __launch_bounds__(256) rxspec_mac_kernel(const V* xb, const V* gb, V* __restrict__ out, long long nb, long long row0, long long nr,
                                                         long long channels, int first, int autos) {
    using RT = typename real_of<V>::type;
    const long long total = channels * nb;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
        const long long c = e / nb, k = e - c * nb;
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

// the cut into slices (slice_count): the target item count takes at most 8 thread groups of a workgroup, and a slice holds at least
// 8 rows (it costs M + 1 stored and re-read bins)
constexpr long long kRxspecMaxGroupFactor = 8;
constexpr long long kRxspecMinRows = 8;

bool shape_ok(const RxspecLaunch& L) {
    return L.n >= 1 && L.m >= L.n && real_length_supported(L.m) && L.channels >= 1 && L.batch >= 1 && (L.dtype == F64 || L.dtype == F32) &&
           L.channels < (1ll << 31) && L.batch < (1ll << 31) && L.batch * L.channels < (1ll << 31);
}

// one row of the composed form: its m/2 + 1 bins of either field and its m padded reals (shared by the two fields)
size_t row_bytes(long long m, int dtype) { return 2 * (size_t)(m / 2 + 1) * elem_bytes(dtype) + (size_t)m * (elem_bytes(dtype) / 2); }

template <class V> int pad_and_transform(const void* field, long long row0, long long nr, long long n, long long m, int dtype, void* pad, V* bins, hipStream_t stream) {
    using RT = typename real_of<V>::type;
    if (int rc = pad_rows((const RT*)field + row0 * n, pad, n, m, nr, dtype, stream)) return rc;
    const hipError_t e = launch_real_rows(contiguous_real_rows(dtype, m, nr, +1, 1.0, pad, bins), stream);
    if (e != hipSuccess) return fail(DFFT_EHIP, std::string("rxspec (pad, R2C rows): ") + hipGetErrorString(e));
    return DFFT_OK;
}

template <class V> int rxspec_chunk(const RxspecLaunch& L, long long row0, long long nr, void* scratch, hipStream_t stream) {
    const long long nb = L.m / 2 + 1;
    const bool      autos = L.x == L.g;
    V*              xb = (V*)scratch;         // [nr][nb]
    V*              gb = xb + nr * nb;        // [nr][nb]
    void*           pad = (void*)(gb + nr * nb);  // [nr][m] reals, behind a multiple of sizeof(V) bytes
    if (int rc = pad_and_transform<V>(L.x, row0, nr, L.n, L.m, L.dtype, pad, xb, stream)) return rc;
    if (!autos)
        if (int rc = pad_and_transform<V>(L.g, row0, nr, L.n, L.m, L.dtype, pad, gb, stream)) return rc;
    hipLaunchKernelGGL(rxspec_mac_kernel<V>, dim3(elementwise_grid(L.channels * nb)), dim3(256), 0, stream, (const V*)xb, (const V*)(autos ? xb : gb), (V*)L.out, nb,
                       row0, nr, L.channels, row0 == 0 ? 1 : 0, autos ? 1 : 0);
    DFFT_HIP_TRY(hipGetLastError());
    return DFFT_OK;
}

}  // namespace

bool rxspec_fused_env() { return env_switch_on("DFFT_RXSPEC_FUSED"); }

bool rxspec_vec(const void* x, const void* g, long long n, int dtype) {
    return n % 2 == 0 && (uintptr_t)x % elem_bytes(dtype) == 0 && (uintptr_t)g % elem_bytes(dtype) == 0;
}

bool rxspec_fused(long long n, long long m, int dtype, bool vec) {
    (void)vec;
    if (n < 1 || m < n || !real_length_supported(m) || (dtype != F64 && dtype != F32)) return false;
    return tuned_built<RxspecTag>(m / 2, dtype == F64);
}

long long rxspec_slices(long long m, long long channels, long long batch, int dtype) {
    if (m < 2 || !real_length_supported(m) || channels < 1 || batch < 1 || (dtype != F64 && dtype != F32) || channels >= (1ll << 31) ||
        batch >= (1ll << 31) || batch * channels >= (1ll << 31))
        return 0;
    return slice_count(groups_per_workgroup(m / 2), kRxspecMaxGroupFactor, channels, batch, kRxspecMinRows);
}

size_t rxspec_scratch_bytes(const RxspecLaunch& L, bool fused_on, size_t cap) {
    if (!shape_ok(L)) return 0;
    if (fused_on && rxspec_fused(L.n, L.m, L.dtype, rxspec_vec(L.x, L.g, L.n, L.dtype))) {
        const long long slices = rxspec_slices(L.m, L.channels, L.batch, L.dtype);
        return slices > 1 ? (size_t)slices * L.channels * (L.m / 2 + 1) * elem_bytes(L.dtype) : 0;
    }
    return (size_t)chunk_units(row_bytes(L.m, L.dtype), L.batch * L.channels, cap) * row_bytes(L.m, L.dtype);
}

int rxspec(const RxspecLaunch& L, bool fused_on, size_t cap, void* scratch, size_t scratch_bytes, hipStream_t stream) {
    if (!shape_ok(L) || !L.x || !L.g || !L.out) return fail(DFFT_EINVAL, "rxspec: bad arguments");
    const long long rows = L.batch * L.channels, nb = L.m / 2 + 1;
    const bool      vec = rxspec_vec(L.x, L.g, L.n, L.dtype);
    if (fused_on && rxspec_fused(L.n, L.m, L.dtype, vec)) {
        const long long slices = rxspec_slices(L.m, L.channels, L.batch, L.dtype);
        const size_t    need = slices > 1 ? (size_t)slices * L.channels * nb * elem_bytes(L.dtype) : 0;
        if (need && (!scratch || scratch_bytes < need)) return fail(DFFT_EINVAL, "rxspec: scratch buffer too small");
        RxspecFusedLaunch F;
        std::memset(&F, 0, sizeof(F));
        F.dtype = L.dtype;
        F.n = L.n;
        F.m = L.m;
        F.channels = L.channels;
        F.batch = L.batch;
        F.slices = slices;
        F.vec = vec;
        F.autos = L.x == L.g;
        F.x = L.x;
        F.g = L.g;
        F.dest = slices > 1 ? scratch : L.out;
        if (int rc = get_twiddles((int)(L.m / 2), L.dtype, &F.tw)) return rc;
        if (int rc = get_twiddles((int)L.m, L.dtype, &F.twh)) return rc;
        const hipError_t e = run_tuned<RxspecTag>(L.m / 2, F, stream);
        if (e != hipSuccess) return fail(DFFT_EHIP, std::string("rxspec (fused): ") + hipGetErrorString(e));
        return slices > 1 ? slice_reduce(scratch, L.out, L.channels * nb, slices, L.dtype, stream) : DFFT_OK;
    }
    // chunks of rows whose padded rows and bins fit the scratch buffer
    const size_t    rb = row_bytes(L.m, L.dtype);
    const long long nr = fit_chunk_to_lease("rxspec", chunk_units(rb, rows, cap), rb, scratch, scratch_bytes);
    if (nr < 1) return DFFT_EINVAL;
    for (long long r0 = 0; r0 < rows; r0 += nr) {
        const long long k = std::min(nr, rows - r0);
        const int       rc = L.dtype == F64 ? rxspec_chunk<double2>(L, r0, k, scratch, stream) : rxspec_chunk<float2>(L, r0, k, scratch, stream);
        if (rc) return rc;
    }
    return DFFT_OK;
}

#endif

}  // namespace dfft
