// dfft_stft.hip -- batched short-time Fourier transform and its inverse: rows of reals [rows][n] cut into frames of m = 2 M reals (M a
// single-pass length, real form 1, m <= 8192) that advance by `hop`.  Frame f of row r is
//     xb[i] = P(x[r], f hop - pad + i) win[i]   (P: the sample inside [0, n), outside it 0 or the mirrored sample),
//     out[r][f][k] = scale rfft(xb, m)[k]   or   scale^2 |rfft(xb, m)[k]|^2,   0 <= k <= M,
// and the inverse is torch.istft's least-squares overlap-add, out[r][t] = inv_env[t] sum_f win[i] irfft(in[r][f], m)[i], i = t + pad - f hop.
// Four-step and Bluestein frames (m > 8192), two-sided output and a fused inverse are not built.
//
// Fused forward, stft_frames_kernel (M with a tuned plan, stft_fused_ok): ONE launch, the persistent loop of osconv_blocks_kernel
// (dfft_osconv.hip) over the items it = row * frames + f, one item per thread group (RconvGeom of dfft_rconv_impl.h).  The load base is
// row * n + f hop - pad with a window [lo, hi) clamped to the row; a frame whose window is whole moves two reals per access where n, hop
// and pad are even and `in` is aligned to two reals (VEC), every other frame goes real by real with the zero or the mirrored index.  The
// window values of a thread do not depend on the item: they stay in registers where they are few (the TWH_REG rule).  One run_stages,
// then the split X[k] = (Xe[k] + W^k Xo[k]) with the partner M - k read through the LDS tile; each thread stores the bins of its own E
// values, the thread of k = 0 also bin M.  The framed copy -- m / hop times the signal -- never exists in memory, and a power
// spectrogram writes half the bytes of the complex one.  As in osconv_blocks_kernel the store base is taken from a copy of the item the
// compiler cannot trace back, so that it does not occupy registers across the transform.
//
// Composed forward (every other accepted M, the instantiations stft_fused_ok leaves out, DFFT_STFT_FUSED=0): per chunk of items of at
// most max(256 MiB, one item's) scratch -- stft_gather_kernel into windowed frames, launch_real_rows forward into `out` (pitch M + 1),
// or, for the power form, into scratch bins followed by stft_power_kernel.
//
// Inverse (composed only): per chunk of frames launch_real_rows backward into scratch frames [items][m] -- from a copy of the bins where
// M is untuned, because the two-launch C2R merges in place on its input -- and istft_ola_kernel, one thread per output sample, which
// sums the at most ceil(m / hop) windowed contributions in ascending frame order and multiplies by inv_env[t] / m: no atomics, the
// result does not depend on the chunking.  Chunks hold whole rows where a row fits; a longer row is cut at output samples, and a cut
// transforms again the at most ceil(m / hop) - 1 frames its first outputs share with the cut before.
//
// Compiled once per instantiation group (-DDFFT_INST_GROUP=g: the fused kernels of the tuned lengths of group g) and once with
// -DDFFT_INST_GROUP=DFFT_NUM_INST_GROUPS (the dispatcher and the kernels of the composed forms).
#include "dfft_fused_host.h"
#include "dfft_rconv_impl.h"
#include "dfft_real.h"
#include "dfft_stft.h"

#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <cstring>

#ifndef DFFT_INST_GROUP
#error "compile with -DDFFT_INST_GROUP=<g>"
#endif

namespace dfft {

// One fused launch
struct StftFusedLaunch {
    int         dtype;
    bool        power, vec, reflect;
    long long   n, m, hop, pad, frames, items;
    double      scale;
    const void* in;
    void*       out;
    const void* win;
    const void* tw;   // e^{-2 pi i k / M}
    const void* twh;  // e^{-2 pi i k / m}
};

// (M, dtype) whose frame kernels would keep values in scratch memory (tools/fused_resources.py stft, profiles/2026-10-20_stft/
// kernel_resources.txt) are not built: they run the composed form.
constexpr bool stft_fused_ok(int M, bool f64) {
    if (M == 2401 && f64) return false;  // 7 points per thread on 343 threads: 20 ... 28 bytes per lane (none in fp32)
    if (M == 3125 && f64) return false;  // 25 points per thread on 125 threads: 80 ... 164 bytes per lane (none in fp32)
    return true;
}

// the family (dfft_fused_host.h); run<M>: defined in the translation unit of M's group only
struct StftTag {
    using Launch = StftFusedLaunch;
    static constexpr bool ok(int M, bool f64) { return stft_fused_ok(M, f64); }
    template <int M> static hipError_t run(const Launch& F, hipStream_t stream);
};

// sample s of a row of n, s outside [0, n): the mirrored index, held inside the row whatever the arguments
__device__ __forceinline__ long long stft_mirror(long long s, long long n) {
    const long long r = s < 0 ? -s : 2 * (n - 1) - s;
    return r < 0 ? 0 : r > n - 1 ? n - 1 : r;
}

#if DFFT_INST_GROUP < DFFT_NUM_INST_GROUPS

template <class V, class P, bool POWER, bool VEC>
__global__ void __attribute__((amdgpu_flat_work_group_size(1, RconvGeom<V, P>::KG::THREADS)))
stft_frames_kernel(const typename real_of<V>::type* __restrict__ in, void* __restrict__ outv, const typename real_of<V>::type* __restrict__ win,
                   const typename VecTraits<V>::W* __restrict__ tw, const typename VecTraits<V>::W* __restrict__ twh, unsigned items, unsigned frames,
                   long long n, long long hop, int pad, int reflect, double scale) {
    using RG = RconvGeom<V, P>;
    using KG = typename RG::KG;
    using W = typename VecTraits<V>::W;
    using RT = typename real_of<V>::type;
    constexpr int  E = P::E, T = P::T, M = P::N, G = RG::G, GT = KG::GT;
    constexpr bool TWPOW = KG::TWMODE == TW_REG;
    constexpr bool WIN_REG = RG::TWH_REG;  // a thread's 2 E window values take the registers its E pairing twiddles take
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
    V wn[WIN_REG ? E : 1];  // (win[2 jj], win[2 jj + 1]) of the thread's values jj = j + T k
    if constexpr (WIN_REG) {
#pragma unroll
        for (int k = 0; k < E; ++k) wn[k] = V{win[2 * (j + T * k)], win[2 * (j + T * k) + 1]};
    }
    const RT   sc = (RT)(0.5 * scale);  // the halves of Xe, Xo are folded in
    const auto clamp_m = [](long long x) { return (int)(x < 0 ? 0 : x > 2 * M ? 2 * M : x); };
    for (unsigned i0 = blockIdx.x * G; i0 < items; i0 += gridDim.x * G) {
        const unsigned it = i0 + g;
        const bool     valid = it < items;
        const unsigned row = valid ? it / frames : 0u;
        // real i of the frame is sample s0 + i of its row
        const long long s0 = (long long)(valid ? it - row * frames : 0u) * hop - pad;
        // samples i in [lo, hi) lie inside [0, n); an item past the last one loads nothing (and stores nothing)
        const int       lo = valid ? clamp_m(-s0) : 0, hi = valid ? clamp_m(n - s0) : 0;
        const long long rbase = (long long)row * n;  // 64-bit bases; dereferenced at samples inside the row only
        V               v[E];
        if (VEC && lo == 0 && hi == 2 * M) {  // a whole frame; n, hop and pad even: rbase + s0 is even
#pragma unroll
            for (int k = 0; k < E; ++k) v[k] = *reinterpret_cast<const V*>(in + (rbase + s0 + 2 * (j + T * k)));
        } else {
#pragma unroll
            for (int k = 0; k < E; ++k) {
                const int i = 2 * (j + T * k);
                RT        a = (RT)0, b = (RT)0;
                if (i >= lo && i < hi) a = in[rbase + s0 + i];
                else if (reflect && valid) a = in[rbase + stft_mirror(s0 + i, n)];
                if (i + 1 >= lo && i + 1 < hi) b = in[rbase + s0 + i + 1];
                else if (reflect && valid) b = in[rbase + stft_mirror(s0 + i + 1, n)];
                v[k] = V{a, b};
            }
        }
#pragma unroll
        for (int k = 0; k < E; ++k) {
            const V w2 = WIN_REG ? wn[WIN_REG ? k : 0] : V{win[2 * (j + T * k)], win[2 * (j + T * k) + 1]};
            v[k] = V{v[k].x * w2.x, v[k].y * w2.y};
        }
        run_stages<V, P, 0, +1, 1, KG::PAD, KG::WAVE_LOCAL, KG::TWMODE, TWPOW, 1, 1, KG::NW, KG::LOCALX>(v, twr, lds, j, 0);
        group_sync<KG::WAVE_LOCAL>();
#pragma unroll
        for (int k = 0; k < E; ++k) lds[lds_index<1, KG::PAD>(j + T * k, 0)] = v[k];
        group_sync<KG::WAVE_LOCAL>();
        // the store base, from a copy of the item the compiler cannot trace back: not held across the transform
        unsigned it2 = it;
        asm volatile("" : "+v"(it2));
        const bool      valid2 = it2 < items;
        const long long obase = (long long)it2 * (M + 1);
#pragma unroll
        for (int k = 0; k < E; ++k) {
            const int kk = j + T * k;
            const V   zm = lds[lds_index<1, KG::PAD>(kk == 0 ? 0 : M - kk, 0)];
            const W   w = RG::TWH_REG ? wh[RG::TWH_REG ? k : 0] : twh[kk];
            const V   xe{v[k].x + zm.x, v[k].y - zm.y};  // 2 Xe[k]
            const V   xo{v[k].y + zm.y, zm.x - v[k].x};  // 2 Xo[k]
            const V   t = cmul(xo, w);
            const V   xk{(xe.x + t.x) * sc, (xe.y + t.y) * sc};  // scale X[k]
            const V   xm{(xe.x - t.x) * sc, (t.y - xe.y) * sc};  // scale X[M - k] = conj(Xe - W^k Xo): stored for k = 0 (bin M) only
            if (valid2) {
                if constexpr (POWER) {
                    RT* out = reinterpret_cast<RT*>(outv);
                    out[obase + kk] = xk.x * xk.x + xk.y * xk.y;
                    if (kk == 0) out[obase + M] = xm.x * xm.x + xm.y * xm.y;
                } else {
                    V* out = reinterpret_cast<V*>(outv);
                    out[obase + kk] = xk;
                    if (kk == 0) out[obase + M] = xm;
                }
            }
        }
        group_sync<KG::WAVE_LOCAL>();  // every partner is read before the next item's exchanges reuse the tile
    }
}

template <class V, class P, bool POWER, bool VEC> hipError_t launch_stft_plan(const StftFusedLaunch& F, hipStream_t stream) {
    using RG = RconvGeom<V, P>;
    using W = typename VecTraits<V>::W;
    using RT = typename real_of<V>::type;
    auto                    kern = stft_frames_kernel<V, P, POWER, VEC>;
    static std::atomic<int> blocks_per_cu[kMaxDevices];
    hipError_t              e;
    const int               bpc = resident_blocks_per_cu(reinterpret_cast<const void*>(kern), RG::KG::THREADS, RG::LDS_BYTES, blocks_per_cu, &e);
    if (bpc == 0) return e;
    const long long grid = persistent_grid(device_info().cus, bpc, (F.items + RG::G - 1) / RG::G);
    if (grid < 1) return hipSuccess;
    (void)hipGetLastError();
    hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(RG::KG::THREADS), RG::LDS_BYTES, stream, (const RT*)F.in, F.out, (const RT*)F.win, (const W*)F.tw,
                       (const W*)F.twh, (unsigned)F.items, (unsigned)F.frames, F.n, F.hop, (int)F.pad, (int)F.reflect, F.scale);
    return hipGetLastError();
}

template <class V, int M> hipError_t stft_run_typed(const StftFusedLaunch& F, hipStream_t stream) {
    using P = typename PlanFor<M>::type;
    if constexpr (stft_fused_ok(M, sizeof(V) == 16)) {
        if (F.power) return F.vec ? launch_stft_plan<V, P, true, true>(F, stream) : launch_stft_plan<V, P, true, false>(F, stream);
        return F.vec ? launch_stft_plan<V, P, false, true>(F, stream) : launch_stft_plan<V, P, false, false>(F, stream);
    }
    return hipErrorInvalidValue;  // not built (stft_fused_ok): the dispatcher does not come here
}
template <int M> hipError_t StftTag::run(const StftFusedLaunch& F, hipStream_t stream) {
    if (F.dtype == F64) return stft_run_typed<double2, M>(F, stream);
    if (F.dtype == F32) return stft_run_typed<float2, M>(F, stream);
    return hipErrorInvalidValue;
}
DFFT_FUSED_INSTANTIATE(StftTag)

#else  // the dispatcher and the kernels of the composed forms

// item (it0 + t) = (row, f): row = item / frames, f = item % frames
// windowed frames: p[t][i] = P(x[row], f hop - pad + i) win[i]
template <class RT>
__global__ void __launch_bounds__(256) stft_gather_kernel(const RT* __restrict__ in, RT* __restrict__ p, const RT* __restrict__ win, long long n, long long m,
                                                          long long hop, long long pad, long long frames, int reflect, long long it0, long long total) {
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
        const long long t = e / m, i = e - t * m;
        const long long row = (it0 + t) / frames, f = (it0 + t) - row * frames;
        const long long s = f * hop - pad + i;
        RT              x = (RT)0;
        if (s >= 0 && s < n) x = in[row * n + s];
        else if (reflect) x = in[row * n + stft_mirror(s, n)];
        p[e] = x * win[i];
    }
}
// out[e] = |bins[e]|^2
template <class V>
__global__ void __launch_bounds__(256) stft_power_kernel(const V* __restrict__ bins, typename real_of<V>::type* __restrict__ out, long long total) {
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
        const V x = bins[e];
        out[e] = x.x * x.x + x.y * x.y;
    }
}
// Overlap-add of the frames [f0, f0 + nf) of the rows [r0, r0 + nr) held in c [nr][nf][m], for the samples t in [t0, t1) of each row:
// every frame that reaches such a sample lies in the chunk (the host cuts rows that way).  Frames are summed in ascending order.
template <class RT>
__global__ void __launch_bounds__(256) istft_ola_kernel(const RT* __restrict__ c, RT* __restrict__ out, const RT* __restrict__ win,
                                                        const RT* __restrict__ inv_env, long long n, long long m, long long hop, long long pad, long long r0,
                                                        long long f0, long long nf, long long t0, long long t1, long long total, double inv_m) {
    const RT        sc = (RT)inv_m;
    const long long span = t1 - t0;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
        const long long rl = e / span, t = t0 + (e - rl * span);
        const long long u = t + pad;                                   // frame f holds the sample at i = u - f hop, 0 <= i < m
        long long       flo = u - m + 1 <= 0 ? 0 : (u - m + hop) / hop;  // ceil((u - m + 1) / hop)
        long long       fhi = u / hop;
        if (flo < f0) flo = f0;
        if (fhi > f0 + nf - 1) fhi = f0 + nf - 1;
        RT sum = (RT)0;
        for (long long f = flo; f <= fhi; ++f) {
            const long long i = u - f * hop;
            sum += win[i] * c[(rl * nf + (f - f0)) * m + i];
        }
        out[(r0 + rl) * n + t] = sum * inv_env[t] * sc;
    }
}

namespace {

bool tuned_half(long long M) { return tuned_built<AnyTuned>(M); }

// forward: the m windowed reals of an item, and for the power form its m/2 + 1 bins
size_t fwd_item_bytes(long long m, int dtype, int out_kind) {
    return (size_t)m * (elem_bytes(dtype) / 2) + (out_kind == STFT_OUT_POWER ? (size_t)(m / 2 + 1) * elem_bytes(dtype) : 0);
}
// inverse: the m reals of an item, and for an untuned m/2 the copy of its m/2 + 1 bins
size_t inv_item_bytes(long long m, int dtype) {
    return (size_t)m * (elem_bytes(dtype) / 2) + (tuned_half(m / 2) ? 0 : (size_t)(m / 2 + 1) * elem_bytes(dtype));
}
// items of a chunk: what fits 256 MiB, or DFFT_STFT_CHUNK_BYTES
long long chunk_items(size_t ib, long long items, long long at_least) { return chunk_units(ib, items, chunk_cap_env("DFFT_STFT_CHUNK_BYTES"), at_least); }

bool common_ok(int dtype, long long n, long long m, long long hop, long long pad, long long frames, long long rows) {
    return (dtype == F64 || dtype == F32) && n >= 1 && m >= 1 && hop >= 1 && pad >= 0 && pad < m && frames >= 1 && rows >= 1 && real_length_supported(m) &&
           stft_items_ok(rows, frames);
}
bool fwd_ok(const StftLaunch& L) {
    return common_ok(L.dtype, L.n, L.m, L.hop, L.pad, L.frames, L.rows) && (L.pad_mode == STFT_PAD_ZERO || (L.pad_mode == STFT_PAD_REFLECT && L.pad < L.n)) &&
           (L.out_kind == STFT_OUT_COMPLEX || L.out_kind == STFT_OUT_POWER) && L.frames <= stft_frames(L.n, L.m, L.hop, L.pad);
}
bool inv_ok(const IstftLaunch& L) {
    return common_ok(L.dtype, L.n, L.m, L.hop, L.pad, L.frames, L.rows) && istft_length_ok(L.n, L.m, L.hop, L.pad, L.frames);
}
// frames that one output sample sums, at most
long long frames_per_sample(long long m, long long hop, long long frames) { return std::min(frames, (m + hop - 1) / hop); }

template <class V> int stft_chunk(const StftLaunch& L, long long it0, long long ni, void* scratch, hipStream_t stream) {
    using RT = typename real_of<V>::type;
    const long long m = L.m, nbins = m / 2 + 1;
    const bool      power = L.out_kind == STFT_OUT_POWER;
    V*              bins = (V*)scratch;                            // power form: [ni][nbins], in front so that the frames stay aligned to V
    RT*             fr = (RT*)(bins + (power ? ni * nbins : 0));   // [ni][m]
    (void)hipGetLastError();
    hipLaunchKernelGGL(stft_gather_kernel<RT>, dim3(elementwise_grid(ni * m)), dim3(256), 0, stream, (const RT*)L.in, fr, (const RT*)L.win, L.n, m, L.hop, L.pad,
                       L.frames, (int)(L.pad_mode == STFT_PAD_REFLECT), it0, ni * m);
    DFFT_HIP_TRY(hipGetLastError());
    const hipError_t e = launch_real_rows(contiguous_real_rows(L.dtype, m, ni, +1, L.scale, fr, power ? (void*)bins : (void*)((V*)L.out + it0 * nbins)), stream);
    if (e != hipSuccess) return fail(DFFT_EHIP, std::string("stft (R2C rows): ") + hipGetErrorString(e));
    if (power) {
        hipLaunchKernelGGL(stft_power_kernel<V>, dim3(elementwise_grid(ni * nbins)), dim3(256), 0, stream, (const V*)bins, (RT*)L.out + it0 * nbins, ni * nbins);
        DFFT_HIP_TRY(hipGetLastError());
    }
    return DFFT_OK;
}

// frames [f0, f0 + nf) of the rows [r0, r0 + nr) -> samples [t0, t1) of those rows
template <class V> int istft_chunk(const IstftLaunch& L, long long r0, long long nr, long long f0, long long nf, long long t0, long long t1, void* scratch,
                                   hipStream_t stream) {
    using RT = typename real_of<V>::type;
    const long long m = L.m, nbins = m / 2 + 1, ni = nr * nf;
    const bool      copy = !tuned_half(m / 2);
    V*              bins = (V*)scratch;                          // untuned m/2: [ni][nbins]
    RT*             fr = (RT*)(bins + (copy ? ni * nbins : 0));  // [ni][m]
    const V*        src = (const V*)L.in + (r0 * L.frames + f0) * nbins;  // nr == 1, or f0 == 0 and nf == frames: the items are contiguous
    if (copy) {
        DFFT_HIP_TRY(hipMemcpyAsync(bins, src, (size_t)ni * nbins * sizeof(V), hipMemcpyDeviceToDevice, stream));
        src = bins;
    }
    const hipError_t e = launch_real_rows(contiguous_real_rows(L.dtype, m, ni, -1, 1.0, src, fr), stream);
    if (e != hipSuccess) return fail(DFFT_EHIP, std::string("istft (C2R rows): ") + hipGetErrorString(e));
    const long long total = nr * (t1 - t0);
    (void)hipGetLastError();
    hipLaunchKernelGGL(istft_ola_kernel<RT>, dim3(elementwise_grid(total)), dim3(256), 0, stream, (const RT*)fr, (RT*)L.out, (const RT*)L.win, (const RT*)L.inv_env,
                       L.n, m, L.hop, L.pad, r0, f0, nf, t0, t1, total, 1.0 / (double)m);
    DFFT_HIP_TRY(hipGetLastError());
    return DFFT_OK;
}

}  // namespace

long long stft_frames(long long n, long long m, long long hop, long long pad) {
    if (n < 1 || m < 1 || hop < 1 || pad < 0 || pad >= m || n + 2 * pad < m) return 0;
    return 1 + (n + 2 * pad - m) / hop;
}

bool stft_fused_env() { return env_switch_on("DFFT_STFT_FUSED"); }

bool stft_vec(const void* in, long long n, long long hop, long long pad, int dtype) {
    return n % 2 == 0 && hop % 2 == 0 && pad % 2 == 0 && (uintptr_t)in % elem_bytes(dtype) == 0;
}

bool stft_fused(long long m, int dtype) {
    if ((dtype != F64 && dtype != F32) || m < 4 || m % 2 || !real_length_supported(m)) return false;
    return tuned_built<StftTag>(m / 2, dtype == F64);
}

size_t stft_scratch_bytes(const StftLaunch& L, bool fused_on) {
    if (!fwd_ok(L)) return 0;
    if (fused_on && stft_fused(L.m, L.dtype)) return 0;
    const size_t ib = fwd_item_bytes(L.m, L.dtype, L.out_kind);
    return (size_t)chunk_items(ib, L.rows * L.frames, 1) * ib;
}

size_t istft_scratch_bytes(const IstftLaunch& L) {
    if (!inv_ok(L)) return 0;
    const size_t ib = inv_item_bytes(L.m, L.dtype);
    return (size_t)chunk_items(ib, L.rows * L.frames, frames_per_sample(L.m, L.hop, L.frames)) * ib;
}

int stft(const StftLaunch& L, bool fused_on, void* scratch, size_t scratch_bytes, hipStream_t stream) {
    if (!L.in || !L.out || !L.win || !fwd_ok(L)) return fail(DFFT_EINVAL, "stft: bad arguments");
    const long long items = L.rows * L.frames;
    if (fused_on && stft_fused(L.m, L.dtype)) {
        StftFusedLaunch F;
        std::memset(&F, 0, sizeof(F));
        F.dtype = L.dtype;
        F.power = L.out_kind == STFT_OUT_POWER;
        F.vec = stft_vec(L.in, L.n, L.hop, L.pad, L.dtype);
        F.reflect = L.pad_mode == STFT_PAD_REFLECT;
        F.n = L.n;
        F.m = L.m;
        F.hop = L.hop;
        F.pad = L.pad;
        F.frames = L.frames;
        F.items = items;
        F.scale = L.scale;
        F.in = L.in;
        F.out = L.out;
        F.win = L.win;
        if (int rc = get_twiddles((int)(L.m / 2), L.dtype, &F.tw)) return rc;
        if (int rc = get_twiddles((int)L.m, L.dtype, &F.twh)) return rc;
        const hipError_t e = run_tuned<StftTag>(L.m / 2, F, stream);
        if (e == hipSuccess) return DFFT_OK;
        return fail(DFFT_EHIP, std::string("stft (fused): ") + hipGetErrorString(e));
    }
    // chunks of items whose windowed frames (and bins) fit the scratch buffer
    const size_t ib = fwd_item_bytes(L.m, L.dtype, L.out_kind);
    const long long ni = fit_chunk_to_lease("stft", chunk_items(ib, items, 1), ib, scratch, scratch_bytes);
    if (ni < 1) return DFFT_EINVAL;
    for (long long i0 = 0; i0 < items; i0 += ni) {
        const long long k = std::min(ni, items - i0);
        const int       rc = L.dtype == F64 ? stft_chunk<double2>(L, i0, k, scratch, stream) : stft_chunk<float2>(L, i0, k, scratch, stream);
        if (rc) return rc;
    }
    return DFFT_OK;
}

int istft(const IstftLaunch& L, void* scratch, size_t scratch_bytes, hipStream_t stream) {
    if (!L.in || !L.out || !L.win || !L.inv_env || !inv_ok(L)) return fail(DFFT_EINVAL, "istft: bad arguments");
    const size_t    ib = inv_item_bytes(L.m, L.dtype);
    const long long per = frames_per_sample(L.m, L.hop, L.frames);
    const long long ni = fit_chunk_to_lease("istft", chunk_items(ib, L.rows * L.frames, per), ib, scratch, scratch_bytes, per);
    if (ni < 1) return DFFT_EINVAL;
    const auto run = [&](long long r0, long long nr, long long f0, long long nf, long long t0, long long t1) {
        return L.dtype == F64 ? istft_chunk<double2>(L, r0, nr, f0, nf, t0, t1, scratch, stream)
                              : istft_chunk<float2>(L, r0, nr, f0, nf, t0, t1, scratch, stream);
    };
    if (L.frames <= ni) {  // whole rows
        const long long rpc = ni / L.frames;
        for (long long r0 = 0; r0 < L.rows; r0 += rpc)
            if (int rc = run(r0, std::min(rpc, L.rows - r0), 0, L.frames, 0, L.n)) return rc;
        return DFFT_OK;
    }
    // A row is cut at output samples: the cut that starts at sample t0 begins with the first frame that reaches t0, holds ni >= per
    // frames, and ends before the first sample that the frame behind its last one reaches.
    for (long long r = 0; r < L.rows; ++r) {
        for (long long t0 = 0; t0 < L.n;) {
            const long long u = t0 + L.pad;
            const long long f0 = u - L.m + 1 <= 0 ? 0 : (u - L.m + L.hop) / L.hop;
            const long long f1 = std::min(L.frames, f0 + ni);
            const long long t1 = f1 == L.frames ? L.n : std::min(L.n, f1 * L.hop - L.pad);
            if (t1 <= t0) return fail(DFFT_EHIP, "istft: a cut of a row made no progress");
            if (int rc = run(r, 1, f0, f1 - f0, t0, t1)) return rc;
            t0 = t1;
        }
    }
    return DFFT_OK;
}

#endif

}  // namespace dfft
