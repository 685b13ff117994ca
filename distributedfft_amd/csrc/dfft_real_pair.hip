// dfft_real_pair.hip -- real-to-complex / complex-to-real rows of ANY length n by the two-for-one method: rows a and b (2p and 2p + 1)
// are packed into one complex row z = a + i b, and one n-point complex transform gives both spectra
//     A[k] = (Z[k] + conj Z[(n-k) mod n]) / 2,   B[k] = (Z[k] - conj Z[(n-k) mod n]) / (2i),   k = 0 .. n/2.
// The inverse builds Z[k] = A[k] + i B[k] (k <= n/2) and conj A[n-k] + i conj B[n-k] (k > n/2) from the two bin rows -- the imaginary
// parts of bin 0 and, n even, bin n/2 taken as zero (numpy's rule) -- runs the inverse n-point transform and stores Re into row a and
// Im into row b: n * numpy.fft.irfft of each row for any input.  Works for every n with an n-point complex transform, odd n included;
// the HBM bytes per row are those of the half-length method of dfft_real.hip.  The two rows of a pair share one transform, so each
// row's rounding error is bounded relative to the pair's combined magnitude, not its own.
//
// Forms (dfft_real_form 2 and 3; form 1, the half-length kernels of dfft_real.hip, does not come through here):
//   * n odd with a tuned plan (dfft_plans.h: 3 5 7 9 25 27 49 81 125 243 343 625 729 2187 2401 3125): ONE launch,
//     r2c_pair_rows_kernel / c2r_pair_rows_kernel -- the C2C row kernel's geometry (RealGeom of dfft_real.hip): a thread group loads
//     the two real rows as z, runs run_stages (dfft_fft_impl.h), and (R2C) puts Z in LDS in natural order; after one barrier the thread
//     holding Z[k] stores A[k] for k <= n/2 and B[n-k] for k > n/2, so every thread stores about one bin per point.  C2R builds Z at
//     load time from the two bin rows and needs no exchange besides the stages'.
//   * every other n (the remaining single-pass lengths through the row kernels -- 2, and the odd ones the run-time-scheduled kernel
//     of dfft_generic.hip serves --, four-step lengths through long_fft, Bluestein lengths through bluestein_fft), per batch chunk:
//     r2c_pair_pack_kernel -> n-point transform in scratch -> r2c_pair_split_kernel, or c2r_pair_merge_kernel -> inverse transform
//     -> c2r_pair_unpack_kernel.  Chunks keep the packed rows within max(256 MiB, one pair's).
// An odd last row is paired with a zero row (R2C) or its partner's output is dropped (C2R): nothing outside the caller's rows is read
// or written.  Rows are addressed as (plane, row) pairs, so a pair may straddle a plane boundary.
//
// Compiled once per instantiation group (-DDFFT_INST_GROUP=g: the fused kernels of the odd tuned lengths of group g) and once with
// -DDFFT_INST_GROUP=DFFT_NUM_INST_GROUPS (the dispatcher and the pack / split / merge / unpack kernels).
#include "dfft_fused_host.h"
#include "dfft_bluestein.h"
#include "dfft_long.h"
#include "dfft_real_pair.h"

#include <algorithm>
#include <atomic>
#include <cstring>

#ifndef DFFT_INST_GROUP
#error "compile with -DDFFT_INST_GROUP=<g>"
#endif

namespace dfft {

// element offset of row r of a (plane, row) tiling
__device__ __forceinline__ long long pair_row_off(unsigned r, unsigned rows_per_plane, long long pitch, long long plane) {
    const unsigned a = r / rows_per_plane, b = r - a * rows_per_plane;
    return (long long)a * plane + (long long)b * pitch;
}

// Geometry: the C2C row kernel's (one n-point FFT per thread group, about 256 threads per workgroup); the LDS tile of a group also holds
// the n points of the split step in natural order
template <class V, class P> struct PairGeom {
    static constexpr int G = ConstMax1<256 / P::T>::value;
    using KG = KernelGeom<V, P, 1, G, TuneDefault>;
    static constexpr int SPLIT = KG::PAD ? P::N + P::N / 8 : P::N;  // > lds_index<1, PAD>(N - 1)
    static constexpr int EXR = ((KG::LDS_ELEMS > SPLIT ? KG::LDS_ELEMS : SPLIT) + 1) / 2 * 2;
    static constexpr size_t LDS_BYTES = (size_t)EXR * G * sizeof(V) + KG::TW_BYTES;
};

// R2C: real rows (strides in reals) -> bin rows (n/2 + 1 bins; strides in complex elements)
template <class V, class P>
__global__ void __attribute__((amdgpu_flat_work_group_size(1, PairGeom<V, P>::KG::THREADS)))
r2c_pair_rows_kernel(const typename real_of<V>::type* __restrict__ in, V* __restrict__ out, const typename VecTraits<V>::W* __restrict__ tw,
                     unsigned rows, unsigned rows_per_plane, long long ipitch, long long iplane, long long opitch, long long oplane) {
    using PG = PairGeom<V, P>;
    using KG = typename PG::KG;
    using W = typename VecTraits<V>::W;
    using RT = typename real_of<V>::type;
    constexpr int E = P::E, T = P::T, N = P::N, G = PG::G, GT = KG::GT;
    constexpr bool TWPOW = KG::TWMODE == TW_REG;
    extern __shared__ __attribute__((aligned(16))) char dfft_smem[];
    const int g = threadIdx.x / GT;
    const int j = tile_j<1, KG::NW>((int)threadIdx.x - g * GT);
    V*        lds = reinterpret_cast<V*>(dfft_smem + KG::TW_BYTES) + g * PG::EXR;
    W         twreg[KG::TWMODE == TW_REG && KG::TWN > 0 ? KG::TWN : 1];
    const W*  twr = stage_twiddles<V, P, +1, KG>(twreg, reinterpret_cast<W*>(dfft_smem), tw, j);
    const RT  half = (RT)0.5;
    const unsigned pairs = (rows + 1) / 2;
    for (unsigned p0 = blockIdx.x * G; p0 < pairs; p0 += gridDim.x * G) {
        const unsigned pr = p0 + g;
        const bool     va = pr < pairs, vb = va && 2 * pr + 1 < rows;
        const RT*      ia = in + (va ? pair_row_off(2 * pr, rows_per_plane, ipitch, iplane) : 0);
        const RT*      ib = in + (vb ? pair_row_off(2 * pr + 1, rows_per_plane, ipitch, iplane) : 0);
        V              v[E];
#pragma unroll
        for (int k = 0; k < E; ++k) {
            const int kk = j + T * k;
            v[k] = V{va ? ia[kk] : (RT)0, vb ? ib[kk] : (RT)0};
        }
        run_stages<V, P, 0, +1, 1, KG::PAD, KG::WAVE_LOCAL, KG::TWMODE, TWPOW, 1, 1, KG::NW, KG::LOCALX>(v, twr, lds, j, 0);
        group_sync<KG::WAVE_LOCAL>();
#pragma unroll
        for (int k = 0; k < E; ++k) lds[lds_index<1, KG::PAD>(j + T * k, 0)] = v[k];
        group_sync<KG::WAVE_LOCAL>();
        if (va) {
            V* oa = out + pair_row_off(2 * pr, rows_per_plane, opitch, oplane);
            V* ob = vb ? out + pair_row_off(2 * pr + 1, rows_per_plane, opitch, oplane) : oa;
#pragma unroll
            for (int k = 0; k < E; ++k) {
                const int kk = j + T * k, km = kk == 0 ? 0 : N - kk;
                const V   zm = lds[lds_index<1, KG::PAD>(km, 0)];
                if (2 * kk <= N) {  // A[kk] (and B[kk] for the self-paired bins 0 and n/2)
                    oa[kk] = V{(v[k].x + zm.x) * half, (v[k].y - zm.y) * half};
                    if (vb && (kk == 0 || 2 * kk == N)) ob[kk] = V{(v[k].y + zm.y) * half, (zm.x - v[k].x) * half};
                } else if (vb) {  // B[n - kk] from Z[n - kk] = zm and its partner Z[kk]
                    ob[km] = V{(zm.y + v[k].y) * half, (v[k].x - zm.x) * half};
                }
            }
        }
        group_sync<KG::WAVE_LOCAL>();  // the next pair's exchanges reuse the tile
    }
}

// C2R: bin rows (strides in complex elements) -> real rows (strides in reals)
template <class V, class P>
__global__ void __attribute__((amdgpu_flat_work_group_size(1, PairGeom<V, P>::KG::THREADS)))
c2r_pair_rows_kernel(const V* __restrict__ in, typename real_of<V>::type* __restrict__ out, const typename VecTraits<V>::W* __restrict__ tw,
                     unsigned rows, unsigned rows_per_plane, long long ipitch, long long iplane, long long opitch, long long oplane) {
    using PG = PairGeom<V, P>;
    using KG = typename PG::KG;
    using W = typename VecTraits<V>::W;
    using RT = typename real_of<V>::type;
    constexpr int E = P::E, T = P::T, N = P::N, G = PG::G, GT = KG::GT;
    constexpr bool TWPOW = KG::TWMODE == TW_REG;
    extern __shared__ __attribute__((aligned(16))) char dfft_smem[];
    const int g = threadIdx.x / GT;
    const int j = tile_j<1, KG::NW>((int)threadIdx.x - g * GT);
    V*        lds = reinterpret_cast<V*>(dfft_smem + KG::TW_BYTES) + g * PG::EXR;
    W         twreg[KG::TWMODE == TW_REG && KG::TWN > 0 ? KG::TWN : 1];
    const W*  twr = stage_twiddles<V, P, -1, KG>(twreg, reinterpret_cast<W*>(dfft_smem), tw, j);
    const unsigned pairs = (rows + 1) / 2;
    for (unsigned p0 = blockIdx.x * G; p0 < pairs; p0 += gridDim.x * G) {
        const unsigned pr = p0 + g;
        const bool     va = pr < pairs, vb = va && 2 * pr + 1 < rows;
        const V*       ia = in + (va ? pair_row_off(2 * pr, rows_per_plane, ipitch, iplane) : 0);
        const V*       ib = in + (vb ? pair_row_off(2 * pr + 1, rows_per_plane, ipitch, iplane) : 0);
        V              v[E];
#pragma unroll
        for (int k = 0; k < E; ++k) {
            const int  kk = j + T * k;
            const bool lo = 2 * kk <= N;
            const int  m = lo ? kk : N - kk;
            V          a = va ? ia[m] : V{0, 0};
            V          b = vb ? ib[m] : V{0, 0};
            if (m == 0 || 2 * m == N) {  // the imaginary parts of the DC and Nyquist bins are ignored
                a.y = (RT)0;
                b.y = (RT)0;
            }
            v[k] = lo ? V{a.x - b.y, a.y + b.x} : V{a.x + b.y, b.x - a.y};  // A + i B, or conj A + i conj B
        }
        group_sync<KG::WAVE_LOCAL>();  // the previous pair's stages are done with the tile
        run_stages<V, P, 0, -1, 1, KG::PAD, KG::WAVE_LOCAL, KG::TWMODE, TWPOW, 1, 1, KG::NW, KG::LOCALX>(v, twr, lds, j, 0);
        if (va) {
            RT* oa = out + pair_row_off(2 * pr, rows_per_plane, opitch, oplane);
#pragma unroll
            for (int k = 0; k < E; ++k) oa[j + T * k] = v[k].x;
            if (vb) {
                RT* ob = out + pair_row_off(2 * pr + 1, rows_per_plane, opitch, oplane);
#pragma unroll
                for (int k = 0; k < E; ++k) ob[j + T * k] = v[k].y;
            }
        }
    }
}

template <class V, class P> hipError_t launch_pair_plan(const RealPairLaunch& L, const void* tw, hipStream_t stream) {
    using PG = PairGeom<V, P>;
    using W = typename VecTraits<V>::W;
    using RT = typename real_of<V>::type;
    const bool              fwd = L.dir > 0;
    const void*             kern = fwd ? reinterpret_cast<const void*>(r2c_pair_rows_kernel<V, P>) : reinterpret_cast<const void*>(c2r_pair_rows_kernel<V, P>);
    static std::atomic<int> blocks_per_cu[2][kMaxDevices];  // per kernel: R2C, C2R
    hipError_t              e;
    const int               bpc = resident_blocks_per_cu(kern, PG::KG::THREADS, PG::LDS_BYTES, blocks_per_cu[fwd ? 0 : 1], &e);
    if (bpc == 0) return e;
    const long long pairs = (L.rows + 1) / 2;
    const long long grid = persistent_grid(device_info().cus, bpc, (pairs + PG::G - 1) / PG::G);
    if (grid < 1) return hipSuccess;
    (void)hipGetLastError();
    if (fwd)
        hipLaunchKernelGGL((r2c_pair_rows_kernel<V, P>), dim3((unsigned)grid), dim3(PG::KG::THREADS), PG::LDS_BYTES, stream, (const RT*)L.in, (V*)L.out,
                           (const W*)tw, (unsigned)L.rows, (unsigned)L.rows_per_plane, L.rpitch, L.rplane, L.cpitch, L.cplane);
    else
        hipLaunchKernelGGL((c2r_pair_rows_kernel<V, P>), dim3((unsigned)grid), dim3(PG::KG::THREADS), PG::LDS_BYTES, stream, (const V*)L.in, (RT*)L.out,
                           (const W*)tw, (unsigned)L.rows, (unsigned)L.rows_per_plane, L.cpitch, L.cplane, L.rpitch, L.rplane);
    return hipGetLastError();
}

// entry point of the odd tuned length N: defined (and explicitly instantiated) in the translation unit of N's group only
template <bool ON, int N> struct PairInst {};
template <int N> struct PairInst<true, N> {
    static hipError_t run(const RealPairLaunch& L, const void* tw, hipStream_t stream);
};

#if DFFT_INST_GROUP < DFFT_NUM_INST_GROUPS

template <int N> hipError_t PairInst<true, N>::run(const RealPairLaunch& L, const void* tw, hipStream_t stream) {
    if (L.dtype == F64) return launch_pair_plan<double2, typename PlanFor<N>::type>(L, tw, stream);
    if (L.dtype == F32) return launch_pair_plan<float2, typename PlanFor<N>::type>(L, tw, stream);
    return hipErrorInvalidValue;
}
#define DFFT_PAIR_INST(N, GRP, E, ...) template struct PairInst<(GRP == DFFT_INST_GROUP && N % 2 == 1), N>;
DFFT_PLAN_TABLE(DFFT_PAIR_INST)
#undef DFFT_PAIR_INST

#else  // the dispatcher, and the kernels of the multi-launch form

template <int N> hipError_t pair_fused_run(const RealPairLaunch& L, const void* tw, hipStream_t stream) {
    if constexpr (N % 2 == 1) return PairInst<true, N>::run(L, tw, stream);
    return hipErrorInvalidValue;
}

// Z[p][k] = a[k] + i b[k] for the rows a = row0 + 2p, b = row0 + 2p + 1 (a zero row past nrows)   (e runs over pairs * n)
template <class V>
__global__ void __launch_bounds__(256) r2c_pair_pack_kernel(const typename real_of<V>::type* __restrict__ in, V* __restrict__ z, unsigned n,
                                                            unsigned row0, unsigned nrows, unsigned rows_per_plane, long long pitch,
                                                            long long plane, unsigned total) {
    using RT = typename real_of<V>::type;
    for (unsigned e = blockIdx.x * 256u + threadIdx.x; e < total; e += gridDim.x * 256u) {
        const unsigned p = e / n, k = e - p * n, r = 2 * p;
        const RT       a = in[pair_row_off(row0 + r, rows_per_plane, pitch, plane) + k];
        const RT       b = r + 1 < nrows ? in[pair_row_off(row0 + r + 1, rows_per_plane, pitch, plane) + k] : (RT)0;
        z[e] = V{a, b};
    }
}

// A[m], B[m] (m <= n/2) of every pair from Z   (e runs over pairs * (n/2 + 1))
template <class V>
__global__ void __launch_bounds__(256) r2c_pair_split_kernel(const V* __restrict__ z, V* __restrict__ out, unsigned n, unsigned row0,
                                                             unsigned nrows, unsigned rows_per_plane, long long pitch, long long plane,
                                                             unsigned total) {
    using RT = typename real_of<V>::type;
    const unsigned nh = n / 2 + 1;
    const RT       half = (RT)0.5;
    for (unsigned e = blockIdx.x * 256u + threadIdx.x; e < total; e += gridDim.x * 256u) {
        const unsigned p = e / nh, m = e - p * nh, r = 2 * p;
        const V        zk = z[(size_t)p * n + m], zm = z[(size_t)p * n + (m == 0 ? 0 : n - m)];
        out[pair_row_off(row0 + r, rows_per_plane, pitch, plane) + m] = V{(zk.x + zm.x) * half, (zk.y - zm.y) * half};
        if (r + 1 < nrows) out[pair_row_off(row0 + r + 1, rows_per_plane, pitch, plane) + m] = V{(zk.y + zm.y) * half, (zm.x - zk.x) * half};
    }
}

// Z[p][k] from the two bin rows of pair p (conjugates above n/2; imaginary parts of bins 0 and n/2 ignored)   (e runs over pairs * n)
template <class V>
__global__ void __launch_bounds__(256) c2r_pair_merge_kernel(const V* __restrict__ in, V* __restrict__ z, unsigned n, unsigned row0,
                                                             unsigned nrows, unsigned rows_per_plane, long long pitch, long long plane,
                                                             unsigned total) {
    using RT = typename real_of<V>::type;
    for (unsigned e = blockIdx.x * 256u + threadIdx.x; e < total; e += gridDim.x * 256u) {
        const unsigned p = e / n, k = e - p * n, r = 2 * p;
        const bool     lo = 2 * k <= n;
        const unsigned m = lo ? k : n - k;
        V              a = in[pair_row_off(row0 + r, rows_per_plane, pitch, plane) + m];
        V              b = r + 1 < nrows ? in[pair_row_off(row0 + r + 1, rows_per_plane, pitch, plane) + m] : V{0, 0};
        if (m == 0 || 2 * m == n) {
            a.y = (RT)0;
            b.y = (RT)0;
        }
        z[e] = lo ? V{a.x - b.y, a.y + b.x} : V{a.x + b.y, b.x - a.y};
    }
}

// row a = Re Z, row b = Im Z (dropped past nrows)   (e runs over pairs * n)
template <class V>
__global__ void __launch_bounds__(256) c2r_pair_unpack_kernel(const V* __restrict__ z, typename real_of<V>::type* __restrict__ out, unsigned n,
                                                              unsigned row0, unsigned nrows, unsigned rows_per_plane, long long pitch,
                                                              long long plane, unsigned total) {
    for (unsigned e = blockIdx.x * 256u + threadIdx.x; e < total; e += gridDim.x * 256u) {
        const unsigned p = e / n, k = e - p * n, r = 2 * p;
        const V        v = z[e];
        out[pair_row_off(row0 + r, rows_per_plane, pitch, plane) + k] = v.x;
        if (r + 1 < nrows) out[pair_row_off(row0 + r + 1, rows_per_plane, pitch, plane) + k] = v.y;
    }
}

namespace {

// packed pairs per batch chunk (at most max(256 MiB, one pair's) of them), and the scratch such a chunk needs
long long chunk_pairs(long long n, int dtype, long long pairs, size_t cap) {
    const size_t zb = (size_t)n * elem_bytes(dtype);
    return chunk_units(zb, pairs, cap);
}
size_t chunk_bytes(long long n, int dtype, long long np, const BluesteinTables* T, bool fused, size_t cap) {
    const size_t zb = (size_t)np * n * elem_bytes(dtype);
    if (T) return zb + bluestein_scratch_bytes(*T, 1, np, fused, cap);
    return n > 4096 ? 2 * zb : zb;  // four-step: long_fft's scratch as large as its data
}

// n-point transforms of the np packed rows in z, in place
int pair_fft(void* z, long long np, const RealPairLaunch& L, const BluesteinTables* T, bool fused, void* inner, size_t inner_bytes,
             hipStream_t stream) {
    if (T) return bluestein_fft(*T, z, z, 1, np, 1.0, fused, inner, inner_bytes, stream);
    if (L.n > 4096) return long_fft(z, z, L.n, 1, np, L.dtype, L.dir, 1.0, inner, stream);
    const void* tw = nullptr;
    if (int rc = get_twiddles((int)L.n, L.dtype, &tw)) return rc;
    FftLaunch F;
    std::memset(&F, 0, sizeof(F));
    F.dtype = L.dtype;
    F.n = (int)L.n;
    F.dir = L.dir;
    F.cols = 0;
    F.in = z;
    F.out = z;
    F.tw = tw;
    F.imap = F.omap = AxisMap{(int)L.n, 1, 0, 1, 0, 0, 1, 0};
    F.itile = F.otile = TileMap{L.n, 0};
    F.ntiles = np;
    F.tiles_per_a = 1;
    F.ncols = 1;
    const hipError_t e = launch_fft(F, stream);
    if (e == hipSuccess) return DFFT_OK;
    return fail(DFFT_EHIP, std::string("real pair rows: n-point transform: ") + hipGetErrorString(e));
}

template <class V>
int pair_chunk(const RealPairLaunch& L, long long r0, long long nr, const BluesteinTables* T, bool fused, void* z, void* inner,
               size_t inner_bytes, hipStream_t stream) {
    using RT = typename real_of<V>::type;
    const unsigned  n = (unsigned)L.n, rpp = (unsigned)L.rows_per_plane;
    const long long np = (nr + 1) / 2, tz = np * (long long)n, tb = np * (long long)(n / 2 + 1);
    (void)hipGetLastError();
    if (L.dir > 0) {
        hipLaunchKernelGGL(r2c_pair_pack_kernel<V>, dim3(elementwise_grid(tz)), dim3(256), 0, stream, (const RT*)L.in, (V*)z, n, (unsigned)r0, (unsigned)nr,
                           rpp, L.rpitch, L.rplane, (unsigned)tz);
        DFFT_HIP_TRY(hipGetLastError());
        if (int rc = pair_fft(z, np, L, T, fused, inner, inner_bytes, stream)) return rc;
        hipLaunchKernelGGL(r2c_pair_split_kernel<V>, dim3(elementwise_grid(tb)), dim3(256), 0, stream, (const V*)z, (V*)L.out, n, (unsigned)r0, (unsigned)nr,
                           rpp, L.cpitch, L.cplane, (unsigned)tb);
        DFFT_HIP_TRY(hipGetLastError());
    } else {
        hipLaunchKernelGGL(c2r_pair_merge_kernel<V>, dim3(elementwise_grid(tz)), dim3(256), 0, stream, (const V*)L.in, (V*)z, n, (unsigned)r0, (unsigned)nr,
                           rpp, L.cpitch, L.cplane, (unsigned)tz);
        DFFT_HIP_TRY(hipGetLastError());
        if (int rc = pair_fft(z, np, L, T, fused, inner, inner_bytes, stream)) return rc;
        hipLaunchKernelGGL(c2r_pair_unpack_kernel<V>, dim3(elementwise_grid(tz)), dim3(256), 0, stream, (const V*)z, (RT*)L.out, n, (unsigned)r0, (unsigned)nr,
                           rpp, L.rpitch, L.rplane, (unsigned)tz);
        DFFT_HIP_TRY(hipGetLastError());
    }
    return DFFT_OK;
}

}  // namespace

bool real_pair_fused(long long n) {
    switch (n) {
#define DFFT_PAIR_TUNED(N, GRP, E, ...) case N:
        DFFT_PLAN_TABLE(DFFT_PAIR_TUNED)
#undef DFFT_PAIR_TUNED
        return n % 2 == 1;
        default: return false;
    }
}

size_t real_pair_scratch_bytes(long long n, int dtype, long long rows, const BluesteinTables* T, bool bluestein_fused, size_t cap) {
    if (n < 1 || rows <= 0 || real_pair_fused(n)) return 0;
    return chunk_bytes(n, dtype, chunk_pairs(n, dtype, (rows + 1) / 2, cap), T, bluestein_fused, cap);
}

int real_pair_rows(const RealPairLaunch& L, const BluesteinTables* T, bool bluestein_fused, size_t cap, void* scratch, size_t scratch_bytes,
                   hipStream_t stream) {
    if (L.n < 1 || (L.dir != 1 && L.dir != -1) || (L.dtype != F64 && L.dtype != F32) || !L.in || !L.out)
        return fail(DFFT_EINVAL, "real pair rows: bad arguments");
    if (L.rows <= 0) return DFFT_OK;
    if (L.rows >= (1ll << 31) || L.rows_per_plane < 1 || L.rows_per_plane >= (1ll << 31))
        return fail(DFFT_EINVAL, "real pair rows: more than 2^31 rows");
    if (T && (T->n != L.n || T->dtype != L.dtype || T->dir != L.dir)) return fail(DFFT_EINVAL, "real pair rows: Bluestein tables of another transform");
    if (real_pair_fused(L.n)) {
        const void* tw = nullptr;
        if (int rc = get_twiddles((int)L.n, L.dtype, &tw)) return rc;
        hipError_t e = hipErrorInvalidValue;
        switch (L.n) {
#define DFFT_PAIR_CASE(N, GRP, E, ...) \
    case N: e = pair_fused_run<N>(L, tw, stream); break;
            DFFT_PLAN_TABLE(DFFT_PAIR_CASE)
#undef DFFT_PAIR_CASE
            default: break;
        }
        if (e == hipSuccess) return DFFT_OK;
        return fail(DFFT_EHIP, std::string(L.dir > 0 ? "R2C pair rows: " : "C2R pair rows: ") + hipGetErrorString(e));
    }
    if (!T && L.n > 4096) {
        int a, b;
        if (!long_split(L.n, &a, &b)) return fail(DFFT_EINVAL, "real pair rows: length " + std::to_string(L.n) + " needs Bluestein tables");
    }
    // batch chunks of whole pairs that fit the scratch
    long long np = chunk_pairs(L.n, L.dtype, (L.rows + 1) / 2, cap);
    while (np > 1 && chunk_bytes(L.n, L.dtype, np, T, bluestein_fused, cap) > scratch_bytes) np = (np + 1) / 2;
    if (!scratch || chunk_bytes(L.n, L.dtype, np, T, bluestein_fused, cap) > scratch_bytes) return fail(DFFT_EINVAL, "real pair rows: scratch buffer too small");
    const size_t zb = (size_t)np * L.n * elem_bytes(L.dtype);
    void*        inner = (char*)scratch + zb;
    const size_t inner_bytes = scratch_bytes - zb;
    for (long long r0 = 0; r0 < L.rows; r0 += 2 * np) {
        const long long nr = std::min(2 * np, L.rows - r0);
        const int       rc = L.dtype == F64 ? pair_chunk<double2>(L, r0, nr, T, bluestein_fused, scratch, inner, inner_bytes, stream)
                                            : pair_chunk<float2>(L, r0, nr, T, bluestein_fused, scratch, inner, inner_bytes, stream);
        if (rc) return rc;
    }
    return DFFT_OK;
}

#endif

}  // namespace dfft
