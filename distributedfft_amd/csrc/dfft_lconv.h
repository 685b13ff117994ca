// dfft_lconv.h -- host-side interface of the long batched 1-D real FFT convolution (dfft_lconv.hip): every row of reals
// [batch][channels][n] filtered by its channel's spectrum, y = irfft(rfft(x, m) * H, m)[:n], for padded lengths beyond the single-pass
// range of dfft_rconv.hip: m even, 8192 < m <= 2^23, m/2 = N1 * N2 a product of two tuned single-pass lengths (four-step).  Internal
// header (the C-ABI is include/dfft.h: dfft_rconv1d_long).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

#include "dfft_rconv.h"

namespace dfft {

// Row r of the batch * channels rows of n reals (contiguous) uses filter row r % channels of hp [channels][m/2 + 1], the filter in the
// layout of lconv_filter.  `out` == `in` (exactly) is allowed; otherwise the two do not overlap and `in` is never written.
struct LconvLaunch {
    int         dtype;        // DType: F64 = double, F32 = float
    int         filter_kind;  // RCONV_FILTER_*
    long long   n, m, channels, batch;
    const void* in;
    void*       out;
    const void* hp;
};

// Lengths of the two factors: every 2^a, 3 * 2^a, 5 * 2^a in [64, 2048], 81 and 125 (all with tuned plans, dfft_plans.h)
constexpr bool lconv_factor(long long N) {
    if (N == 81 || N == 125) return true;
    if (N < 64 || N > 2048) return false;
    while (N % 2 == 0) N /= 2;
    return N == 1 || N == 3 || N == 5;
}
// m even, 8192 < m <= 2^23, m/2 = N1 * N2 with both factors lconv_factor lengths: the most balanced such pair, N1 <= N2.
bool lconv_split(long long m, int* n1, int* n2);
// Smallest accepted m >= at_least; 0 if none.
long long lconv_length(long long at_least);
// DFFT_RCONV_LONG_FUSED, read per call: "0" sends every length to the composed route.
bool lconv_fused_env();
// The three-launch pipeline runs m: its split's kernels for `dtype` keep nothing in scratch memory (lconv_fused_ok) and were not measured
// slower than the composed route.  Depends on (m, dtype) alone.
bool lconv_fused(long long m, int dtype);
// Rows per chunk of the pipeline (their m/2 complex of scratch each within max(256 MiB, one row's)) and the scratch of such a chunk
long long lconv_chunk_rows(long long m, int dtype, long long rows, size_t cap);
size_t    lconv_scratch_bytes(long long m, int dtype, long long rows, size_t cap);
// The pipeline of L on `scratch` (lconv_scratch_bytes(L.m, L.dtype, rows) bytes, aliasing none of in, out, hp): per chunk of rows pass A
// (N1-point columns of the row seen as [N1][N2] complex, times W_M^{k1 j2}, into scratch), Mid (N2-point forward, pair / multiply /
// merge, N2-point inverse, per pair of scratch rows, in place) and pass C (times W_M^{-k1 j2}, N1-point inverse columns, the first n
// reals into `out`).  Enqueues on `stream` only; allocates nothing once the twiddle tables of (device, m, dtype) exist.
int lconv_run(const LconvLaunch& L, size_t cap, void* scratch, size_t scratch_bytes, hipStream_t stream);

// hp[c][k1 N2 + k2] = h[c][k1 + N1 k2], hp[c][M] = h[c][M]: `count` = channels * (M + 1) elements of `esize` bytes (8 or 16: the real
// or complex type of F64; 4 or 8 of F32)
int lconv_filter(const void* h, void* hp, long long m, long long channels, int esize, hipStream_t stream);

// The multiply of the composed route between the real transforms of length m (dfft_batch.cpp runs those, and pad_rows / trunc_rows of
// dfft_rows_common.h around them): bins [nr][m/2 + 1] *= H / m with H read from hp (rows row0 ... of the call).
int lconv_mul(void* bins, const void* hp, long long m, long long row0, long long channels, long long nr, int dtype, int filter_kind, hipStream_t stream);

}  // namespace dfft
