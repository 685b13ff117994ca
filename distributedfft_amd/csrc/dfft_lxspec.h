// dfft_lxspec.h -- host-side interface of the long batched 1-D real cross-spectrum (dfft_lxspec.hip): the rows of two real fields
// [batch][channels][n], zero-padded to m, reduced over the batch to S[c][k] = sum_b conj(rfft(x[b, c], m)[k]) rfft(g[b, c], m)[k], for the
// padded lengths of dfft_lconv.h (m even, 8192 < m <= 2^23, m/2 = N1 * N2): the filter gradient of dfft_rconv1d_long.  Internal header
// (the C-ABI is include/dfft.h: dfft_rxspec1d_long).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

namespace dfft {

// Row (b, c) of either field holds n contiguous reals at ((b * channels) + c) * n.  g == x (exactly) is the auto-spectrum; out
// [channels][m/2 + 1] complex overlaps neither field, and neither field is ever written.  order 0: out[c][k] = S[c][k]; order 1: the
// order of lconv_filter, out[c][k1 N2 + k2] = S[c][k1 + N1 k2], out[c][M] = S[c][M].
struct LxspecLaunch {
    int         dtype;  // DType: F64 = double, F32 = float
    int         order;
    long long   n, m, channels, batch;
    const void* x;
    const void* g;
    void*       out;
};

// Fixed constants of the cuts (never the device): see lxspec_slices (lxspec_chunk_rows: the cap of chunk_cap_env)
constexpr long long kLxspecTargetItems = 2048;  // (slice, channel, row pair) items worth cutting the batch for
constexpr long long kLxspecMinSteps = 8;        // rows of a channel in a slice, at least

// DFFT_RXSPEC_LONG_FUSED, read per call: "0" sends every length to the composed route.
bool lxspec_fused_env();
// The fused route runs m: the kernels of its split for `dtype` keep nothing in scratch memory (lxspec_fused_ok).  (m, dtype) alone.
bool lxspec_fused(long long m, int dtype);
// Rows per chunk of the fused route: the batch * channels rows are cut, in order, into chunks whose pass-A results (m/2 complex per row
// and field, two fields counted also for the auto-spectrum) fit max(256 MiB, one row's).
long long lxspec_chunk_rows(long long m, int dtype, long long rows, size_t cap);
// Slices of a chunk of `rows` rows: a channel has at most steps = ceil(rows / channels) rows in the chunk, and these steps are cut into
//     slices = max(1, min(kLxspecTargetItems / (channels * ceil(N1 / 2)), steps / kLxspecMinSteps))
// contiguous ranges, the first steps % slices of them one step longer.  0 for refused sizes.
long long lxspec_slices(long long m, long long channels, long long rows);
// Scratch of the fused route: chunk rows * 2 * (m/2) complex, plus the partial sums [slices of the first chunk][channels][m/2 + 1].
size_t lxspec_scratch_bytes(long long m, int dtype, long long channels, long long rows, size_t cap);
// The fused route of L on `scratch` (lxspec_scratch_bytes bytes, aliasing none of x, g, out): per chunk of rows pass A on both fields
// (one for the auto-spectrum), the accumulating Mid kernel into the partial sums, and the reduction over the slices that writes (first
// chunk) or adds to (later chunks) `out` in the requested order.  A call of one chunk and one slice in order 1 stores straight to out.
// Sums rows of a slice in order, slices in order, chunks in order: no atomics.  Enqueues on `stream` only.
int lxspec_run(const LxspecLaunch& L, size_t cap, void* scratch, size_t scratch_bytes, hipStream_t stream);

// The accumulation of the composed route behind the real transforms of length m (dfft_batch.cpp runs those, behind pad_rows of
// dfft_rows_common.h): out[c][.] (+)= the sum over the chunk's rows of channel c, in row order, of conj(xb) gb (row r of the chunk is row row0 + r of
// the call; row0 == 0 starts the sum; gb == xb: the auto-spectrum), bins [nr][m/2 + 1] in natural order, out in `order`.
int lxspec_mac(const void* xb, const void* gb, void* out, long long m, long long row0, long long nr, long long channels, int dtype, int order,
               hipStream_t stream);

}  // namespace dfft
