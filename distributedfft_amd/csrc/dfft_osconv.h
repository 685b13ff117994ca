// dfft_osconv.h -- host-side interface of the overlap-save 1-D real FFT convolution (dfft_osconv.hip): rows of reals [batch][channels][n]
// of any length filtered block by block, m reals per block of which the first `discard` results are dropped.  Internal header (the
// C-ABI is include/dfft.h: dfft_rconv1d_os).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

namespace dfft {

// With S = m - discard and nb = ceil(n_out / S), block b of row r is
//     xb[i] = in[r][b S - discard + i] (0 where that index is outside [0, n)),  cb = irfft(rfft(xb, m) * h[r % channels], m),
//     out[r][b S + j] = cb[discard + j]   (0 <= j < S, b S + j < n_out).
// in [batch * channels][n] and out [batch * channels][n_out] do not overlap (blocks read what their neighbours write); h
// [channels][m/2 + 1] overlaps neither; in and h are never written.
struct OsconvLaunch {
    int         dtype;        // DType: F64 = double, F32 = float
    int         filter_kind;  // RCONV_FILTER_* of dfft_rconv.h
    long long   n, n_out, m, discard, channels, batch;
    const void* in;
    void*       out;
    const void* h;
};

// Blocks per row, ceil(n_out / (m - discard)); 0 for sizes outside 1 <= n_out, 0 <= discard < m
long long osconv_blocks(long long n_out, long long m, long long discard);
// n, n_out and discard even and both buffers aligned to two reals: the fused kernel moves two reals as one value
bool osconv_vec(const void* in, const void* out, long long n, long long n_out, long long discard, int dtype);
// One launch of the fused kernel: the rule of rconv_fused (m/2 tuned, rconv_fused_ok) less the (m/2, dtype) whose block kernels would
// keep values in scratch memory (osconv_fused_ok).  Depends on m and dtype only.
bool osconv_fused(long long m, int dtype);
// Scratch bytes osconv needs: 0 for the fused kernel, else the gathered blocks and the bins of one chunk of items (an item is one
// block of one row) of at most max(256 MiB, one item's).
size_t osconv_scratch_bytes(const OsconvLaunch& L, bool fused_on, size_t cap);
// The convolution of L: the fused kernel, or -- per chunk of items -- gather kernel, R2C rows (launch_real_rows), multiply kernel (H / m,
// in place on the bins), C2R rows, scatter kernel into `out`.  `scratch` holds scratch_bytes >= one item's bytes and aliases none of
// in, out, h.  Enqueues on `stream` only; allocates nothing (the twiddle tables of m/2 and m are cached per device).  DFFT_OK or DFFT_E*.
int osconv(const OsconvLaunch& L, bool fused_on, size_t cap, void* scratch, size_t scratch_bytes, hipStream_t stream);
// The block for `taps` taps and n_out results per row: discard = taps - 1 rounded up to even, and the accepted m > discard with the
// smallest ceil(n_out / (m - discard)) * t(m) over the table of per-block times in dfft_osconv.hip; one block where one fits.
// false: taps outside [1, 8191], n_out < 1 or a bad dtype.
bool osconv_block(long long taps, long long n_out, int dtype, long long* m, long long* discard);

}  // namespace dfft
