// dfft_real_cols.h -- host-side interface of the real transforms along a strided axis (dfft_real_cols.hip): the middle axis of
// [batch][n][s] reals <-> [batch][n/2 + 1][s] Hermitian bins, for every n that has an n-point complex transform.  Internal header (the
// C-ABI is include/dfft.h: dfft_rfft1d_strided, dfft_rfft2d_batch).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

#include "dfft_bluestein.h"

namespace dfft {

//   dir = +1 (R2C): reals in [batch][n][s] -> bins out [batch][n/2 + 1][s]   (numpy.fft.rfft(x, axis=1))
//   dir = -1 (C2R): bins in -> reals out, n * numpy.fft.irfft(X, n, axis=1) for any input (imaginary parts of bin 0 and, n even, bin n/2
//                   ignored)
// Unnormalised.  Real columns 2c and 2c + 1 share one n-point complex transform (z = a + i b); an odd last column is paired with a zero
// column (forward) or its partner's output is dropped (backward).  `in` and `out` are element-aligned and do not overlap.
struct RealColsLaunch {
    int         dtype;  // DType: F64 = double reals / double2 bins, F32 = float / float2
    long long   n, s, batch;
    int         dir;
    const void* in;
    void*       out;
};

// One launch of r2c_pair_cols_kernel / c2r_pair_cols_kernel: n has a tuned single-pass plan (dfft_plans.h) (no fused instantiation
// keeps anything in scratch memory), a batch item's points fit 32-bit offsets (n * s < 2^31), and the multi-pass form did not measure
// faster for (n, s, dtype) (dfft_real_cols.hip, multi_pass_faster).
bool real_cols_fused(long long n, long long s, int dtype);
// Scratch bytes real_cols needs: 0 for the fused form, else the packed column pairs of one batch chunk (at most max(256 MiB, one batch
// item's)) plus the scratch of the n-point transform on that chunk (four-step: as much again; Bluestein: bluestein_scratch_bytes).
// `T`: the Bluestein tables of (n, dtype, dir) when n is a Bluestein length, else nullptr.
size_t real_cols_scratch_bytes(long long n, long long s, long long batch, int dtype, const BluesteinTables* T, bool bluestein_fused, size_t cap);
// The transform of L: the fused kernel, or -- per batch chunk -- pack (skipped where s is even and `in` is aligned to a complex element),
// the n-point complex transform down the column pairs (the C2C column launch, long_fft or bluestein_fft with T), split (R2C); merge,
// inverse transform, unpack (C2R; the transform stores straight into `out` where s is even and `out` is aligned).  `scratch` holds
// scratch_bytes >= real_cols_scratch_bytes(n, s, 1, dtype, T, bluestein_fused) bytes and does not alias in / out; `in` is never
// written.  Enqueues on `stream` only; allocates nothing.  DFFT_OK or DFFT_E*.
int real_cols(const RealColsLaunch& L, const BluesteinTables* T, bool bluestein_fused, size_t cap, void* scratch, size_t scratch_bytes,
              hipStream_t stream);

}  // namespace dfft
