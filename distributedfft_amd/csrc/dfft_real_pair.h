// dfft_real_pair.h -- host-side interface of the two-for-one real transforms (dfft_real_pair.hip): rows of n reals <-> rows of n/2 + 1
// Hermitian bins for every n that has an n-point complex transform (single-pass, four-step or Bluestein), odd n included.  Internal header
// (the C-ABI is include/dfft.h: dfft_real_form, dfft_rfft1d, dfft_plan_create_r2c_any).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

#include "dfft_bluestein.h"

namespace dfft {

// `rows` real rows of length n, tiled like RealLaunch (dfft_real.h): row r = (plane a, row b), a = r / rows_per_plane,
// b = r % rows_per_plane.
//   dir = +1 (R2C): reals in + a * rplane + b * rpitch (n reals) -> bins out + a * cplane + b * cpitch (n/2 + 1 bins)
//   dir = -1 (C2R): bins in (imaginary parts of bin 0 and, n even, bin n/2 ignored) -> reals out; n * numpy.fft.irfft(row, n)
// Unnormalised.  Rows 2p and 2p + 1 share one n-point complex transform (z = a + i b); an odd last row is paired with a zero row
// (forward) or its partner's output is dropped (backward).  Real-side strides count reals, complex-side strides complex elements.
struct RealPairLaunch {
    int         dtype;  // DType: F64 = double reals / double2 bins, F32 = float / float2
    long long   n;
    int         dir;
    const void* in;
    void*       out;
    long long   rows, rows_per_plane;
    long long   rpitch, rplane;
    long long   cpitch, cplane;
};

// one launch of r2c_pair_rows_kernel / c2r_pair_rows_kernel: n odd with a tuned single-pass plan (dfft_plans.h)
bool real_pair_fused(long long n);
// Scratch bytes real_pair_rows needs for `rows` rows: 0 for the fused form, else the packed pairs of one batch chunk (at most
// max(256 MiB, one pair's)) plus the scratch of the n-point transform on that chunk (four-step: as much again; Bluestein:
// bluestein_scratch_bytes).  `T`: the Bluestein tables of (n, dtype, dir) when n is a Bluestein length, else nullptr.
size_t real_pair_scratch_bytes(long long n, int dtype, long long rows, const BluesteinTables* T, bool bluestein_fused, size_t cap);
// The rows of L: the fused kernel, or -- per batch chunk -- pack, the n-point complex transform (single-pass, long_fft or bluestein_fft
// with T), split (R2C); merge, inverse transform, unpack (C2R).  `scratch` holds scratch_bytes >= real_pair_scratch_bytes(n, dtype, 2, T,
// fused) bytes and does not alias in / out; `in` is never written.  Enqueues on `stream` only; allocates nothing.  DFFT_OK or DFFT_E*.
int real_pair_rows(const RealPairLaunch& L, const BluesteinTables* T, bool bluestein_fused, size_t cap, void* scratch, size_t scratch_bytes,
                   hipStream_t stream);

}  // namespace dfft
