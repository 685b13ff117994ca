// dfft_rconv.h -- host-side interface of the batched 1-D real FFT convolution (dfft_rconv.hip): every row of reals [batch][channels][n]
// filtered by its channel's spectrum, y = irfft(rfft(x, m) * H, m)[:n].  Internal header (the C-ABI is include/dfft.h: dfft_rconv1d).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

namespace dfft {

// filter kinds, as DFFT_FILTER_* of include/dfft.h
enum { RCONV_FILTER_COMPLEX = 0, RCONV_FILTER_REAL = 1 };

// Row r of the batch * channels rows of n reals (contiguous) uses filter row r % channels of h [channels][m/2 + 1].  `out` == `in`
// (exactly) is allowed; otherwise the two do not overlap and `in` is never written.  h overlaps neither and is never written.
struct RconvLaunch {
    int         dtype;        // DType: F64 = double, F32 = float
    int         filter_kind;  // RCONV_FILTER_*: elements of the complex type, or of the real type
    long long   n, m, channels, batch;
    const void* in;
    void*       out;
    const void* h;
};

// Smallest m >= at_least that the convolution accepts (m even, m/2 a single-pass length: real form 1, so m <= 8192); 0 if none.
long long rconv_length(long long at_least);
// DFFT_RCONV_FUSED, read per call: "0" sends every length to the composed route.
bool rconv_fused_env();
// n even and both buffers aligned to two reals: the fused kernel and the pad / truncate kernels move two reals as one value
bool rconv_vec(const void* in, const void* out, long long n, int dtype);
// One launch of the fused kernel: m/2 has a tuned single-pass plan (dfft_plans.h) whose instantiations for `dtype` keep nothing in
// scratch memory (rconv_fused_ok) and were not measured slower than the composed route.  The rule does not depend on the filter kind or
// on `vec` (an instantiation that would spill sends all four of its (length, dtype) to the composed route), so the scratch of a call is
// known from its shape alone.
bool rconv_fused(long long n, long long m, int dtype, int filter_kind, bool vec);
// Scratch bytes rconv needs: 0 for the fused kernel, else the padded rows and the bins of one batch chunk of at most
// max(256 MiB, one row's).
size_t rconv_scratch_bytes(const RconvLaunch& L, bool fused_on, size_t cap);
// The convolution of L: the fused kernel, or -- per chunk of rows -- pad kernel, R2C rows (launch_real_rows), multiply kernel (H / m, in
// place on the bins), C2R rows, truncate kernel into `out`.  `scratch` holds scratch_bytes >= rconv_scratch_bytes(L with one row)
// bytes and aliases none of in, out, h.  Enqueues on `stream` only; allocates nothing (the twiddle tables of m/2 and m are cached per
// device).  DFFT_OK or DFFT_E*.
int rconv(const RconvLaunch& L, bool fused_on, size_t cap, void* scratch, size_t scratch_bytes, hipStream_t stream);

}  // namespace dfft
