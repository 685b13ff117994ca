// dfft_xspec.h -- host-side interface of the batched 1-D real cross-spectrum (dfft_xspec.hip): the rows of two real fields
// [batch][channels][n], zero-padded to m, reduced over the batch to S[c][k] = sum_b conj(rfft(x[b, c], m)[k]) rfft(g[b, c], m)[k].
// Internal header (the C-ABI is include/dfft.h: dfft_rxspec1d).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

namespace dfft {

// Row (b, c) of either field holds n contiguous reals at ((b * channels) + c) * n.  g == x (exactly) is the auto-spectrum; out
// [channels][m/2 + 1] complex overlaps neither field, and neither field is ever written.
struct RxspecLaunch {
    int         dtype;  // DType: F64 = double, F32 = float
    long long   n, m, channels, batch;
    const void* x;
    const void* g;
    void*       out;
};

// DFFT_RXSPEC_FUSED, read per call: "0" sends every length to the composed route.
bool rxspec_fused_env();
// n even and both fields aligned to two reals: the fused kernel loads two reals as one value
bool rxspec_vec(const void* x, const void* g, long long n, int dtype);
// The fused kernel: m/2 has a tuned single-pass plan (dfft_plans.h) whose instantiations for `dtype` keep nothing in scratch memory
// and were not measured slower than the composed route (rxspec_fused_ok).  The rule depends on neither n nor `vec`.
bool rxspec_fused(long long n, long long m, int dtype, bool vec);
// Slices the batch is cut into (contiguous ranges, the first batch % slices of them one row longer): fixed constants only -- about as
// many (channel, slice) items as a 256-CU part holds thread groups, at least kRxspecMinRows rows per slice.  0 for refused sizes.
long long rxspec_slices(long long m, long long channels, long long batch, int dtype);
// Scratch bytes rxspec needs.  Fused: the partial sums [slices][channels][m/2 + 1] (0 for one slice).  Composed: the padded rows and
// the bins of both fields for one chunk of rows of at most max(256 MiB, one row's).
size_t rxspec_scratch_bytes(const RxspecLaunch& L, bool fused_on, size_t cap);
// The cross-spectrum of L: the fused kernel (and, for more than one slice, the kernel that sums the slices in order), or -- per chunk
// of rows -- pad kernel on both fields, R2C rows (launch_real_rows) on both, and a kernel that adds each channel's rows to `out` in row
// order.  `scratch` holds scratch_bytes >= rxspec_scratch_bytes(L) bytes (composed: at least one row's) and aliases none of x, g, out.
// Enqueues on `stream` only; allocates nothing (twiddle tables are cached per device).  DFFT_OK or DFFT_E*.
int rxspec(const RxspecLaunch& L, bool fused_on, size_t cap, void* scratch, size_t scratch_bytes, hipStream_t stream);

}  // namespace dfft
