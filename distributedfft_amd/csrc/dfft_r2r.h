// dfft_r2r.h -- host-side interface of the real-to-real transforms (dfft_r2r.hip): DCT / DST of types II and III along the middle axis
// of reals [batch][n][s], for every n that has an n-point complex transform.  Types I and IV are not built.  Internal header (the C-ABI
// is include/dfft.h: dfft_r2r1d_strided).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <memory>

#include "dfft_bluestein.h"

namespace dfft {

// kinds, as DFFT_R2R_* of include/dfft.h.  Unnormalised (scipy.fft norm=None, FFTW's REDFT10 / REDFT01 / RODFT10 / RODFT01):
//   DCT2: y[k] = 2 sum_j x[j] cos(pi k (2j + 1) / 2n)            DCT3: y[j] = x[0] + 2 sum_{k >= 1} x[k] cos(pi k (2j + 1) / 2n)
//   DST2: y[k] = 2 sum_j x[j] sin(pi (k + 1) (2j + 1) / 2n)      DST3: y[j] = (-1)^j x[n-1] + 2 sum_{k < n-1} x[k] sin(pi (k + 1) (2j + 1) / 2n)
enum { R2R_DCT2 = 0, R2R_DCT3 = 1, R2R_DST2 = 2, R2R_DST3 = 3 };

// Two real sequences share one n-point complex transform: columns 2c and 2c + 1 (s > 1) or rows 2p and 2p + 1 (s = 1); an odd last one
// is paired with zeros.  `out` == `in` (exactly) is allowed; otherwise the two do not overlap and `in` is never written.
struct R2rLaunch {
    int         dtype;  // DType: F64 = double, F32 = float
    int         kind;   // R2R_*
    long long   n, s, batch;
    const void* in;
    void*       out;
};

// The quarter-wave table w_k = exp(-i pi k / 2n), k < n, of one (device, n, dtype): computed in double on the host, rounded once.
struct R2rTable {
    int       dev = 0;
    long long n = 0;
    int       dtype = 0;
    void*     w = nullptr;
    ~R2rTable();
};
typedef std::shared_ptr<const R2rTable> R2rTablePtr;
// The cached table of (current device, n, dtype); built (one hipMalloc and one blocking copy) on first use.
int r2r_table(long long n, int dtype, R2rTablePtr* out);
// Drops the cache (dfft_trim): every owning device is drained first, as for the Bluestein tables.
void r2r_trim();

// DFFT_R2R_FUSED, read per call: "0" sends every length to the composed route.
bool r2r_fused_env();
// s even and both buffers aligned to two reals: the fused column kernels and the pre / post kernels move a column pair as one value
bool r2r_vec(const void* in, const void* out, long long s, int dtype);
// One launch of the fused kernels: n has a tuned single-pass plan (dfft_plans.h) whose instantiation for (dtype, type II / III, form:
// rows at s = 1, else column pairs as one value (vec) or as two reals) keeps nothing in scratch memory, and, for s >= 2, a batch
// item's points fit 32-bit offsets (n * s < 2^31).
bool r2r_fused(long long n, long long s, int dtype, int kind, bool vec);
// Scratch bytes r2r needs: 0 for the fused forms, else the packed pairs of one batch chunk (at most max(256 MiB, one item's or pair's))
// plus the scratch of the n-point transform on that chunk (four-step: as much again; Bluestein: bluestein_scratch_bytes).
// `T`: the Bluestein tables of (n, dtype, +1 for type II / -1 for type III) when n is a Bluestein length, else nullptr.
size_t r2r_scratch_bytes(const R2rLaunch& L, bool fused_on, const BluesteinTables* T, bool bluestein_fused, size_t cap);
// The transform of L: the fused kernel, or -- per batch chunk -- pre kernel (permute or pre-twiddle, pack pairs into scratch), the n-point
// complex transform on the scratch (the C2C row / column launch, long_fft or bluestein_fft with T), post kernel into `out`.  `scratch`
// holds scratch_bytes >= r2r_scratch_bytes(L with batch 1, ...) bytes and aliases neither in nor out.  Enqueues on `stream` only; allocates
// nothing.  DFFT_OK or DFFT_E*.
int r2r(const R2rLaunch& L, const R2rTable& W, bool fused_on, const BluesteinTables* T, bool bluestein_fused, size_t cap, void* scratch, size_t scratch_bytes,
        hipStream_t stream);

}  // namespace dfft
