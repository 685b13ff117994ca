// dfft_bluestein.h -- any-length transforms by Bluestein's chirp-z algorithm (dfft_bluestein.hip): the lengths neither the single-pass
// kernels (7-smooth, <= 4096) nor the four-step form (products of two tuned lengths, <= 2^24) serve, up to 2^23.  Internal header (the
// C-ABI is include/dfft.h: dfft_length_kind, dfft_bluestein_length, dfft_fft1d_any, DFFT_PLAN_ANY_LENGTH).
#pragma once
#include <hip/hip_runtime.h>

#include <memory>

namespace dfft {

constexpr long long kBluesteinMaxLength = 1ll << 23;
constexpr long long kBluesteinFusedMaxLength = 2048;

// Padded length M of a Bluestein transform of length n (1 <= n <= 2^23; the caller decides that n is a Bluestein length): 1 for n = 1,
// the smallest tuned single-pass length >= 2n - 1 for n <= 2048 (dfft_plans.h; at most 4096), else the smallest length >= 2n - 1 that
// long_split accepts (at most 2^24).  0 outside that range.
long long bluestein_padded_length(long long n);

// Device tables of one (device, n, dtype, direction): the chirp c_m = exp(-d i pi (m^2 mod 2n) / n), m < n, and
// B^ = FFT_M(b) / M with b_m = conj(c_|m|) for |m| < n (wrapped mod M), 0 elsewhere -- computed in fp64 with the library's own forward
// FFT and rounded once for fp32.  Owned through shared_ptr: a plan keeps the tables of its axes alive across dfft_trim.
struct BluesteinTables {
    int       dev = 0, dtype = 0, dir = 0;
    long long n = 0, M = 0;
    void*     chirp = nullptr;  // n elements of the dtype's complex type
    void*     bhat = nullptr;   // M elements
    ~BluesteinTables();
};
typedef std::shared_ptr<const BluesteinTables> BluesteinTablesPtr;

// The cached tables of (current device, n, dtype, dir), built on first use (allocates and synchronises: call it at plan creation or
// at the top of a plan-less call, never inside dfft_execute).  DFFT_OK, or a DFFT_E* code with dfft_last_error set.
int bluestein_tables(long long n, int dtype, int dir, BluesteinTablesPtr* out);
// Drops the cache's references (dfft_trim); tables a plan still holds live on until the plan is destroyed.
void bluestein_trim();

// DFFT_BLUESTEIN_FUSED (default 1): 0 forces the multi-pass form for n <= 2048 (A/B and measurement switch; same M, same tables)
bool bluestein_fused_env();
// Whether bluestein_fft runs [batch][n][s] as one launch (`fused`: the caller's DFFT_BLUESTEIN_FUSED reading): n <= 2048 and, for s > 1,
// n * s < 2^31; otherwise the multi-pass form in batch chunks.
bool bluestein_runs_fused(long long n, long long s, bool fused);
// Scratch bytes a call of bluestein_fft on [batch][n][s] needs (0 for the fused form); batch chunks keep it at most
// max(256 MiB, what one transform needs).
size_t bluestein_scratch_bytes(const BluesteinTables& T, long long s, long long batch, bool fused, size_t cap);
// Length-n transforms along the middle axis of data[batch][n][s], unnormalised, times `scale` (0 = 1).  in == out is allowed.
// `scratch` holds scratch_bytes >= bluestein_scratch_bytes(T, s, 1, fused) bytes (the batch is run in chunks that fit it) and does not
// alias in / out.  Enqueues on `stream` only; allocates nothing.
int bluestein_fft(const BluesteinTables& T, const void* in, void* out, long long s, long long batch, double scale, bool fused,
                  void* scratch, size_t scratch_bytes, hipStream_t stream);

}  // namespace dfft
