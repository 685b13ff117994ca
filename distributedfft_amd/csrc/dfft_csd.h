// dfft_csd.h -- host-side interface of the framed (Welch) 1-D real cross-spectrum (dfft_csd.hip): rows of two real fields [rows][n] cut
// into whole frames of m reals that advance by `hop`, windowed, transformed and reduced over the frames of a row to
//     out[r][k] = scale sum_f conj(rfft(win x[r, f hop : f hop + m])[k]) rfft(win g[r, f hop : f hop + m])[k],   k = 0 ... m/2.
// Internal header (the C-ABI is include/dfft.h: dfft_rcsd1d).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

namespace dfft {

// Row r of either field holds n contiguous reals at r * n; frame f of it is the samples [f hop, f hop + m): no padding, no centring,
// frames = stft_frames(n, m, hop, 0) >= 1, and the samples behind the last whole frame (and, for hop > m, between frames) are never
// read.  g == x (exactly) is the auto-spectrum; out [rows][m/2 + 1] complex overlaps neither field nor the window, and neither field nor
// the window is ever written.
struct RcsdLaunch {
    int         dtype;  // DType: F64 = double, F32 = float
    long long   n, m, hop, frames, rows;
    double      scale;
    const void* x;
    const void* g;
    void*       out;
    const void* win;
};

// The size rule that the entry points (dfft_csd_api.cpp) and the dispatcher (dfft_csd.hip) share: rows and frames below 2^31 each
// (rows * slices stays below 2^31 with them: several slices mean at most 16384 items)
inline bool rcsd_items_ok(long long rows, long long frames) { return rows < (1ll << 31) && frames < (1ll << 31); }
// DFFT_RCSD_FUSED, read per call: "0" sends every length to the composed route.
bool rcsd_fused_env();
// n and hop even and both fields aligned to two reals: the fused kernel loads two reals as one value
bool rcsd_vec(const void* x, const void* g, long long n, long long hop, int dtype);
// The fused kernel: m/2 has a tuned single-pass plan (dfft_plans.h) whose instantiations for `dtype` keep nothing in scratch memory
// (rcsd_fused_ok), for the auto-spectrum kernel (autos: g == x) or the cross kernel, which needs more registers.  Measured against the
// composed route at m = 256, 1024, 2048 and 8192: kept where it is faster by more than the spreads, which sent fp32
// m = 2048 cross to the composed route; every other length is kept on the resource inventory alone.  Depends on m, dtype and autos only.
bool rcsd_fused(long long m, int dtype, bool autos);
// Slices the frames of a row are cut into (contiguous ranges, the first frames % slices of them one frame longer): fixed constants
// only -- about as many (row, slice) items as a 256-CU part holds thread groups, at least kRcsdMinFrames frames per slice.  0 for
// refused sizes.
long long rcsd_slices(long long m, long long rows, long long frames, int dtype);
// Scratch bytes rcsd needs.  Fused: the partial sums [slices][rows][m/2 + 1] (0 for one slice).  Composed: the windowed frames and the
// bins of both fields for one chunk of frames of at most max(cap, one frame's), cap = 256 MiB (or DFFT_RCSD_CHUNK_BYTES, read per
// call: the tests' way to make several chunks of a small problem).
size_t rcsd_scratch_bytes(const RcsdLaunch& L, bool fused_on);
// The framed cross-spectrum of L: the fused kernel (and, for more than one slice, the kernel that sums the slices in order), or -- per
// chunk of frames -- gather-and-window kernel and R2C rows (launch_real_rows) on both fields, and a kernel that adds the chunk's frames of
// each row to `out` in frame order.  `scratch` holds scratch_bytes >= rcsd_scratch_bytes(L) bytes (composed: at least one frame's) and
// aliases none of x, g, win, out.  Enqueues on `stream` only; allocates nothing (twiddle tables are cached per device).  DFFT_OK or DFFT_E*.
int rcsd(const RcsdLaunch& L, bool fused_on, void* scratch, size_t scratch_bytes, hipStream_t stream);

}  // namespace dfft
