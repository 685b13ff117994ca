// dfft_real.h -- host-side launch descriptor of the real-row kernels (dfft_real.hip): the Z stage of the real-to-complex /
// complex-to-real slab plans.  Internal header (the C-ABI is include/dfft.h).
#pragma once
#include <hip/hip_runtime.h>

namespace dfft {

// `rows` rows of the real axis (length n2, even), tiled like the plan's row launches: row r = (plane a, row b) with
// a = r / rows_per_plane, b = r % rows_per_plane.
//   dir = +1 (R2C): real row  in  + a * rplane + b * rpitch (n2 reals)  ->  complex row out + a * cplane + b * cpitch (n2/2 + 1 bins)
//   dir = -1 (C2R): complex row in + a * cplane + b * cpitch (n2/2 + 1 bins, imaginary parts of bins 0 and n2/2 ignored)
//                   -> real row out + a * rplane + b * rpitch (n2 reals)
// Both unnormalised; results are multiplied by `scale` on their way out.  Real-side strides count reals and must be even (a real row is
// read / written as n2/2 complex values), complex-side strides count complex elements.
struct RealLaunch {
    int         dtype;  // DType: F64 = double reals / double2 bins, F32 = float / float2
    int         n2;
    int         dir;
    const void* in;
    void*       out;
    long long   rows, rows_per_plane;
    long long   rpitch, rplane;
    long long   cpitch, cplane;
    double      scale;
};

// n2 even and n2/2 an FFT length of the single-pass range (fft_length_supported, at most 4096)
bool real_length_supported(long long n2);
// One launch of the fused row kernel where n2/2 has a tuned plan (dfft_plans.h); otherwise the row kernel of the run-time-scheduled
// length n2/2 plus a split (R2C, after it) or merge (C2R, before it) kernel.  The two-launch C2R form merges IN PLACE on `in`.
// hipErrorInvalidValue for an unsupported length.
hipError_t launch_real_rows(const RealLaunch& L, hipStream_t stream);

}  // namespace dfft
