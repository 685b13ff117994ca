// dfft_conv.h -- the X stage of the spectral-filter (FFT convolution) plans, dfft_plan_create_conv (dfft_conv.hip): forward transform
// along X, multiply by the plan's filter copy, inverse transform along X -- on the slab [x][row][z] the two YZ stages hand over.
// Internal header (the C-ABI is include/dfft.h).
#pragma once
#include <hip/hip_runtime.h>

namespace dfft {

// The slab the X stage works on and the filter copy share ONE physical layout: element (x, r, z) lies at
//     x * plane + r * pitch + (rot ? (z + rot * x) & (ncols - 1) : z)                                      (units of one complex element)
// P = 1 with the padded hand-over buffer: plane / pitch are its padded strides; P = 1 without: N1 * N2 / N2; P > 1: the received slab
// [x][yl][N2] with its rows rotated by rot * x where the C2C plan rotates them (RotMap, dfft_kernels.h; ncols is a power of two then).
struct ConvLaunch {
    int         dtype;        // DType
    int         n0;           // transform length
    int         filter_real;  // the filter copy holds reals (half the bytes) instead of complex elements
    int         forward_only; // store the forward transform times `scale` instead (dfft_conv_set_kernel: `out` is the filter copy)
    const void* in;
    void*       out;          // == in: in place; else a buffer of the same layout
    const void* filt;
    const void* tw;           // n0-entry twiddle table of the dtype
    long long   plane, pitch;
    long long   rows, ncols;
    int         rot;          // elements per plane, 0 = plain rows
    double      scale;        // forward_only only (a filter copy has the scale folded in)
};

// lengths with a fused kernel (xconv_cols_kernel): 64, 128, 256, 384, 512, 768, 1024
bool conv_fused_length(int n0);
// whether launch_conv_fused serves the launch: a fused length, and for fp32 column PAIRS (even ncols, plane, pitch and rot)
bool conv_fused_applies(const ConvLaunch& L);
hipError_t launch_conv_fused(const ConvLaunch& L, hipStream_t stream);
// multi route: data[i] *= filt[i] over `count` elements of the shared layout (padding included), 16-byte accesses
hipError_t launch_conv_mul(int dtype, int filter_real, void* data, const void* filt, long long count, hipStream_t stream);
// filter re-layout (dfft_conv_set_filter): dst[layout(kx, r, z)] = scale * h[(r * ncols + z) * n0 + kx]; h and dst complex or real
hipError_t launch_conv_relayout(const ConvLaunch& L, const void* h, void* dst, hipStream_t stream);

}  // namespace dfft
