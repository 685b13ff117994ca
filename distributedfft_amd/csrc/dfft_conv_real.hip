// dfft_conv_real.hip -- device code of the real-field spectral-filter plans (dfft_plan_create_conv_real): y = irfftn( rfftn(x) . H ).
//
// The pipeline is built from what the library has: the R2C / C2R row kernels (dfft_real.hip) on the Z axis, the C2C column kernels on Y,
// and the X stage of dfft_conv.hip -- xconv_cols_kernel in place on the half spectrum, whose guard `col < ncols` serves the ragged last
// tile and whose un-rotated form serves a row length that is no power of two.  What is new is the geometry: the half spectrum is private
// to the plan, so it is Nc = conv_real_width(Nh) columns wide instead of Nh = N2/2 + 1 (dfft_conv_real.h has the rule), and the filter --
// given in the layout a forward R2C plan returns, [y_local][Nh][N0] -- has to be brought into that slab.
//
// Why the pad columns Nh .. Nc - 1 of the spectrum hold zeros at every execute, without a pass that writes them:
//   * the intermediate [x_local][N1][pitch] is cleared once when the plan is created;
//   * the R2C row kernels store bins 0 .. Nh - 1 of a row and nothing else (r2c_rows_kernel: op[kk], kk < M, and op[M]; r2c_split_kernel:
//     z[k], z[m - k], z[m]), the in-place C2R merge likewise;
//   * every later pass treats a column on its own and is linear in it: the Y columns map a zero column to a zero column (in place, or
//     packing into the send buffer / unpacking from the receive buffer -- whose Nc-wide rows are overwritten WHOLE by every exchange, pad
//     columns included, so a pooled receive buffer's old contents never survive), and the X stage multiplies a zero column by the filter
//     copy's zero column (written below).
// Were a pad column ever non-zero it would still not reach the result -- no pass mixes columns and the C2R rows read Nh bins -- but zeros
// keep the arithmetic on them free of NaNs and denormals.
#include "dfft_conv_real.h"
#include "dfft_internal.h"

#include <algorithm>

namespace dfft {

namespace {

template <class E> __device__ __forceinline__ E xr_scaled(E v, double s);
template <> __device__ __forceinline__ double xr_scaled(double v, double s) { return v * s; }
template <> __device__ __forceinline__ float xr_scaled(float v, double s) { return (float)((double)v * s); }
template <> __device__ __forceinline__ double2 xr_scaled(double2 v, double s) { return double2{v.x * s, v.y * s}; }
template <> __device__ __forceinline__ float2 xr_scaled(float2 v, double s) { return float2{(float)((double)v.x * s), (float)((double)v.y * s)}; }

// One workgroup moves a 32 x 32 tile (kx, kz) of row r through LDS: the source is read along kx, the slab written along kz.
// grid = (ceil(n0 / 32), ceil(pitch / 32), rows), block = (32, 8).  Columns kz in [nh, pitch) receive zeros.
template <class E>
__global__ void __launch_bounds__(256) xconv_real_relayout_kernel(const E* __restrict__ h, E* __restrict__ dst, int n0, int nh, int pitch,
                                                                  long long plane, double scale) {
    __shared__ E    tile[32][33];
    const long long r = blockIdx.z;
    const int       kx0 = (int)blockIdx.x * 32, kz0 = (int)blockIdx.y * 32;
    for (int i = (int)threadIdx.y; i < 32; i += 8) {
        const int kz = kz0 + i, kx = kx0 + (int)threadIdx.x;
        E         v{};
        if (kz < nh && kx < n0) v = xr_scaled(h[(r * nh + kz) * (long long)n0 + kx], scale);
        tile[i][threadIdx.x] = v;
    }
    __syncthreads();
    for (int i = (int)threadIdx.y; i < 32; i += 8) {
        const int kx = kx0 + i, kz = kz0 + (int)threadIdx.x;
        if (kx < n0 && kz < pitch) dst[(long long)kx * plane + r * pitch + kz] = tile[threadIdx.x][i];
    }
}

template <class E> hipError_t xr_launch(const ConvLaunch& L, long long nh, const void* h, void* dst, hipStream_t stream) {
    const dim3 grid((unsigned)((L.n0 + 31) / 32), (unsigned)((L.pitch + 31) / 32), (unsigned)L.rows), block(32, 8);
    hipLaunchKernelGGL(xconv_real_relayout_kernel<E>, grid, block, 0, stream, (const E*)h, (E*)dst, L.n0, (int)nh, (int)L.pitch, L.plane, L.scale);
    return hipGetLastError();
}

}  // namespace

long long conv_real_width(long long nh, int dtype) {
    if (nh < 1) return 0;
    const long long line = dtype == F32 ? 16 : 8;
    for (long long g = line; g > 2; g /= 2) {
        const long long w = (nh + g - 1) / g * g;
        if ((w - nh) * 32 <= nh) return w;
    }
    return (nh + 1) / 2 * 2;
}

hipError_t launch_conv_real_relayout(const ConvLaunch& L, long long nh, const void* h, void* dst, hipStream_t stream) {
    if (L.rows < 1 || L.n0 < 1 || nh < 1) return hipSuccess;
    // the slab of a real-field plan: plain rows of `pitch` elements, planes of exactly `rows` rows; the grid's y / z extents are 16-bit
    if (L.rot != 0 || nh > L.ncols || L.ncols > L.pitch || L.plane != L.rows * L.pitch || L.pitch >= (1ll << 20) || L.rows > 65535)
        return hipErrorInvalidValue;
    (void)hipGetLastError();
    if (L.dtype == F64) return L.filter_real ? xr_launch<double>(L, nh, h, dst, stream) : xr_launch<double2>(L, nh, h, dst, stream);
    if (L.dtype == F32) return L.filter_real ? xr_launch<float>(L, nh, h, dst, stream) : xr_launch<float2>(L, nh, h, dst, stream);
    return hipErrorInvalidValue;
}

}  // namespace dfft
