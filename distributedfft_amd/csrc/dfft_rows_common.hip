// dfft_rows_common.hip -- the element-wise kernels that the composed forms of the 1-D real kernel families share: zero-padded rows
// (rconv, rxspec and their long forms), truncated rows (rconv and its long form) and the slice reduction of the fused cross-spectrum
// kernels (rxspec, rcsd).  One kernel template and one host launcher each; compiled once.  Kernels whose indexing differs from family
// to family (the filter multiplies, the gathers and scatters, the accumulating kernels, the permuting reduction of the long
// cross-spectrum) stay in their units.
#include "dfft_fused_host.h"
#include "dfft_rows_common.h"

namespace dfft {

// padded rows: p[r][i] = x[r][i] (i < n), 0 (n <= i < m)
template <class RT>
__global__ void __launch_bounds__(256) pad_rows_kernel(const RT* __restrict__ in, RT* __restrict__ p, long long n, long long m, long long total) {
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
        const long long r = e / m, i = e - r * m;
        p[e] = i < n ? in[r * n + i] : (RT)0;
    }
}
// y[r][i] = p[r][i], i < n.  `out` may be the buffer the chunk was padded from: p is the scratch.
template <class RT>
__global__ void __launch_bounds__(256) trunc_rows_kernel(const RT* __restrict__ p, RT* __restrict__ out, long long n, long long m, long long total) {
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
        const long long r = e / n, i = e - r * n;
        out[e] = p[r * m + i];
    }
}
// out[e] = partial[0][e] + partial[1][e] + ... in slice order, e < count
template <class V>
__global__ void __launch_bounds__(256) slice_reduce_kernel(const V* __restrict__ partial, V* __restrict__ out, long long count, unsigned slices) {
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < count; e += (long long)gridDim.x * 256) {
        V acc = partial[e];
        for (unsigned s = 1; s < slices; ++s) {
            const V p = partial[(long long)s * count + e];
            acc.x += p.x;
            acc.y += p.y;
        }
        out[e] = acc;
    }
}

int pad_rows(const void* in, void* pad, long long n, long long m, long long nr, int dtype, hipStream_t stream) {
    (void)hipGetLastError();
    if (dtype == F64) hipLaunchKernelGGL(pad_rows_kernel<double>, dim3(elementwise_grid(nr * m)), dim3(256), 0, stream, (const double*)in, (double*)pad, n, m, nr * m);
    else hipLaunchKernelGGL(pad_rows_kernel<float>, dim3(elementwise_grid(nr * m)), dim3(256), 0, stream, (const float*)in, (float*)pad, n, m, nr * m);
    DFFT_HIP_TRY(hipGetLastError());
    return DFFT_OK;
}

int trunc_rows(const void* pad, void* out, long long n, long long m, long long nr, int dtype, hipStream_t stream) {
    (void)hipGetLastError();
    if (dtype == F64) hipLaunchKernelGGL(trunc_rows_kernel<double>, dim3(elementwise_grid(nr * n)), dim3(256), 0, stream, (const double*)pad, (double*)out, n, m, nr * n);
    else hipLaunchKernelGGL(trunc_rows_kernel<float>, dim3(elementwise_grid(nr * n)), dim3(256), 0, stream, (const float*)pad, (float*)out, n, m, nr * n);
    DFFT_HIP_TRY(hipGetLastError());
    return DFFT_OK;
}

int slice_reduce(const void* partial, void* out, long long count, long long slices, int dtype, hipStream_t stream) {
    (void)hipGetLastError();
    if (dtype == F64)
        hipLaunchKernelGGL(slice_reduce_kernel<double2>, dim3(elementwise_grid(count)), dim3(256), 0, stream, (const double2*)partial, (double2*)out, count,
                           (unsigned)slices);
    else
        hipLaunchKernelGGL(slice_reduce_kernel<float2>, dim3(elementwise_grid(count)), dim3(256), 0, stream, (const float2*)partial, (float2*)out, count,
                           (unsigned)slices);
    DFFT_HIP_TRY(hipGetLastError());
    return DFFT_OK;
}

}  // namespace dfft
