// dfft_rows_common.h -- the element-wise kernels that the composed forms of the 1-D real kernel families share (dfft_rows_common.hip):
// zero-padded rows, truncated rows and the slice reduction.  Internal header.
#pragma once
#include <hip/hip_runtime.h>

namespace dfft {

// `nr` zero-padded rows: pad[r][i] = in[r][i] (i < n), 0 (n <= i < m).  dtype: the precision of the reals.
int pad_rows(const void* in, void* pad, long long n, long long m, long long nr, int dtype, hipStream_t stream);
// out[r][i] = pad[r][i], i < n.  `out` may be the buffer the rows were padded from.
int trunc_rows(const void* pad, void* out, long long n, long long m, long long nr, int dtype, hipStream_t stream);
// out[e] = partial[0][e] + partial[1][e] + ... in slice order, e < count complex values of precision dtype
int slice_reduce(const void* partial, void* out, long long count, long long slices, int dtype, hipStream_t stream);

}  // namespace dfft
