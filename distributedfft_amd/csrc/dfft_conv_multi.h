// dfft_conv_multi.h -- the K-output X stage of the multi-output real-field spectral-filter plans, dfft_plan_create_conv_real_multi
// (dfft_conv_multi.hip): forward transform along X once, multiply by the plan's one filter copy once, then per output k the separable
// factors a_k[x] . b_k[row] . c_k[col] and the inverse transform along X into slab k.  Internal header (the C-ABI is include/dfft.h).
#pragma once
#include <hip/hip_runtime.h>

#include "dfft_conv.h"

namespace dfft {

constexpr int CONV_MAX_OUTPUTS = 8;  // DFFT_CONV_MAX_OUTPUTS of include/dfft.h

// The K slabs and the factor tables, passed to the kernels BY VALUE (one kernel argument; no table of pointers in memory).
// Every slab has the layout of ConvLaunch (plain rows: real-field plans never rotate); out[0] may be the input slab.
// ax[k]: N0 complex elements of the dtype; by[k]: `rows` elements (the plan's own part of the caller's vector, from y0);
// cz[k]: `ncols` elements, zeros behind N2/2 + 1, on a 16-byte boundary (fp32 reads it as column pairs).  Never NULL: a factor nobody
// set points at a table of ones.
struct ConvMultiArgs {
    void*       out[CONV_MAX_OUTPUTS];
    const void* ax[CONV_MAX_OUTPUTS];
    const void* by[CONV_MAX_OUTPUTS];
    const void* cz[CONV_MAX_OUTPUTS];
};

// Fused form (xconv_multi_cols_kernel; the fused lengths and tile geometry of dfft_conv.hip): reads L.in and L.filt, writes M.out[0 .. K).
// L.out and L.rot are not used (rot must be 0).  Whether it applies: conv_fused_applies(L).
hipError_t launch_conv_multi_fused(const ConvLaunch& L, const ConvMultiArgs& M, int K, hipStream_t stream);
// Multi route, output k: dst[i] = src[i] . ax[x] . by[row] . cz[col] over the whole slab of L's layout (16-byte accesses; columns
// ncols .. pitch - 1 receive zeros); dst == src is allowed.
hipError_t launch_conv_factor_mul(const ConvLaunch& L, const void* src, void* dst, const void* ax, const void* by, const void* cz,
                                  hipStream_t stream);

}  // namespace dfft
