// dfft_conv_real.h -- what the real-field spectral-filter plans (dfft_plan_create_conv_real) add to dfft_conv.h: the width of the plan's
// private half spectrum and the re-layout of a filter given in the R2C result layout into the X stage's slab (dfft_conv_real.hip).
// Internal header (the C-ABI is include/dfft.h).
#pragma once
#include <hip/hip_runtime.h>

#include "dfft_conv.h"

namespace dfft {

// Complex width Nc >= Nh = N2/2 + 1 of the plan's spectrum (columns Nh .. Nc - 1 hold zeros).  Nobody but the plan sees the spectrum, so
// its rows may be as wide as suits the kernels:
//   * Nc is even: fp32 Y passes, pack / unpack and the fused X stage then run on column pairs instead of the scalar float2 kernels;
//   * Nc is a multiple of the largest power of two g <= one 128-byte line of elements (8 fp64, 16 fp32) whose padding costs at most
//     Nh / 32 columns (3.1 % of the exchange bytes and of every pass): rows of the received slab [x][y_local][Nc] then start on whole
//     lines (g = a line) or on as coarse a boundary as that budget buys; g = 2 when nothing coarser fits.
// Nh = 257: 264 in both precisions (+2.7 %; fp32 rows on 64-byte boundaries); Nh = 129: 132 (+2.3 %); Nh = 33: 34; Nh = 16: 16.
// Pure host arithmetic.
long long conv_real_width(long long nh, int dtype);

// Filter re-layout of dfft_conv_set_filter on a real-field plan: the caller's h[(r * nh + kz) * n0 + kx] (L.filter_real: reals, else
// complex elements of L.dtype) times L.scale into the slab layout of L, dst[kx * L.plane + r * L.pitch + kz].  Runs over the DESTINATION:
// every element of the L.pitch-wide rows is written, zeros in the columns nh .. L.pitch - 1 (pad columns of the spectrum and the row
// padding of the intermediate) -- L.plane == L.rows * L.pitch in every layout these plans use, so the whole copy is defined afterwards.
hipError_t launch_conv_real_relayout(const ConvLaunch& L, long long nh, const void* h, void* dst, hipStream_t stream);

}  // namespace dfft
