// dfft_xspec_api.cpp -- the plan-less entry points of the batched 1-D real cross-spectrum (dfft_xspec.hip): dfft_rxspec1d, and the host
// arithmetic that tells its route, slice count and scratch.
#include <cstring>

#include "dfft_plan_impl.h"
#include "dfft_xspec.h"

using namespace dfft;

namespace {

RxspecLaunch make_launch(const void* x, const void* g, void* out, long long n, long long m, long long channels, long long batch, int dtype) {
    RxspecLaunch L;
    std::memset(&L, 0, sizeof(L));
    L.dtype = dtype;
    L.n = n;
    L.m = m;
    L.channels = channels;
    L.batch = batch;
    L.x = x;
    L.g = g;
    L.out = out;
    return L;
}

bool rows_ok(long long channels, long long batch) { return channels < (1ll << 31) && batch < (1ll << 31) && batch * channels < (1ll << 31); }

}  // namespace

extern "C" {

int dfft_rxspec1d_fused_applies(long long n, long long m, int dtype, int vec) {
    return valid_dtype(dtype) && rxspec_fused_env() && rxspec_fused(n, m, dtype, vec != 0);
}

long long dfft_rxspec1d_slices(long long m, long long channels, long long batch, int dtype) {
    if (!valid_dtype(dtype) || m < 1 || channels < 1 || batch < 1 || real_form(m) != 1 || !rows_ok(channels, batch)) return 0;
    return rxspec_slices(m, channels, batch, dtype);
}

unsigned long long dfft_rxspec1d_scratch_bytes(long long n, long long m, long long channels, long long batch, int dtype) {
    if (!valid_dtype(dtype) || n < 1 || m < n || channels < 1 || batch < 1 || real_form(m) != 1 || !rows_ok(channels, batch)) return 0;
    // (the route depends on neither the alignment nor on whether g is x)
    return rxspec_scratch_bytes(make_launch(nullptr, nullptr, nullptr, n, m, channels, batch, dtype), rxspec_fused_env(), chunk_cap_env());
}

// Cross-spectrum of the rows of reals x, g [batch][channels][n], zero-padded to m, summed over the batch into out [channels][m/2 + 1]
int dfft_rxspec1d(const void* x, const void* g, void* out, long long n, long long m, long long channels, long long batch, int dtype, void* stream) {
    if (!x || !g || !out || n < 1 || m < 1 || channels < 1 || batch < 1 || m < n || !valid_dtype(dtype))
        return fail(DFFT_EINVAL, "dfft_rxspec1d: bad arguments");
    if (real_form(m) != 1)
        return fail(DFFT_EUNSUPPORTED, "dfft_rxspec1d: m = " + std::to_string(m) + " -- the padded length must be of dfft_real_form 1 (even, m/2 a single-pass "
                                       "length, so at most 8192; dfft_rconv1d_length); longer sequences are not built");
    if (!rows_ok(channels, batch)) return fail(DFFT_EUNSUPPORTED, "dfft_rxspec1d: batch * channels = 2^31 or more rows: split the batch");
    const size_t    cs = elem_bytes(dtype), rs = cs / 2;
    const uintptr_t ibytes = (uintptr_t)batch * channels * n * rs, obytes = (uintptr_t)channels * (m / 2 + 1) * cs;
    if (ranges_overlap(x, ibytes, out, obytes) || ranges_overlap(g, ibytes, out, obytes))
        return fail(DFFT_EINVAL, "dfft_rxspec1d: out overlaps x or g");
    if (dfft_device_count() < 1) return fail(DFFT_ENOGPU, "dfft_rxspec1d: no HIP device visible (no CPU fallback)");
    const hipStream_t  st = (hipStream_t)stream;
    const bool         fused_on = rxspec_fused_env();
    const size_t       cap = chunk_cap_env();
    const RxspecLaunch L = make_launch(x, g, out, n, m, channels, batch, dtype);
    const size_t       need = rxspec_scratch_bytes(L, fused_on, cap);
    ScratchLease       lease;
    if (need && !lease.acquire(need, st)) return fail(DFFT_EHIP, "dfft_rxspec1d: cannot allocate the scratch buffer");
    return rxspec(L, fused_on, cap, lease.get(), need, st);
}

}  // extern "C"
