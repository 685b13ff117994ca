// dfft_csd_api.cpp -- the plan-less entry points of the framed (Welch) 1-D real cross-spectrum (dfft_csd.hip): dfft_rcsd1d, and the host
// arithmetic that tells its route, slice count and scratch.
#include <cstring>

#include "dfft_csd.h"
#include "dfft_plan_impl.h"
#include "dfft_stft.h"

using namespace dfft;

namespace {

RcsdLaunch make_launch(const void* x, const void* g, void* out, const void* win, long long n, long long m, long long hop, long long frames, long long rows,
                       double scale, int dtype) {
    RcsdLaunch L;
    std::memset(&L, 0, sizeof(L));
    L.dtype = dtype;
    L.n = n;
    L.m = m;
    L.hop = hop;
    L.frames = frames;
    L.rows = rows;
    L.scale = scale;
    L.x = x;
    L.g = g;
    L.out = out;
    L.win = win;
    return L;
}

}  // namespace

extern "C" {

int dfft_rcsd1d_fused_applies(long long m, int dtype, int autos) { return valid_dtype(dtype) && rcsd_fused_env() && rcsd_fused(m, dtype, autos != 0); }

long long dfft_rcsd1d_slices(long long m, long long rows, long long frames, int dtype) {
    if (!valid_dtype(dtype) || m < 1 || rows < 1 || frames < 1 || real_form(m) != 1 || !rcsd_items_ok(rows, frames)) return 0;
    return rcsd_slices(m, rows, frames, dtype);
}

unsigned long long dfft_rcsd1d_scratch_bytes(long long m, long long frames, long long rows, int dtype, int autos) {
    if (!valid_dtype(dtype) || m < 1 || rows < 1 || frames < 1 || real_form(m) != 1 || !rcsd_items_ok(rows, frames)) return 0;
    // the lease depends on neither n nor hop: a call with hop = m that has this many frames (g == x: the auto-spectrum's route)
    const void* x = &dtype;
    const void* g = autos ? x : (const void*)&autos;
    return rcsd_scratch_bytes(make_launch(x, g, nullptr, nullptr, frames * m, m, m, frames, rows, 1.0, dtype), rcsd_fused_env());
}

// Rows of reals x, g [rows][n] -> out [rows][m/2 + 1]: scale times the sum over the whole frames of m reals that advance by hop of
// conj(rfft(win * frame of x)) * rfft(win * frame of g)
int dfft_rcsd1d(const void* x, const void* g, void* out, const void* win, long long n, long long m, long long hop, long long frames, long long rows,
                double scale, int dtype, void* stream) {
    if (!x || !g || !out || !win || n < 1 || m < 1 || hop < 1 || frames < 1 || rows < 1 || n < m || !valid_dtype(dtype) ||
        frames != stft_frames(n, m, hop, 0))
        return fail(DFFT_EINVAL, "dfft_rcsd1d: bad arguments (hop >= 1, n >= m, frames = dfft_stft1d_frames(n, m, hop, 0) = 1 + (n - m) / hop)");
    if (real_form(m) != 1)
        return fail(DFFT_EUNSUPPORTED, "dfft_rcsd1d: m = " + std::to_string(m) + " -- the frame length must be of dfft_real_form 1 (even, m/2 a single-pass "
                                       "length, so at most 8192); four-step and Bluestein frames are not built");
    // several slices mean at most 16384 (row, slice) items, so the item count reaches 2^31 with the rows alone
    if (rows >= (1ll << 31))
        return fail(DFFT_EUNSUPPORTED, "dfft_rcsd1d: rows * slices = 2^31 or more items: split the rows into several calls");
    if (frames >= (1ll << 31))
        return fail(DFFT_EUNSUPPORTED, "dfft_rcsd1d: 2^31 or more frames per row: split the rows at a multiple of hop (the second part starts at sample "
                                       "frames_1 * hop) and add the results");
    const size_t    cs = elem_bytes(dtype), rs = cs / 2;
    // rows < 2^31; a field of 2^63 bytes or more cannot exist: its extent is held at the largest value instead of wrapping
    const unsigned __int128 wide = (unsigned __int128)rows * (unsigned __int128)n * rs;
    const uintptr_t         ibytes = wide > (unsigned __int128)UINTPTR_MAX ? UINTPTR_MAX : (uintptr_t)wide;
    const uintptr_t         wbytes = (uintptr_t)m * rs, obytes = (uintptr_t)rows * (m / 2 + 1) * cs;
    if (ranges_overlap(x, ibytes, out, obytes) || ranges_overlap(g, ibytes, out, obytes)) return fail(DFFT_EINVAL, "dfft_rcsd1d: out overlaps x or g");
    if (ranges_overlap(win, wbytes, out, obytes)) return fail(DFFT_EINVAL, "dfft_rcsd1d: the window overlaps out");
    if (dfft_device_count() < 1) return fail(DFFT_ENOGPU, "dfft_rcsd1d: no HIP device visible (no CPU fallback)");
    const hipStream_t st = (hipStream_t)stream;
    const bool        fused_on = rcsd_fused_env();
    const RcsdLaunch  L = make_launch(x, g, out, win, n, m, hop, frames, rows, scale, dtype);
    const size_t      need = rcsd_scratch_bytes(L, fused_on);
    ScratchLease      lease;
    if (need && !lease.acquire(need, st)) return fail(DFFT_EHIP, "dfft_rcsd1d: cannot allocate the scratch buffer");
    return rcsd(L, fused_on, lease.get(), need, st);
}

}  // extern "C"
