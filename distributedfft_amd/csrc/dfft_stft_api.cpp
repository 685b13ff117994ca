// dfft_stft_api.cpp -- the plan-less entry points of the batched short-time Fourier transform and its inverse (dfft_stft.hip):
// dfft_stft1d, dfft_istft1d, and the host arithmetic that tells their frame count, route and scratch.
#include <cstring>

#include "dfft_plan_impl.h"
#include "dfft_stft.h"

using namespace dfft;

namespace {

StftLaunch fwd_launch(const void* in, void* out, const void* win, long long n, long long m, long long hop, long long pad, long long frames, long long rows,
                      int dtype, int pad_mode, int out_kind, double scale) {
    StftLaunch L;
    std::memset(&L, 0, sizeof(L));
    L.dtype = dtype;
    L.pad_mode = pad_mode;
    L.out_kind = out_kind;
    L.n = n;
    L.m = m;
    L.hop = hop;
    L.pad = pad;
    L.frames = frames;
    L.rows = rows;
    L.scale = scale;
    L.in = in;
    L.out = out;
    L.win = win;
    return L;
}

IstftLaunch inv_launch(const void* in, void* out, const void* win, const void* inv_env, long long n, long long m, long long hop, long long pad,
                       long long frames, long long rows, int dtype) {
    IstftLaunch L;
    std::memset(&L, 0, sizeof(L));
    L.dtype = dtype;
    L.n = n;
    L.m = m;
    L.hop = hop;
    L.pad = pad;
    L.frames = frames;
    L.rows = rows;
    L.in = in;
    L.out = out;
    L.win = win;
    L.inv_env = inv_env;
    return L;
}

}  // namespace

extern "C" {

long long dfft_stft1d_frames(long long n, long long m, long long hop, long long pad) { return stft_frames(n, m, hop, pad); }

int dfft_stft1d_fused_applies(long long m, int dtype) { return valid_dtype(dtype) && stft_fused_env() && stft_fused(m, dtype); }

unsigned long long dfft_stft1d_scratch_bytes(long long m, long long frames, long long rows, int dtype, int out_kind) {
    if (!valid_dtype(dtype) || m < 1 || frames < 1 || rows < 1 || real_form(m) != 1 || !stft_items_ok(rows, frames) ||
        (out_kind != DFFT_STFT_OUT_COMPLEX && out_kind != DFFT_STFT_OUT_POWER))
        return 0;
    // the lease depends on neither n, hop, pad nor the pad mode: a call with hop = m and no padding that has this many frames
    const StftLaunch L = fwd_launch(nullptr, nullptr, nullptr, frames * m, m, m, 0, frames, rows, dtype, DFFT_STFT_PAD_ZERO, out_kind, 1.0);
    return stft_scratch_bytes(L, stft_fused_env());
}

unsigned long long dfft_istft1d_scratch_bytes(long long m, long long frames, long long rows, int dtype) {
    if (!valid_dtype(dtype) || m < 1 || frames < 1 || rows < 1 || real_form(m) != 1 || !stft_items_ok(rows, frames)) return 0;
    // hop = m: one frame per output sample, the smallest lease of this (m, frames, rows); a smaller hop may raise it to ceil(m / hop) items
    const IstftLaunch L = inv_launch(nullptr, nullptr, nullptr, nullptr, 1, m, m, 0, frames, rows, dtype);
    return istft_scratch_bytes(L);
}

// Rows of reals [rows][n] -> [rows][frames][m/2 + 1] bins (or their squared moduli) of the windowed frames of m reals that advance by hop
int dfft_stft1d(const void* in, void* out, const void* win, long long n, long long m, long long hop, long long pad, long long frames, long long rows,
                int dtype, int pad_mode, int out_kind, double scale, void* stream) {
    if (!in || !out || !win || n < 1 || m < 1 || hop < 1 || pad < 0 || pad > m - 1 || frames < 1 || rows < 1 || !valid_dtype(dtype) ||
        (pad_mode != DFFT_STFT_PAD_ZERO && pad_mode != DFFT_STFT_PAD_REFLECT) || (out_kind != DFFT_STFT_OUT_COMPLEX && out_kind != DFFT_STFT_OUT_POWER) ||
        (pad_mode == DFFT_STFT_PAD_REFLECT && pad >= n) || frames > stft_frames(n, m, hop, pad))
        return fail(DFFT_EINVAL, "dfft_stft1d: bad arguments (1 <= frames <= dfft_stft1d_frames, 0 <= pad < m, reflect padding needs pad < n)");
    if (real_form(m) != 1)
        return fail(DFFT_EUNSUPPORTED, "dfft_stft1d: m = " + std::to_string(m) + " -- the frame length must be of dfft_real_form 1 (even, m/2 a single-pass "
                                       "length, so at most 8192); four-step and Bluestein frames are not built");
    if (!stft_items_ok(rows, frames)) return fail(DFFT_EUNSUPPORTED, "dfft_stft1d: rows * frames = 2^31 or more items: split the batch");
    const size_t    cs = elem_bytes(dtype), rs = cs / 2;
    const uintptr_t ibytes = (uintptr_t)rows * n * rs, wbytes = (uintptr_t)m * rs;
    const uintptr_t obytes = (uintptr_t)rows * frames * (m / 2 + 1) * (out_kind == DFFT_STFT_OUT_POWER ? rs : cs);
    if (ranges_overlap(in, ibytes, out, obytes)) return fail(DFFT_EINVAL, "dfft_stft1d: in and out overlap (frames read what their neighbours write)");
    if (ranges_overlap(win, wbytes, out, obytes)) return fail(DFFT_EINVAL, "dfft_stft1d: the window overlaps out");
    if (ranges_overlap(win, wbytes, in, ibytes)) return fail(DFFT_EINVAL, "dfft_stft1d: the window overlaps in");
    if (dfft_device_count() < 1) return fail(DFFT_ENOGPU, "dfft_stft1d: no HIP device visible (no CPU fallback)");
    const hipStream_t st = (hipStream_t)stream;
    const bool        fused_on = stft_fused_env();
    const StftLaunch  L = fwd_launch(in, out, win, n, m, hop, pad, frames, rows, dtype, pad_mode, out_kind, scale);
    const size_t      need = stft_scratch_bytes(L, fused_on);
    ScratchLease      lease;
    if (need && !lease.acquire(need, st)) return fail(DFFT_EHIP, "dfft_stft1d: cannot allocate the scratch buffer");
    return stft(L, fused_on, lease.get(), need, st);
}

// [rows][frames][m/2 + 1] bins -> rows of reals [rows][n]: the windowed overlap-add of the frames' inverse transforms times inv_env
int dfft_istft1d(const void* in, void* out, const void* win, const void* inv_env, long long n, long long m, long long hop, long long pad, long long frames,
                 long long rows, int dtype, void* stream) {
    if (!in || !out || !win || !inv_env || n < 1 || m < 1 || hop < 1 || pad < 0 || pad > m - 1 || frames < 1 || rows < 1 || !valid_dtype(dtype) ||
        !istft_length_ok(n, m, hop, pad, frames))
        return fail(DFFT_EINVAL, "dfft_istft1d: bad arguments (0 <= pad < m, 1 <= n <= (frames - 1) hop + m - pad)");
    if (real_form(m) != 1)
        return fail(DFFT_EUNSUPPORTED, "dfft_istft1d: m = " + std::to_string(m) + " -- the frame length must be of dfft_real_form 1 (even, m/2 a single-pass "
                                       "length, so at most 8192); four-step and Bluestein frames are not built");
    if (!stft_items_ok(rows, frames)) return fail(DFFT_EUNSUPPORTED, "dfft_istft1d: rows * frames = 2^31 or more items: split the batch");
    const size_t    cs = elem_bytes(dtype), rs = cs / 2;
    const uintptr_t ibytes = (uintptr_t)rows * frames * (m / 2 + 1) * cs, obytes = (uintptr_t)rows * n * rs, wbytes = (uintptr_t)m * rs, ebytes = (uintptr_t)n * rs;
    if (ranges_overlap(in, ibytes, out, obytes)) return fail(DFFT_EINVAL, "dfft_istft1d: in and out overlap");
    if (ranges_overlap(win, wbytes, out, obytes)) return fail(DFFT_EINVAL, "dfft_istft1d: the window overlaps out");
    if (ranges_overlap(inv_env, ebytes, out, obytes)) return fail(DFFT_EINVAL, "dfft_istft1d: inv_env overlaps out");
    if (ranges_overlap(win, wbytes, in, ibytes) || ranges_overlap(inv_env, ebytes, in, ibytes) || ranges_overlap(win, wbytes, inv_env, ebytes))
        return fail(DFFT_EINVAL, "dfft_istft1d: in, win and inv_env overlap");
    if (dfft_device_count() < 1) return fail(DFFT_ENOGPU, "dfft_istft1d: no HIP device visible (no CPU fallback)");
    const hipStream_t st = (hipStream_t)stream;
    const IstftLaunch L = inv_launch(in, out, win, inv_env, n, m, hop, pad, frames, rows, dtype);
    const size_t      need = istft_scratch_bytes(L);
    ScratchLease      lease;
    if (!need || !lease.acquire(need, st)) return fail(DFFT_EHIP, "dfft_istft1d: cannot allocate the scratch buffer");
    return istft(L, lease.get(), need, st);
}

}  // extern "C"
