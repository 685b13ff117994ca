// dfft_batch.cpp -- the plan-less batched entry points: complex and real 1-D transforms along rows or a strided axis, batched 2-D
// transforms, real-to-real transforms, the 1-D real FFT convolution with its overlap-save and long forms, the long cross-spectrum,
// dfft_scale and dfft_trim.
#include <map>
#include <mutex>
#include <tuple>

#include "dfft_fused_host.h"
#include "dfft_lconv.h"
#include "dfft_lxspec.h"
#include "dfft_osconv.h"
#include "dfft_plan_impl.h"
#include "dfft_r2r.h"
#include "dfft_rconv.h"
#include "dfft_real.h"
#include "dfft_real_cols.h"
#include "dfft_real_pair.h"
#include "dfft_rows_common.h"

using namespace dfft;

// ---- batched 2D transform: the plan's t0 stage as an entry point of its own ------------------------------------
// Planes per group of `batch` planes of plane_b bytes that fit the 256 MiB Infinity Cache (dfft_plan_create's rule for single-GPU plans:
// one plane less per group from 8 MiB planes on, groups of equal size): the column pass then reads what the row pass wrote from the cache.
// (Not cache_chunk_planes: that rule has no "fits as a whole" answer of its own, and its DFFT_CHUNK_MB / DFFT_CHUNK_PLANES overrides are
// plan options that the plan-less entry points have never read.)
static long long cache_plane_group(long long batch, long long plane_b) {
    return batch * plane_b <= (256ll << 20) ? batch : evened_chunk_planes(batch, plane_b, 256);
}

// State of the one-launch stage for one (device, stream, plane shape, structure): the kernel's control block, its pinned error word and
// the host's running ticket / execute counters (dfft_zy.hip) -- what a plan keeps in dfft_plan_s, cached here because the call is
// plan-less.  Freed by dfft_trim().
namespace {
struct Zy2dCtx {
    ZyCtl*    ctl = nullptr;
    unsigned* err = nullptr;
    unsigned  ticket = 0, execs = 0;
    long long batch = 0;    // planes of the last launch on this context (0: none since the control block was zeroed)
    bool      off = false;  // a launch gave up: this context stays on two launches per chunk
};
struct Zy2dKey {
    int         dev;
    hipStream_t stream;
    int         n1, n2, sign;
    bool        operator<(const Zy2dKey& o) const { return std::tie(dev, stream, n1, n2, sign) < std::tie(o.dev, o.stream, o.n1, o.n2, o.sign); }
};
std::mutex                 g_zy2d_mutex;
std::map<Zy2dKey, Zy2dCtx> g_zy2d;

void zy2d_trim() {
    std::lock_guard<std::mutex> lk(g_zy2d_mutex);
    int                         cur = 0;
    (void)hipGetDevice(&cur);
    for (auto& kv : g_zy2d) {
        (void)hipSetDevice(kv.first.dev);
        (void)hipDeviceSynchronize();
        if (kv.second.ctl) (void)hipFree(kv.second.ctl);
        if (kv.second.err) (void)hipHostFree(kv.second.err);
    }
    g_zy2d.clear();
    (void)hipSetDevice(cur);
}
}  // namespace

// ---- shared by dfft_rfft1d, dfft_rfft1d_strided and dfft_rfft2d_batch ------------------------------------------------------------------
// A caller that needs the per-(device, stream) scratch for more than one step at a time (dfft_rfft2d_batch's inverse: the bins of a plane
// group and the scratch of the transforms on them) takes ONE lease for all of it -- the lease is not re-entrant -- so these helpers size
// their scratch first (*_prepare) and then run on whatever scratch they are given (*_run).

// Real rows of dfft_rfft1d: `rows` rows of n reals <-> n/2 + 1 bins.  in_is_scratch: the C2R input is the caller's own scratch, which
// the two-launch C2R form of real form 1 may merge in place on (no copy into scratch first).
struct RealRowsPass {
    long long          n, chunk;  // rows per launch
    int                dtype, dir, form;
    bool               copy;      // form 1 C2R with n/2 untuned: the bins go through scratch first
    BluesteinTablesPtr t;         // forms 2 / 3 with a Bluestein n
    bool               bs_fused;
    size_t             cap;       // chunk_cap_env() of the call
    size_t             need;      // scratch bytes
};
// sizes_only: tables that carry n, M and the dtype alone stand in for the cached ones -- the lease queries, which touch no device
static int real_rows_prepare(long long n, long long rows, int dtype, int dir, bool in_is_scratch, size_t cap, RealRowsPass* R,
                             const BluesteinTables* sizes_only = nullptr) {
    const size_t    cs = elem_bytes(dtype);
    const long long nh = n / 2 + 1;
    // rows as one plane: real pitch n, complex pitch nh; at most 2^30 rows per launch (an even count: pairs never straddle two calls)
    const long long max_rows = 1ll << 30;
    R->n = n;
    R->dtype = dtype;
    R->dir = dir;
    R->form = real_form(n);
    R->t.reset();
    R->bs_fused = true;
    R->cap = cap;
    R->copy = false;
    R->chunk = max_rows;
    R->need = 0;
    if (R->form == 1) {
        // the half-length kernels; their two-launch C2R form (n/2 without a tuned plan) merges in place on its input, so the bins go
        // through the per-(device, stream) scratch first, in chunks of at most 256 MiB
        R->copy = dir != DFFT_FORWARD && !fft_length_tuned((int)(n / 2)) && !in_is_scratch;
        if (R->copy) {
            R->chunk = std::max(1ll, std::min(max_rows, (long long)((256ll << 20) / (nh * (long long)cs))));
            R->need = (size_t)std::min(R->chunk, rows) * nh * cs;
        }
        return DFFT_OK;
    }
    // two-for-one pairs: the cached Bluestein tables of (n, dtype, direction) for Bluestein lengths
    if (length_kind(n) == 3 && !sizes_only)
        if (int rc = bluestein_tables(n, dtype, dir, &R->t)) return rc;
    R->bs_fused = bluestein_fused_env();
    R->need = real_pair_scratch_bytes(n, dtype, std::min(rows, max_rows), length_kind(n) == 3 && sizes_only ? sizes_only : R->t.get(), R->bs_fused, cap);
    return DFFT_OK;
}
static int real_rows_run(const RealRowsPass& R, const void* in, void* out, long long rows, void* scr, hipStream_t st) {
    const bool      fwd = R.dir == DFFT_FORWARD;
    const long long n = R.n, nh = n / 2 + 1;
    const size_t    cs = elem_bytes(R.dtype), rs = cs / 2;
    int             rc = DFFT_OK;
    for (long long b0 = 0; b0 < rows && rc == DFFT_OK; b0 += R.chunk) {
        const long long m = std::min(R.chunk, rows - b0);
        const void*     ip = (const char*)in + (size_t)b0 * (fwd ? n * rs : nh * cs);
        void*           op = (char*)out + (size_t)b0 * (fwd ? nh * cs : n * rs);
        if (R.form == 1) {
            RealLaunch L;
            std::memset(&L, 0, sizeof(L));
            L.dtype = R.dtype;
            L.n2 = (int)n;
            L.dir = R.dir;
            L.in = ip;
            L.out = op;
            L.rows = m;
            L.rows_per_plane = m;
            L.rpitch = n;
            L.rplane = m * n;
            L.cpitch = nh;
            L.cplane = m * nh;
            L.scale = 1.0;
            if (R.copy) {
                const hipError_t e = hipMemcpyAsync(scr, L.in, (size_t)m * nh * cs, hipMemcpyDeviceToDevice, st);
                if (e != hipSuccess) rc = fail(DFFT_EHIP, std::string("dfft_rfft1d: ") + hipGetErrorString(e));
                L.in = scr;
            }
            if (rc == DFFT_OK) rc = check_launch(launch_real_rows(L, st), fwd ? "dfft_rfft1d (R2C rows)" : "dfft_rfft1d (C2R rows)");
        } else {
            RealPairLaunch P;
            std::memset(&P, 0, sizeof(P));
            P.dtype = R.dtype;
            P.n = n;
            P.dir = R.dir;
            P.in = ip;
            P.out = op;
            P.rows = m;
            P.rows_per_plane = m;
            P.rpitch = n;
            P.rplane = m * n;
            P.cpitch = nh;
            P.cplane = m * nh;
            rc = real_pair_rows(P, R.t.get(), R.bs_fused, R.cap, scr, R.need, st);
        }
    }
    return rc;
}

// dfft_fft1d_any's transforms of [batch][n][s] on caller-provided scratch (the four-step and Bluestein forms need some; dfft_fft1d_any
// itself leases it inside dfft_fft1d_rows / dfft_fft1d_cols / bluestein_pass)
struct AnyPass {
    long long          n, s;
    int                dtype, dir, kind;
    BluesteinTablesPtr t;
    bool               bs_fused;
    size_t             need;
};
static int any_prepare(long long n, long long s, long long batch, int dtype, int dir, size_t cap, AnyPass* A, const BluesteinTables* sizes_only = nullptr) {
    A->n = n;
    A->s = s;
    A->dtype = dtype;
    A->dir = dir;
    A->kind = length_kind(n);
    A->t.reset();
    A->bs_fused = bluestein_fused_env();
    A->need = A->kind == 2 ? (size_t)batch * n * s * elem_bytes(dtype) : 0;
    if (A->kind == 3) {
        if (!sizes_only)
            if (int rc = bluestein_tables(n, dtype, dir, &A->t)) return rc;
        A->need = bluestein_scratch_bytes(sizes_only ? *sizes_only : *A->t, s, batch, A->bs_fused, cap);
    }
    return DFFT_OK;
}
static int any_run(const AnyPass& A, const void* in, void* out, long long batch, void* scr, hipStream_t st) {
    if (A.kind == 3) return bluestein_fft(*A.t, in, out, A.s, batch, 1.0, A.bs_fused, scr, A.need, st);
    if (A.kind == 2) return long_fft(in, out, A.n, A.s, batch, A.dtype, A.dir, 1.0, scr, st);
    return A.s == 1 ? dfft_fft1d_rows((void*)in, out, A.n, batch, A.dtype, A.dir, st) : dfft_fft1d_cols((void*)in, out, A.n, A.s, batch, A.dtype, A.dir, st);
}

// Rows per chunk of the composed long routes (dfft_rconv1d_long, dfft_rxspec1d_long): rows of rb bytes within max(cap, one row's), and
// -- the padded rows are of real form 3, so rows 2p and 2p + 1 of the call share their transforms -- whole pairs unless the chunk is the
// whole call: a chunk of an odd number of rows would pair every later row with its other neighbour.
static long long long_composed_chunk_rows(size_t rb, long long rows, size_t cap) {
    const long long nr = chunk_units(rb, rows, cap, 2);
    return nr < rows ? nr - (nr & 1) : nr;
}

static void sizes_only_tables(BluesteinTables* T, long long n, int dtype, int dir) {
    T->n = n;
    T->M = bluestein_padded_length(n);
    T->dtype = dtype;
    T->dir = dir;
}

extern "C" {

// ---- test hooks: the per-(device, stream) scratch buffer as earlier calls left it (dfft_long.hip).  Without a device they touch none.
int dfft_debug_scratch_fill(unsigned long long at_least_bytes, int byte, void* stream) {
    if (dfft_device_count() < 1) return fail(DFFT_ENOGPU, "dfft_debug_scratch_fill: no HIP device visible");
    return long_scratch_debug_fill((size_t)at_least_bytes, byte, (hipStream_t)stream);
}
unsigned long long dfft_debug_scratch_capacity(void* stream) {
    if (dfft_device_count() < 1) return 0;
    return long_scratch_debug_capacity((hipStream_t)stream);
}
long long dfft_debug_scratch_count(int byte, void* stream) {
    if (dfft_device_count() < 1) return fail(DFFT_ENOGPU, "dfft_debug_scratch_count: no HIP device visible");
    return long_scratch_debug_count(byte, (hipStream_t)stream);
}

// ---- the leases of dfft_rfft1d, dfft_rfft2d_batch and dfft_fft2d_batch by the routines' own rules (host arithmetic, no device): the
// largest single lease of the call, which is what the grow-only buffer holds afterwards; 0: none, or sizes that are refused
unsigned long long dfft_rfft1d_scratch_bytes(long long n, long long batch, int dtype, int direction) {
    if (!valid_dtype(dtype) || !valid_direction(direction) || batch < 1 || real_form(n) == 0) return 0;
    BluesteinTables T;
    sizes_only_tables(&T, n, dtype, direction);
    RealRowsPass R;
    if (real_rows_prepare(n, batch, dtype, direction, false, chunk_cap_env(), &R, &T)) return 0;
    return R.need;
}
unsigned long long dfft_rfft2d_batch_scratch_bytes(long long n1, long long n2, long long batch, int dtype, int direction) {
    if (!valid_dtype(dtype) || !valid_direction(direction) || n1 < 1 || n2 < 1 || batch < 1 || real_form(n2) == 0 || length_kind(n1) == 0) return 0;
    const bool      fwd = direction == DFFT_FORWARD;
    const long long nh = n2 / 2 + 1;
    const uintptr_t cplane_b = (uintptr_t)n1 * nh * elem_bytes(dtype);
    const long long cp = cache_plane_group(batch, (long long)cplane_b);
    BluesteinTables T2, T1;
    sizes_only_tables(&T2, n2, dtype, direction);
    sizes_only_tables(&T1, n1, dtype, direction);
    const size_t cap = chunk_cap_env();
    RealRowsPass R;
    if (real_rows_prepare(n2, cp * n1, dtype, direction, !fwd, cap, &R, &T2)) return 0;
    if (fwd) return std::max<unsigned long long>(R.need, dfft_fft1d_any_scratch_bytes(n1, nh, cp, dtype));  // two leases, one after the other
    AnyPass A;
    if (any_prepare(n1, nh, cp, dtype, direction, cap, &A, &T1)) return 0;
    return (unsigned long long)cp * cplane_b + std::max(R.need, A.need);
}
unsigned long long dfft_fft2d_batch_scratch_bytes(long long n1, long long n2, long long batch, int dtype) {
    if (!valid_dtype(dtype) || n1 < 1 || n2 < 1 || batch < 1 || !dfft_length_supported(n1) || !dfft_length_supported(n2)) return 0;
    if (n1 <= 4096 && n2 <= 4096) return 0;  // single-pass axes, the one-launch stage included: no scratch
    return (unsigned long long)batch * n1 * n2 * elem_bytes(dtype);  // the four-step axis on dfft_fft1d_rows / dfft_fft1d_cols: as much as the data
}

int dfft_fft1d_rows(void* in, void* out, long long n, long long batch, int dtype, int direction, void* stream) {
    if (!in || !out || batch < 0 || !valid_dtype(dtype) || !valid_direction(direction))
        return fail(DFFT_EINVAL, "dfft_fft1d_rows: bad arguments");
    if (!dfft_length_supported(n)) return fail(DFFT_EUNSUPPORTED, "dfft_fft1d_rows: unsupported length");
    if (partly_overlap(in, out, (uintptr_t)batch * (uintptr_t)n * elem_bytes(dtype)))
        return fail(DFFT_EINVAL, "dfft_fft1d_rows: in and out overlap partly (the transform runs out of place or exactly in place)");
    if (dfft_device_count() < 1) return fail(DFFT_ENOGPU, "dfft_fft1d_rows: no HIP device visible (no CPU fallback)");
    return fft_rows(in, out, (int)n, batch, dtype, direction, (hipStream_t)stream);
}

// `batch` planes of [n1][n2] (n2 contiguous), each transformed along both axes; in place (out == in) or out of place (`in` is left
// untouched).  What a 3D plan runs as t0 (reference fftZY, fft_mpi_3d_api.cpp:466-522; templateFFT's FFTDim = 2 application,
// templateFFT.cpp:5767): planes are taken in groups that fit the 256 MiB Infinity Cache, so the column pass reads what the row pass
// wrote from the cache, and plane shapes the one-launch stage is built for (dfft_zy.hip: fp64, n1 in {256, 512, 768 (n2 = 512)}, n2 in
// {256, 512}) run as ONE persistent launch.  Forward: rows n2 then columns n1; backward: the same order with conjugated twiddles
// (the two 1-D transforms of a plane commute).  Un-normalised.
int dfft_fft2d_batch(void* in, void* out, long long n1, long long n2, long long batch, int dtype, int direction, void* stream) {
    if (!in || !out || n1 < 1 || n2 < 1 || batch < 0 || !valid_dtype(dtype) || !valid_direction(direction))
        return fail(DFFT_EINVAL, "dfft_fft2d_batch: bad arguments");
    if (!dfft_length_supported(n1) || !dfft_length_supported(n2)) return fail(DFFT_EUNSUPPORTED, "dfft_fft2d_batch: unsupported length");
    if (partly_overlap(in, out, (uintptr_t)batch * (uintptr_t)n1 * (uintptr_t)n2 * elem_bytes(dtype)))
        return fail(DFFT_EINVAL, "dfft_fft2d_batch: in and out overlap partly (the transform runs out of place or exactly in place)");
    if (dfft_device_count() < 1) return fail(DFFT_ENOGPU, "dfft_fft2d_batch: no HIP device visible (no CPU fallback)");
    if (batch == 0) return DFFT_OK;
    hipStream_t     s = (hipStream_t)stream;
    const long long plane = n1 * n2, plane_b = plane * (long long)elem_bytes(dtype);
    if (n1 > 4096 || n2 > 4096 || plane >= (1ll << 31)) {  // four-step axes: whole-buffer passes on the 1-D entry points
        int rc = dfft_fft1d_rows(in, out, n2, n1 * batch, dtype, direction, stream);
        if (rc == DFFT_OK) rc = dfft_fft1d_cols(out, out, n1, n2, batch, dtype, direction, stream);
        return rc;
    }
    static const bool one_launch_off = [] {
        const char* e = getenv("DFFT_T0_ONE_LAUNCH");
        return e && *e == '0';
    }();
    // ---- one persistent launch
    if (!one_launch_off && zy_supported(dtype, (int)n1, (int)n2) && batch <= ZY_MAX_PLANES) {
        int dev = 0;
        DFFT_HIP_TRY(hipGetDevice(&dev));
        std::lock_guard<std::mutex> lk(g_zy2d_mutex);
        Zy2dCtx&                    c = g_zy2d[Zy2dKey{dev, s, (int)n1, (int)n2, direction}];
        if (!c.off && !c.ctl) {
            // (zeroed on the caller's stream and waited for, like a plan's: dfft_plan_create)
            if (hipMalloc((void**)&c.ctl, sizeof(ZyCtl)) != hipSuccess || hipMemsetAsync(c.ctl, 0, sizeof(ZyCtl), s) != hipSuccess ||
                hipStreamSynchronize(s) != hipSuccess || hipHostMalloc((void**)&c.err, 128, hipHostMallocMapped) != hipSuccess) {
                (void)hipGetLastError();
                if (c.ctl) (void)hipFree(c.ctl);
                c.ctl = nullptr;
                c.off = true;
            } else {
                *c.err = 0u;
            }
        }
        if (!c.off && *(volatile unsigned*)c.err != 0u) {
            c.off = true;  // sticky on the device side too: every later launch on this block would return at once
            return fail(DFFT_EHIP, "dfft_fft2d_batch: an earlier one-launch YZ stage on this stream gave up; the results of that call and of every call queued "
                                   "behind it are invalid, later calls use two launches per chunk");
        }
        if (!c.off) {
            const void *twz = nullptr, *twy = nullptr;
            DFFT_TRY(get_twiddles((int)n2, dtype, &twz));
            DFFT_TRY(get_twiddles((int)n1, dtype, &twy));
            ZyLaunch L;
            std::memset(&L, 0, sizeof(L));
            L.dtype = dtype;
            L.n1 = (int)n1;
            L.n2 = (int)n2;
            L.dir = +1;  // rows first in both directions (the inverse: SIGN = -1, dfft_zy.hip)
            L.sign = direction;
            L.src = in;
            L.w = out;
            L.dst = nullptr;
            L.src_plane = L.w_plane = L.dst_plane = plane;
            L.plane0 = 0;
            L.nplanes = batch;
            const long long fit = std::max(1ll, (230ll << 20) / plane_b), nch = (batch + fit - 1) / fit;
            L.chunk = batch * plane_b <= (256ll << 20) ? batch : (batch + nch - 1) / nch;  // zy_phase_planes
            L.ctl = c.ctl;
            L.twz = twz;
            L.twy = twy;
            L.lazy = 1;
            static const unsigned polls = [] {
                const char* sp = getenv("DFFT_ZY_SPIN_POLLS");
                return sp && atoll(sp) > 0 ? (unsigned)std::min(atoll(sp), 0xffffffffll) : (4u << 20);
            }();
            L.spin_polls = polls;
            if (hipHostGetDevicePointer((void**)&L.err_host, c.err, 0) != hipSuccess) return fail(DFFT_EHIP, "dfft_fft2d_batch: no device pointer for the error word");
            // done_base = execs x producers holds only while every earlier launch on this block covered planes [0, batch): each one
            // added `producers` to done[p] of exactly those planes.  A plan always launches all of its planes, so its counters never
            // drift; this entry point takes any batch, so when the batch changes the control block is zeroed on the caller's stream
            // (stream order puts that behind every earlier launch of this context) and the host counters restart from 0.
            if (c.batch != batch) {
                if (c.batch != 0 && hipMemsetAsync(c.ctl, 0, sizeof(ZyCtl), s) != hipSuccess) {
                    (void)hipGetLastError();
                    return fail(DFFT_EHIP, "dfft_fft2d_batch: cannot reset the control block of the one-launch YZ stage");
                }
                c.ticket = 0;
                c.execs = 0;
                c.batch = batch;
            }
            unsigned producers = 0;
            (void)zy_units_per_plane(L.n1, L.n2, L.dir, 0, &producers);
            L.ticket_base = c.ticket;
            L.done_base = c.execs * producers;
            ++c.execs;
            c.ticket += zy_tickets(L.n1, L.n2, L.dir, 0, L.nplanes, L.chunk);
            return check_launch(launch_zy(L, s), "dfft_fft2d_batch (one-launch YZ stage)");
        }
    }
    // ---- two launches per Infinity-Cache chunk (dfft_plan_create's rule for single-GPU plans)
    const long long cp = cache_plane_group(batch, plane_b);
    const void* twy = nullptr;
    DFFT_TRY(get_twiddles((int)n1, dtype, &twy));
    const bool chunked = cp < batch;
    for (long long x0 = 0; x0 < batch; x0 += cp) {
        const long long nx = std::min(cp, batch - x0);
        DFFT_TRY(fft_rows(in, out, (int)n2, nx * n1, dtype, direction, s, x0 * n1, (chunked && in != out) ? FFT_HINT_STREAM_IN : 0));
        FftLaunch L;
        std::memset(&L, 0, sizeof(L));
        L.dtype = dtype;
        L.n = (int)n1;
        L.dir = direction;
        L.cols = 1;
        L.in = out;
        L.out = out;
        L.tw = twy;
        L.imap = L.omap = plain_axis(n1, n2, 1);
        L.itile = L.otile = TileMap{plane, 1};
        L.na = nx;
        L.a_first = x0;
        L.ncols = (int)n2;
        DFFT_TRY(check_launch(launch_fft(L, s), "dfft_fft2d_batch (columns)"));
    }
    return DFFT_OK;
}

// Did a one-launch stage of dfft_fft2d_batch on (current device, stream) give up?  Meant for after the caller has waited for the stream:
// it reads the pinned error words the kernels write.  A failure reported here is reported once -- the context then stays on two
// launches per chunk, and the next call on it does not report it again.
int dfft_fft2d_batch_status(void* stream) {
    int dev = 0;
    DFFT_HIP_TRY(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lk(g_zy2d_mutex);
    for (auto& kv : g_zy2d) {
        Zy2dCtx& c = kv.second;
        if (kv.first.dev != dev || kv.first.stream != (hipStream_t)stream || c.off || !c.err || *(volatile unsigned*)c.err == 0u) continue;
        c.off = true;
        return fail(DFFT_EHIP, "dfft_fft2d_batch: a one-launch YZ stage on this stream gave up (" + std::string(*c.err == ZY_ERR_DESYNC ? "control block out of step" : "timed out") +
                                   ", " + std::to_string(kv.first.n1) + "x" + std::to_string(kv.first.n2) + "); the results of that call and of every call queued "
                                   "behind it are invalid, later calls use two launches per chunk");
    }
    return DFFT_OK;
}

int dfft_trim(void) {
    long_scratch_trim();
    bluestein_trim();
    r2r_trim();
    zy2d_trim();
    return DFFT_OK;
}

int dfft_scale(void* data, long long count, int dtype, double s, void* stream) {
    if (!data || count < 0 || !valid_dtype(dtype)) return fail(DFFT_EINVAL, "dfft_scale: bad arguments");
    if (dfft_device_count() < 1) return fail(DFFT_ENOGPU, "dfft_scale: no HIP device visible (no CPU fallback)");
    hipError_t e = launch_scale(dtype, data, count, s, (hipStream_t)stream);
    if (e != hipSuccess) return fail(DFFT_EHIP, std::string("dfft_scale: ") + hipGetErrorString(e));
    return DFFT_OK;
}

int dfft_fft1d_any(void* in, void* out, long long n, long long s, long long batch, int dtype, int direction, void* stream) {
    if (!in || !out || batch < 0 || s < 1 || !valid_dtype(dtype) || !valid_direction(direction))
        return fail(DFFT_EINVAL, "dfft_fft1d_any: bad arguments");
    const int kind = length_kind(n);
    if (kind == 0) return fail(DFFT_EUNSUPPORTED, "dfft_fft1d_any: length " + std::to_string(n) + " is outside every form (at most 2^23, or a four-step length)");
    if (partly_overlap(in, out, (uintptr_t)batch * (uintptr_t)n * (uintptr_t)s * elem_bytes(dtype)))
        return fail(DFFT_EINVAL, "dfft_fft1d_any: in and out overlap partly (the transform runs out of place or exactly in place)");
    if (kind != 3)  // single-pass and four-step lengths: exactly the existing entry points
        return s == 1 ? dfft_fft1d_rows(in, out, n, batch, dtype, direction, stream) : dfft_fft1d_cols(in, out, n, s, batch, dtype, direction, stream);
    if (!any_extent_ok(n, s, dtype, aligned16(in), aligned16(out))) return fail(DFFT_EUNSUPPORTED, extent_message("dfft_fft1d_any", n, s));
    if (dfft_device_count() < 1) return fail(DFFT_ENOGPU, "dfft_fft1d_any: no HIP device visible (no CPU fallback)");
    if (batch == 0) return DFFT_OK;
    return bluestein_pass(in, out, n, s, batch, dtype, direction, 1.0, (hipStream_t)stream);
}

int dfft_rfft1d(void* in, void* out, long long n, long long batch, int dtype, int direction, void* stream) {
    if (!in || !out || batch < 0 || !valid_dtype(dtype) || !valid_direction(direction))
        return fail(DFFT_EINVAL, "dfft_rfft1d: bad arguments");
    const int form = real_form(n);
    if (form == 0) return fail(DFFT_EUNSUPPORTED, "dfft_rfft1d: length " + std::to_string(n) + " has no real form (at most 2^23, or a four-step length)");
    const bool      fwd = direction == DFFT_FORWARD;
    const size_t    cs = elem_bytes(dtype), rs = cs / 2;
    const long long nh = n / 2 + 1;
    // out of place: the byte ranges of in and out must not overlap
    if (ranges_overlap(in, (uintptr_t)batch * (fwd ? n * rs : nh * cs), out, (uintptr_t)batch * (fwd ? nh * cs : n * rs)))
        return fail(DFFT_EINVAL, "dfft_rfft1d: in and out overlap (the transform is out of place)");
    if (dfft_device_count() < 1) return fail(DFFT_ENOGPU, "dfft_rfft1d: no HIP device visible (no CPU fallback)");
    if (batch == 0) return DFFT_OK;
    const hipStream_t st = (hipStream_t)stream;
    RealRowsPass      R;
    if (int rc = real_rows_prepare(n, batch, dtype, direction, false, chunk_cap_env(), &R)) return rc;
    ScratchLease lease;
    if (R.need && !lease.acquire(R.need, st)) return fail(DFFT_EHIP, "dfft_rfft1d: cannot allocate the scratch buffer");
    return real_rows_run(R, in, out, batch, lease.get(), st);
}

// Real transforms along the middle axis of [batch][n][s] (dfft_real_cols.hip); s = 1 is dfft_rfft1d.
int dfft_rfft1d_strided(void* in, void* out, long long n, long long s, long long batch, int dtype, int direction, void* stream) {
    if (!in || !out || batch < 0 || s < 1 || !valid_dtype(dtype) || !valid_direction(direction))
        return fail(DFFT_EINVAL, "dfft_rfft1d_strided: bad arguments");
    if (length_kind(n) == 0)
        return fail(DFFT_EUNSUPPORTED, "dfft_rfft1d_strided: length " + std::to_string(n) + " has no real form (at most 2^23, or a four-step length)");
    const bool      fwd = direction == DFFT_FORWARD;
    const size_t    cs = elem_bytes(dtype), rs = cs / 2;
    const uintptr_t rb = (uintptr_t)batch * n * s * rs, cb = (uintptr_t)batch * (n / 2 + 1) * s * cs;
    if (ranges_overlap(in, fwd ? rb : cb, out, fwd ? cb : rb))
        return fail(DFFT_EINVAL, "dfft_rfft1d_strided: in and out overlap (the transform is out of place)");
    if (s == 1) return dfft_rfft1d(in, out, n, batch, dtype, direction, stream);
    if (!real_cols_fused(n, s, dtype)) {  // multi-pass: n-point columns of the (s + 1) / 2 packed pairs, straight from `in` / into `out` where
                                          // s is even and that pointer is aligned to a complex element, else on the scratch
        const bool direct = s % 2 == 0 && (uintptr_t)(fwd ? in : out) % cs == 0;
        const bool p16 = direct ? aligned16(fwd ? in : out) : scratch16();
        if (!any_extent_ok(n, (s + 1) / 2, dtype, fwd ? p16 : scratch16(), fwd ? scratch16() : p16))
            return fail(DFFT_EUNSUPPORTED, extent_message("dfft_rfft1d_strided (packed pairs)", n, (s + 1) / 2));
    }
    if (dfft_device_count() < 1) return fail(DFFT_ENOGPU, "dfft_rfft1d_strided: no HIP device visible (no CPU fallback)");
    if (batch == 0) return DFFT_OK;
    const hipStream_t  st = (hipStream_t)stream;
    BluesteinTablesPtr t;
    if (length_kind(n) == 3)
        if (int rc = bluestein_tables(n, dtype, direction, &t)) return rc;
    const bool       bs_fused = bluestein_fused_env();
    const size_t     cap = chunk_cap_env();
    const size_t     need = real_cols_scratch_bytes(n, s, batch, dtype, t.get(), bs_fused, cap);
    ScratchLease lease;
    if (need && !lease.acquire(need, st)) return fail(DFFT_EHIP, "dfft_rfft1d_strided: cannot allocate the scratch buffer");
    RealColsLaunch L;
    std::memset(&L, 0, sizeof(L));
    L.dtype = dtype;
    L.n = n;
    L.s = s;
    L.batch = batch;
    L.dir = direction;
    L.in = in;
    L.out = out;
    return real_cols(L, t.get(), bs_fused, cap, lease.get(), need, st);
}

// Real-to-real transforms (DCT / DST, types II and III) along the middle axis of [batch][n][s] (dfft_r2r.hip)
int dfft_r2r1d_strided(void* in, void* out, long long n, long long s, long long batch, int dtype, int kind, void* stream) {
    if (!in || !out || n < 1 || s < 1 || batch < 1 || !valid_dtype(dtype) || kind < DFFT_R2R_DCT2 || kind > DFFT_R2R_DST3)
        return fail(DFFT_EINVAL, "dfft_r2r1d_strided: bad arguments");
    if (length_kind(n) == 0)
        return fail(DFFT_EINVAL, "dfft_r2r1d_strided: length " + std::to_string(n) + " is outside every form (at most 2^23, or a four-step length)");
    const uintptr_t bytes = (uintptr_t)batch * n * s * (elem_bytes(dtype) / 2);
    if (in != out && ranges_overlap(in, bytes, out, bytes))
        return fail(DFFT_EINVAL, "dfft_r2r1d_strided: in and out overlap partly (the transform runs out of place or exactly in place)");
    if (s > 1 && !(r2r_fused_env() && r2r_fused(n, s, dtype, kind, r2r_vec(in, out, s, dtype))) &&
        !any_extent_ok(n, (s + 1) / 2, dtype, scratch16(), scratch16()))  // composed route: n-point columns in place on the scratch
        return fail(DFFT_EUNSUPPORTED, extent_message("dfft_r2r1d_strided (packed pairs)", n, (s + 1) / 2));
    if (dfft_device_count() < 1) return fail(DFFT_ENOGPU, "dfft_r2r1d_strided: no HIP device visible (no CPU fallback)");
    const hipStream_t  st = (hipStream_t)stream;
    const bool         three = kind == DFFT_R2R_DCT3 || kind == DFFT_R2R_DST3;
    const bool         fused_on = r2r_fused_env();
    R2rTablePtr        w;
    BluesteinTablesPtr t;
    if (int rc = r2r_table(n, dtype, &w)) return rc;
    if (length_kind(n) == 3)
        if (int rc = bluestein_tables(n, dtype, three ? DFFT_BACKWARD : DFFT_FORWARD, &t)) return rc;
    const bool   bs_fused = bluestein_fused_env();
    const size_t cap = chunk_cap_env();
    R2rLaunch    L;
    std::memset(&L, 0, sizeof(L));
    L.dtype = dtype;
    L.kind = kind;
    L.n = n;
    L.s = s;
    L.batch = batch;
    L.in = in;
    L.out = out;
    const size_t     need = r2r_scratch_bytes(L, fused_on, t.get(), bs_fused, cap);
    ScratchLease lease;
    if (need && !lease.acquire(need, st)) return fail(DFFT_EHIP, "dfft_r2r1d_strided: cannot allocate the scratch buffer");
    return r2r(L, *w, fused_on, t.get(), bs_fused, cap, lease.get(), need, st);
}

// Batched 1-D real FFT convolution of the rows of reals [batch][channels][n] with the spectra h [channels][m/2 + 1] (dfft_rconv.hip)
int dfft_rconv1d(const void* in, void* out, const void* h, long long n, long long m, long long channels, long long batch, int dtype, int filter_kind,
                 void* stream) {
    if (!in || !out || !h || n < 1 || m < 1 || channels < 1 || batch < 1 || m < n || !valid_dtype(dtype) ||
        (filter_kind != DFFT_FILTER_COMPLEX && filter_kind != DFFT_FILTER_REAL))
        return fail(DFFT_EINVAL, "dfft_rconv1d: bad arguments");
    if (real_form(m) != 1)
        return fail(DFFT_EUNSUPPORTED, "dfft_rconv1d: m = " + std::to_string(m) + " -- the padded length must be of dfft_real_form 1 (even, m/2 a single-pass "
                                       "length, so at most 8192; dfft_rconv1d_length); longer sequences are not built");
    if (channels >= (1ll << 31) || batch >= (1ll << 31) || batch * channels >= (1ll << 31))
        return fail(DFFT_EUNSUPPORTED, "dfft_rconv1d: batch * channels = 2^31 or more rows: split the batch");
    const size_t    cs = elem_bytes(dtype), rs = cs / 2;
    const uintptr_t bytes = (uintptr_t)batch * channels * n * rs;
    if (partly_overlap(in, out, bytes))
        return fail(DFFT_EINVAL, "dfft_rconv1d: in and out overlap partly (the convolution runs out of place or exactly in place)");
    if (ranges_overlap(h, (uintptr_t)channels * (m / 2 + 1) * (filter_kind == DFFT_FILTER_REAL ? rs : cs), out, bytes))
        return fail(DFFT_EINVAL, "dfft_rconv1d: the filter overlaps out");
    if (dfft_device_count() < 1) return fail(DFFT_ENOGPU, "dfft_rconv1d: no HIP device visible (no CPU fallback)");
    const hipStream_t st = (hipStream_t)stream;
    const bool        fused_on = rconv_fused_env();
    const size_t      cap = chunk_cap_env();
    RconvLaunch       L;
    std::memset(&L, 0, sizeof(L));
    L.dtype = dtype;
    L.filter_kind = filter_kind;
    L.n = n;
    L.m = m;
    L.channels = channels;
    L.batch = batch;
    L.in = in;
    L.out = out;
    L.h = h;
    const size_t need = rconv_scratch_bytes(L, fused_on, cap);
    ScratchLease lease;
    if (need && !lease.acquire(need, st)) return fail(DFFT_EHIP, "dfft_rconv1d: cannot allocate the scratch buffer");
    return rconv(L, fused_on, cap, lease.get(), need, st);
}

// Overlap-save 1-D real FFT convolution: rows of reals [batch][channels][n] of any length, filtered in blocks of m reals of which the
// first `discard` results are dropped, into [batch][channels][n_out] (dfft_osconv.hip)
int dfft_rconv1d_os(const void* in, void* out, const void* h, long long n, long long n_out, long long m, long long discard, long long channels,
                    long long batch, int dtype, int filter_kind, void* stream) {
    if (!in || !out || !h || n < 1 || n_out < 1 || m < 1 || discard < 0 || discard > m - 1 || channels < 1 || batch < 1 || n_out - discard > n ||
        !valid_dtype(dtype) || (filter_kind != DFFT_FILTER_COMPLEX && filter_kind != DFFT_FILTER_REAL))
        return fail(DFFT_EINVAL, "dfft_rconv1d_os: bad arguments");
    if (real_form(m) != 1)
        return fail(DFFT_EUNSUPPORTED, "dfft_rconv1d_os: m = " + std::to_string(m) + " -- the block length must be of dfft_real_form 1 (even, m/2 a single-pass "
                                       "length, so at most 8192; dfft_rconv1d_length); four-step and Bluestein halves are not built");
    const long long nb = osconv_blocks(n_out, m, discard);
    if (channels >= (1ll << 31) || batch >= (1ll << 31) || batch * channels >= (1ll << 31) || nb > ((1ll << 31) - 1) / (batch * channels))
        return fail(DFFT_EUNSUPPORTED, "dfft_rconv1d_os: batch * channels * blocks per row = 2^31 or more items: split the batch");
    const size_t    cs = elem_bytes(dtype), rs = cs / 2;
    const uintptr_t ibytes = (uintptr_t)batch * channels * n * rs, obytes = (uintptr_t)batch * channels * n_out * rs;
    if (ranges_overlap(in, ibytes, out, obytes))
        return fail(DFFT_EINVAL, "dfft_rconv1d_os: in and out overlap (blocks read what their neighbours write: there is no in-place form)");
    if (ranges_overlap(h, (uintptr_t)channels * (m / 2 + 1) * (filter_kind == DFFT_FILTER_REAL ? rs : cs), out, obytes))
        return fail(DFFT_EINVAL, "dfft_rconv1d_os: the filter overlaps out");
    if (dfft_device_count() < 1) return fail(DFFT_ENOGPU, "dfft_rconv1d_os: no HIP device visible (no CPU fallback)");
    const hipStream_t st = (hipStream_t)stream;
    const bool        fused_on = rconv_fused_env();
    const size_t      cap = chunk_cap_env();
    OsconvLaunch      L;
    std::memset(&L, 0, sizeof(L));
    L.dtype = dtype;
    L.filter_kind = filter_kind;
    L.n = n;
    L.n_out = n_out;
    L.m = m;
    L.discard = discard;
    L.channels = channels;
    L.batch = batch;
    L.in = in;
    L.out = out;
    L.h = h;
    const size_t need = osconv_scratch_bytes(L, fused_on, cap);
    ScratchLease lease;
    if (need && !lease.acquire(need, st)) return fail(DFFT_EHIP, "dfft_rconv1d_os: cannot allocate the scratch buffer");
    return osconv(L, fused_on, cap, lease.get(), need, st);
}

// Long 1-D real FFT convolution (dfft_lconv.hip): the padded lengths beyond dfft_rconv1d's, m/2 = N1 * N2
static std::string lconv_length_message(const char* who, long long m) {
    return std::string(who) + ": m = " + std::to_string(m) + " -- the padded length must be even, 8192 < m <= 2^23, with m/2 a product of two tuned "
           "single-pass lengths (2^a, 3 * 2^a, 5 * 2^a in [64, 2048], 81, 125; dfft_rconv1d_long_length); Bluestein halves are not built";
}

long long dfft_rconv1d_long_length(long long at_least) { return lconv_length(at_least); }

int dfft_rconv1d_long_split(long long m, int* n1, int* n2) {
    int a = 0, b = 0;
    if (!lconv_split(m, &a, &b)) return 0;
    if (n1) *n1 = a;
    if (n2) *n2 = b;
    return 1;
}

int dfft_rconv1d_long_fused_applies(long long m, int dtype) { return valid_dtype(dtype) && lconv_fused_env() && lconv_fused(m, dtype); }

unsigned long long dfft_rconv1d_long_scratch_bytes(long long n, long long m, long long channels, long long batch, int dtype) {
    if (!valid_dtype(dtype) || n < 1 || m < n || channels < 1 || batch < 1 || channels >= (1ll << 31) || batch >= (1ll << 31) ||
        batch * channels >= (1ll << 31))
        return 0;
    return lconv_scratch_bytes(m, dtype, batch * channels, chunk_cap_env());
}

int dfft_rconv1d_long_filter(const void* h, void* hp, long long m, long long channels, int dtype, int filter_kind, void* stream) {
    if (!h || !hp || m < 1 || channels < 1 || !valid_dtype(dtype) || (filter_kind != DFFT_FILTER_COMPLEX && filter_kind != DFFT_FILTER_REAL))
        return fail(DFFT_EINVAL, "dfft_rconv1d_long_filter: bad arguments");
    if (!lconv_split(m, nullptr, nullptr)) return fail(DFFT_EUNSUPPORTED, lconv_length_message("dfft_rconv1d_long_filter", m));
    const size_t    es = filter_kind == DFFT_FILTER_REAL ? elem_bytes(dtype) / 2 : elem_bytes(dtype);
    const uintptr_t bytes = (uintptr_t)channels * (m / 2 + 1) * es;
    if (ranges_overlap(h, bytes, hp, bytes)) return fail(DFFT_EINVAL, "dfft_rconv1d_long_filter: h and hp overlap (the permutation is out of place)");
    if (dfft_device_count() < 1) return fail(DFFT_ENOGPU, "dfft_rconv1d_long_filter: no HIP device visible (no CPU fallback)");
    return lconv_filter(h, hp, m, channels, (int)es, (hipStream_t)stream);
}

int dfft_rconv1d_long(void* in, void* out, const void* hp, long long n, long long m, long long channels, long long batch, int dtype, int filter_kind,
                      void* stream) {
    if (!in || !out || !hp || n < 1 || m < 1 || channels < 1 || batch < 1 || m < n || !valid_dtype(dtype) ||
        (filter_kind != DFFT_FILTER_COMPLEX && filter_kind != DFFT_FILTER_REAL))
        return fail(DFFT_EINVAL, "dfft_rconv1d_long: bad arguments");
    if (!lconv_split(m, nullptr, nullptr)) return fail(DFFT_EUNSUPPORTED, lconv_length_message("dfft_rconv1d_long", m));
    if (channels >= (1ll << 31) || batch >= (1ll << 31) || batch * channels >= (1ll << 31))
        return fail(DFFT_EUNSUPPORTED, "dfft_rconv1d_long: batch * channels = 2^31 or more rows: split the batch");
    const size_t    cs = elem_bytes(dtype), rs = cs / 2;
    const long long rows = batch * channels, nh = m / 2 + 1;
    const uintptr_t bytes = (uintptr_t)rows * n * rs;
    if (partly_overlap(in, out, bytes))
        return fail(DFFT_EINVAL, "dfft_rconv1d_long: in and out overlap partly (the convolution runs out of place or exactly in place)");
    if (ranges_overlap(hp, (uintptr_t)channels * nh * (filter_kind == DFFT_FILTER_REAL ? rs : cs), out, bytes))
        return fail(DFFT_EINVAL, "dfft_rconv1d_long: the filter overlaps out");
    if (dfft_device_count() < 1) return fail(DFFT_ENOGPU, "dfft_rconv1d_long: no HIP device visible (no CPU fallback)");
    const hipStream_t st = (hipStream_t)stream;
    const size_t      cap = chunk_cap_env();
    ScratchLease      lease;
    if (lconv_fused_env() && lconv_fused(m, dtype)) {
        LconvLaunch L;
        std::memset(&L, 0, sizeof(L));
        L.dtype = dtype;
        L.filter_kind = filter_kind;
        L.n = n;
        L.m = m;
        L.channels = channels;
        L.batch = batch;
        L.in = in;
        L.out = out;
        L.hp = hp;
        const size_t need = lconv_scratch_bytes(m, dtype, rows, cap);
        if (!lease.acquire(need, st)) return fail(DFFT_EHIP, "dfft_rconv1d_long: cannot allocate the scratch buffer");
        return lconv_run(L, cap, lease.get(), need, st);
    }
    // composed route, per chunk of whole row pairs of at most max(256 MiB, one pair's) bins and padded rows: pad, the real rows of length m as
    // dfft_rfft1d runs them, multiply by H / m, the inverse rows, truncate -- on ONE lease (bins, padded rows, the transforms' own scratch)
    const size_t    rb = (size_t)nh * cs + (size_t)m * rs;
    const long long nr = long_composed_chunk_rows(rb, rows, cap);
    RealRowsPass    Rf, Rb;
    if (int rc = real_rows_prepare(m, nr, dtype, DFFT_FORWARD, false, cap, &Rf)) return rc;
    if (int rc = real_rows_prepare(m, nr, dtype, DFFT_BACKWARD, true, cap, &Rb)) return rc;
    const size_t data_b = ((size_t)nr * rb + 255) / 256 * 256;
    if (!lease.acquire(data_b + std::max(Rf.need, Rb.need), st)) return fail(DFFT_EHIP, "dfft_rconv1d_long: cannot allocate the scratch buffer");
    char* bins = (char*)lease.get();          // [nr][nh] complex
    char* pad = bins + (size_t)nr * nh * cs;  // [nr][m] reals
    void* inner = bins + data_b;
    for (long long r0 = 0; r0 < rows; r0 += nr) {
        const long long k = std::min(nr, rows - r0);
        if (int rc = pad_rows((const char*)in + (size_t)r0 * n * rs, pad, n, m, k, dtype, st)) return rc;
        if (int rc = real_rows_run(Rf, pad, bins, k, inner, st)) return rc;
        if (int rc = lconv_mul(bins, hp, m, r0, channels, k, dtype, filter_kind, st)) return rc;
        if (int rc = real_rows_run(Rb, bins, pad, k, inner, st)) return rc;
        if (int rc = trunc_rows(pad, (char*)out + (size_t)r0 * n * rs, n, m, k, dtype, st)) return rc;
    }
    return DFFT_OK;
}

// Long 1-D real cross-spectrum (dfft_lxspec.hip): dfft_rxspec1d at the padded lengths of dfft_rconv1d_long
static bool lxspec_rows_ok(long long channels, long long batch) {
    return channels < (1ll << 31) && batch < (1ll << 31) && batch * channels < (1ll << 31);
}

int dfft_rxspec1d_long_fused_applies(long long m, int dtype) { return valid_dtype(dtype) && lxspec_fused_env() && lxspec_fused(m, dtype); }

long long dfft_rxspec1d_long_slices(long long m, long long channels, long long batch, int dtype) {
    if (!valid_dtype(dtype) || m < 1 || channels < 1 || batch < 1 || !lxspec_rows_ok(channels, batch) || !lconv_split(m, nullptr, nullptr)) return 0;
    return lxspec_slices(m, channels, lxspec_chunk_rows(m, dtype, batch * channels, chunk_cap_env()));
}

unsigned long long dfft_rxspec1d_long_scratch_bytes(long long n, long long m, long long channels, long long batch, int dtype) {
    if (!valid_dtype(dtype) || n < 1 || m < n || channels < 1 || batch < 1 || !lxspec_rows_ok(channels, batch)) return 0;
    return lxspec_scratch_bytes(m, dtype, channels, batch * channels, chunk_cap_env());
}

int dfft_rxspec1d_long(const void* x, const void* g, void* out, long long n, long long m, long long channels, long long batch, int dtype, int order,
                       void* stream) {
    if (!x || !g || !out || n < 1 || m < 1 || channels < 1 || batch < 1 || m < n || !valid_dtype(dtype) || (order != 0 && order != 1))
        return fail(DFFT_EINVAL, "dfft_rxspec1d_long: bad arguments");
    if (!lconv_split(m, nullptr, nullptr)) return fail(DFFT_EUNSUPPORTED, lconv_length_message("dfft_rxspec1d_long", m));
    if (!lxspec_rows_ok(channels, batch)) return fail(DFFT_EUNSUPPORTED, "dfft_rxspec1d_long: batch * channels = 2^31 or more rows: split the batch");
    const size_t    cs = elem_bytes(dtype), rs = cs / 2;
    const long long rows = batch * channels, nh = m / 2 + 1;
    const uintptr_t ibytes = (uintptr_t)rows * n * rs, obytes = (uintptr_t)channels * nh * cs;
    if (ranges_overlap(x, ibytes, out, obytes) || ranges_overlap(g, ibytes, out, obytes))
        return fail(DFFT_EINVAL, "dfft_rxspec1d_long: out overlaps x or g");
    if (dfft_device_count() < 1) return fail(DFFT_ENOGPU, "dfft_rxspec1d_long: no HIP device visible (no CPU fallback)");
    const hipStream_t st = (hipStream_t)stream;
    const size_t      cap = chunk_cap_env();
    ScratchLease      lease;
    if (lxspec_fused_env() && lxspec_fused(m, dtype)) {
        LxspecLaunch L;
        std::memset(&L, 0, sizeof(L));
        L.dtype = dtype;
        L.order = order;
        L.n = n;
        L.m = m;
        L.channels = channels;
        L.batch = batch;
        L.x = x;
        L.g = g;
        L.out = out;
        const size_t need = lxspec_scratch_bytes(m, dtype, channels, rows, cap);
        if (!lease.acquire(need, st)) return fail(DFFT_EHIP, "dfft_rxspec1d_long: cannot allocate the scratch buffer");
        return lxspec_run(L, cap, lease.get(), need, st);
    }
    // composed route, per chunk of whole row pairs of at most max(256 MiB, one pair's) bins of both fields and padded rows: pad, the real rows of
    // length m as dfft_rfft1d runs them, on both fields, and the kernel that adds each channel's rows to out in row order -- on ONE lease
    const bool      autos = x == g;
    const size_t    rb = 2 * (size_t)nh * cs + (size_t)m * rs;
    const long long nr = long_composed_chunk_rows(rb, rows, cap);
    RealRowsPass    Rf;
    if (int rc = real_rows_prepare(m, nr, dtype, DFFT_FORWARD, false, cap, &Rf)) return rc;
    const size_t data_b = ((size_t)nr * rb + 255) / 256 * 256;
    if (!lease.acquire(data_b + Rf.need, st)) return fail(DFFT_EHIP, "dfft_rxspec1d_long: cannot allocate the scratch buffer");
    char* xb = (char*)lease.get();           // [nr][nh] complex
    char* gb = xb + (size_t)nr * nh * cs;    // [nr][nh] complex
    char* pad = gb + (size_t)nr * nh * cs;   // [nr][m] reals, shared by the two fields
    void* inner = xb + data_b;
    for (long long r0 = 0; r0 < rows; r0 += nr) {
        const long long k = std::min(nr, rows - r0);
        if (int rc = pad_rows((const char*)x + (size_t)r0 * n * rs, pad, n, m, k, dtype, st)) return rc;
        if (int rc = real_rows_run(Rf, pad, xb, k, inner, st)) return rc;
        if (!autos) {
            if (int rc = pad_rows((const char*)g + (size_t)r0 * n * rs, pad, n, m, k, dtype, st)) return rc;
            if (int rc = real_rows_run(Rf, pad, gb, k, inner, st)) return rc;
        }
        if (int rc = lxspec_mac(xb, autos ? xb : gb, out, m, r0, k, channels, dtype, order, st)) return rc;
    }
    return DFFT_OK;
}

// `batch` planes of [n1][n2] reals <-> [n1][n2/2 + 1] bins, in groups of planes sized for the 256 MiB Infinity Cache (dfft_fft2d_batch's
// rule, on the complex side): forward R2C rows into `out`, then the n1-point columns in place on `out` (dfft_fft1d_any); backward the
// inverse columns from `in` into a scratch group, then C2R rows from there into `out`.
int dfft_rfft2d_batch(void* in, void* out, long long n1, long long n2, long long batch, int dtype, int direction, void* stream) {
    if (!in || !out || n1 < 1 || n2 < 1 || batch < 0 || !valid_dtype(dtype) || !valid_direction(direction))
        return fail(DFFT_EINVAL, "dfft_rfft2d_batch: bad arguments");
    if (real_form(n2) == 0) return fail(DFFT_EUNSUPPORTED, "dfft_rfft2d_batch: n2 = " + std::to_string(n2) + " has no real form");
    if (length_kind(n1) == 0) return fail(DFFT_EUNSUPPORTED, "dfft_rfft2d_batch: n1 = " + std::to_string(n1) + " is outside every form");
    const bool      fwd = direction == DFFT_FORWARD;
    const size_t    cs = elem_bytes(dtype), rs = cs / 2;
    const long long nh = n2 / 2 + 1;
    const uintptr_t rplane_b = (uintptr_t)n1 * n2 * rs, cplane_b = (uintptr_t)n1 * nh * cs;
    if (ranges_overlap(in, (uintptr_t)batch * (fwd ? rplane_b : cplane_b), out, (uintptr_t)batch * (fwd ? cplane_b : rplane_b)))
        return fail(DFFT_EINVAL, "dfft_rfft2d_batch: in and out overlap (the transform is out of place)");
    if (dfft_device_count() < 1) return fail(DFFT_ENOGPU, "dfft_rfft2d_batch: no HIP device visible (no CPU fallback)");
    if (batch == 0) return DFFT_OK;
    const hipStream_t st = (hipStream_t)stream;
    const long long   cp = cache_plane_group(batch, (long long)cplane_b);  // planes per group
    const size_t      cap = chunk_cap_env();
    RealRowsPass      R;
    if (int rc = real_rows_prepare(n2, cp * n1, dtype, direction, !fwd, cap, &R)) return rc;
    if (fwd) {
        for (long long p0 = 0; p0 < batch; p0 += cp) {
            const long long  np = std::min(cp, batch - p0);
            void*            op = (char*)out + p0 * cplane_b;
            {  // the lease goes back before dfft_fft1d_any takes its own
                ScratchLease lease;
                if (R.need && !lease.acquire(R.need, st)) return fail(DFFT_EHIP, "dfft_rfft2d_batch: cannot allocate the scratch buffer");
                DFFT_TRY(real_rows_run(R, (const char*)in + p0 * rplane_b, op, np * n1, lease.get(), st));
            }
            if (int rc2 = dfft_fft1d_any(op, op, n1, nh, np, dtype, direction, stream)) return rc2;
        }
        return DFFT_OK;
    }
    AnyPass A;
    if (int rc = any_prepare(n1, nh, cp, dtype, direction, cap, &A)) return rc;
    const size_t     gb = (size_t)cp * cplane_b;  // the bins of one plane group
    const size_t     inner = std::max(R.need, A.need);
    ScratchLease lease;  // ONE lease across the loop, sized for both steps of a group (the lease is not re-entrant)
    if (!lease.acquire(gb + inner, st)) return fail(DFFT_EHIP, "dfft_rfft2d_batch: cannot allocate the scratch buffer");
    void* const scr = lease.get();
    void*       iscr = inner ? (char*)scr + gb : nullptr;
    int   rc = DFFT_OK;
    for (long long p0 = 0; p0 < batch && rc == DFFT_OK; p0 += cp) {
        const long long np = std::min(cp, batch - p0);
        rc = any_run(A, (const char*)in + p0 * cplane_b, scr, np, iscr, st);
        if (rc == DFFT_OK) rc = real_rows_run(R, scr, (char*)out + p0 * rplane_b, np * n1, iscr, st);
    }
    return rc;
}

int dfft_fft1d_cols(void* in, void* out, long long n, long long width, long long batch, int dtype, int direction,
                    void* stream) {
    if (!in || !out || batch < 0 || width < 1 || !valid_dtype(dtype) || !valid_direction(direction))
        return fail(DFFT_EINVAL, "dfft_fft1d_cols: bad arguments");
    if (!dfft_length_supported(n)) return fail(DFFT_EUNSUPPORTED, "dfft_fft1d_cols: unsupported length");
    if (partly_overlap(in, out, (uintptr_t)batch * (uintptr_t)n * (uintptr_t)width * elem_bytes(dtype)))
        return fail(DFFT_EINVAL, "dfft_fft1d_cols: in and out overlap partly (the transform runs out of place or exactly in place)");
    if (!cols_extent_ok(n, width, dtype, aligned16(in), aligned16(out))) return fail(DFFT_EUNSUPPORTED, extent_message("dfft_fft1d_cols", n, width));
    if (dfft_device_count() < 1) return fail(DFFT_ENOGPU, "dfft_fft1d_cols: no HIP device visible (no CPU fallback)");
    if (n > 4096) {
        if (batch == 0) return DFFT_OK;
        ScratchLease lease;
        if (!lease.acquire((size_t)batch * n * width * elem_bytes(dtype), (hipStream_t)stream))
            return fail(DFFT_EHIP, "dfft_fft1d_cols: cannot allocate the scratch buffer of the four-step transform");
        return long_fft(in, out, n, width, batch, dtype, direction, 1.0, lease.get(), (hipStream_t)stream);
    }
    const void* tw = nullptr;
    int         rc = get_twiddles((int)n, dtype, &tw);
    if (rc) return rc;
    FftLaunch L;
    std::memset(&L, 0, sizeof(L));
    L.dtype = dtype;
    L.n = (int)n;
    L.dir = direction;
    L.cols = 1;
    L.in = in;
    L.out = out;
    L.tw = tw;
    L.imap = L.omap = plain_axis(n, width, 1);
    L.itile = L.otile = TileMap{n * width, 1};
    L.na = batch;
    L.ncols = (int)width;
    return check_launch(launch_fft(L, (hipStream_t)stream), "dfft_fft1d_cols");
}

}  // extern "C"
