// dfft_core.cpp -- what needs no plan and launches nothing: the last-error state, the twiddle cache, the length and extent rules and
// the query-only entry points of the C-ABI (include/dfft.h).
//
// Reference being replaced (behaviour, not code): /root/reference/3dmpifft_opt/include/fft_mpi_3d_api.cpp
//   getProperDeviceNum :232-272, getDataCountForNode :274-287, getMaxDataCount :289-316.
#include <cmath>
#include <map>
#include <mutex>

#include "dfft_plan_impl.h"
#include "dfft_r2r.h"
#include "dfft_osconv.h"
#include "dfft_rconv.h"
#include "dfft_real.h"
#include "dfft_real_cols.h"

namespace dfft {

static thread_local std::string g_last_error;
void set_error(const std::string& msg) { g_last_error = msg; }
int  fail(int code, const std::string& msg) {
    g_last_error = msg;
    trace_on_error(code, msg);  // communication failures print the process's last control-plane events (dfft_trace.cpp)
    return code;
}
const std::string& last_error() { return g_last_error; }

// ---------------------------------------------------------------------------------------------------------------
// twiddle tables
struct TwKey {
    int  dev, n, dtype;
    bool operator<(const TwKey& o) const {
        if (dev != o.dev) return dev < o.dev;
        if (n != o.n) return n < o.n;
        return dtype < o.dtype;
    }
};
static std::mutex               g_tw_mutex;
static std::map<TwKey, void*>   g_tw_cache;

int get_twiddles(int n, int dtype, const void** table) {
    int dev = 0;
    DFFT_HIP_TRY(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lk(g_tw_mutex);
    TwKey key{dev, n, dtype};
    auto it = g_tw_cache.find(key);
    if (it != g_tw_cache.end()) {
        *table = it->second;
        return DFFT_OK;
    }
    // e^{-2 pi i k / n} evaluated in extended precision and rounded once (the reference builds its LUT with host
    // double cos/sin, templateFFT.cpp:5120-5141).
    const long double two_pi = 6.283185307179586476925286766559005768L;
    void*             dptr = nullptr;
    if (dtype == DFFT_F64) {
        std::vector<double> h(2 * (size_t)n);
        for (int k = 0; k < n; ++k) {
            const long double a = two_pi * (long double)k / (long double)n;
            h[2 * k] = (double)cosl(a);
            h[2 * k + 1] = (double)(-sinl(a));
        }
        DFFT_HIP_TRY(hipMalloc(&dptr, h.size() * sizeof(double)));
        DFFT_HIP_TRY(hipMemcpy(dptr, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice));
    } else {
        std::vector<float> h(2 * (size_t)n);
        for (int k = 0; k < n; ++k) {
            const long double a = two_pi * (long double)k / (long double)n;
            h[2 * k] = (float)cosl(a);
            h[2 * k + 1] = (float)(-sinl(a));
        }
        DFFT_HIP_TRY(hipMalloc(&dptr, h.size() * sizeof(float)));
        DFFT_HIP_TRY(hipMemcpy(dptr, h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice));
    }
    g_tw_cache[key] = dptr;
    *table = dptr;
    return DFFT_OK;
}

int length_kind(long long n) {
    if (n >= 1 && n <= 4096 && fft_length_supported((int)n)) return 1;
    if (n < 1 || n >= (1ll << 30)) return 0;
    int a, b;
    if (long_split(n, &a, &b)) return 2;
    return n <= kBluesteinMaxLength ? 3 : 0;
}

int real_form(long long n) {
    if (real_length_supported(n)) return 1;
    const int k = length_kind(n);
    return k == 1 ? 2 : (k == 0 ? 0 : 3);
}

// ---- supported extent of the plan-less column transforms (include/dfft.h, "Supported extent") ------------------------------------------------
// The tuned column kernels keep a thread's offsets inside one [n][width] matrix in 32 bits, in units of one V (cols_offsets_fit32,
// dfft_kernels.h): 16 bytes for fp64 and for fp32 column pairs (even width, both pointers 16-byte aligned), 8 bytes for scalar fp32.
// Every route that ends in those kernels is judged here, before the device is queried and before any scratch is leased.
// DFFT_NO_PAIRS (make_pair_launch's measurement switch): fp32 columns on the scalar kernels whatever their width
static bool pairs_disabled_env() {
    const char* e = getenv("DFFT_NO_PAIRS");
    return e && *e && *e != '0';
}
bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0 && !pairs_disabled_env(); }
bool scratch16() { return !pairs_disabled_env(); }
// one launch of the tuned n-point column kernels on [n][width]
static bool tuned_cols_ok(long long n, long long width, int dtype, bool pairs) {
    if (width + kTileColsMax > (1ll << 31)) return false;  // column indices are ints, a ragged last tile counts up to one tile further
    const bool paired = dtype == DFFT_F32 && pairs && width % 2 == 0;
    return cols_offsets_fit32(n, paired ? width / 2 : width);
}
// long_fft on [n][s], n = N1 * N2: pass A runs N1-point columns of width N2 * s from `in` into the scratch, pass B N2-point columns of
// width s in place on the scratch (s = 1: rows)
static bool four_step_ok(long long n, long long s, int dtype, bool in16) {
    int N1 = 0, N2 = 0;
    if (!long_split(n, &N1, &N2)) return false;
    return tuned_cols_ok(N1, (long long)N2 * s, dtype, in16 && scratch16()) && (s == 1 || tuned_cols_ok(N2, s, dtype, scratch16()));
}
// dfft_fft1d_cols on [n][width], kinds 1 and 2
bool cols_extent_ok(long long n, long long width, int dtype, bool in16, bool out16) {
    if (width + kTileColsMax > (1ll << 31)) return false;
    if (n > 4096) return four_step_ok(n, width, dtype, in16);
    return !fft_length_tuned((int)n) || tuned_cols_ok(n, width, dtype, in16 && out16);  // run-time-scheduled kernel: 64-bit offsets
}
// bluestein_fft on [n][s]: one launch, or pad -> M-point transforms in place on the scratch -> finish.  (The pad buffer of a chunk and,
// M > 4096, long_fft's scratch behind it are 16-byte aligned for fp32 only where M * s is even.)
bool bluestein_extent_ok(long long n, long long s, int dtype) {
    if (s == 1 || bluestein_runs_fused(n, s, bluestein_fused_env())) return true;
    const long long M = bluestein_padded_length(n);
    if (M <= 4096) return tuned_cols_ok(M, s, dtype, scratch16());
    return four_step_ok(M, s, dtype, scratch16() && (M * s) % 2 == 0);
}
// n-point transforms along the middle axis of [batch][n][s] (dfft_fft1d_any, and the inner transforms of the real and r2r composed routes)
bool any_extent_ok(long long n, long long s, int dtype, bool in16, bool out16) {
    if (s == 1) return true;  // rows: tile bases only
    return length_kind(n) == 3 ? (s + kTileColsMax <= (1ll << 31) && bluestein_extent_ok(n, s, dtype)) : cols_extent_ok(n, s, dtype, in16, out16);
}
std::string extent_message(const char* fn, long long n, long long s) {
    return std::string(fn) + ": n = " + std::to_string(n) + ", width = " + std::to_string(s) +
           ": a column pass would span 2^32 or more 16-byte (fp32, odd width or unaligned: 8-byte) units, or width > 2^31 - 64";
}

}  // namespace dfft

using namespace dfft;

extern "C" {

const char* dfft_version(void) { return "dfft-mi355x 0.1 (gfx950)"; }
const char* dfft_last_error(void) { return g_last_error.c_str(); }

int dfft_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int dfft_device_pci_bus_id(int device, char* buf, int len) {
    if (!buf || len < 16) return fail(DFFT_EINVAL, "dfft_device_pci_bus_id: buffer too small");
    if (device < 0) DFFT_HIP_TRY(hipGetDevice(&device));
    DFFT_HIP_TRY(hipDeviceGetPCIBusId(buf, len, device));
    return DFFT_OK;
}

int dfft_length_supported(long long n) {
    if (n <= 0 || n >= (1ll << 30)) return 0;
    if (fft_length_supported((int)n)) return 1;
    int a, b;
    return long_split(n, &a, &b) ? 1 : 0;  // two-pass (four-step) plans above 4096
}

int dfft_length_kind(long long n) { return length_kind(n); }
int dfft_real_form(long long n) { return real_form(n); }

long long dfft_bluestein_length(long long n) { return length_kind(n) == 3 ? bluestein_padded_length(n) : 0; }

// Route predicates of the plan-less entry points (read-only; the environment switches are read as a call would read them)
int dfft_bluestein_fused_applies(long long n, long long s) { return length_kind(n) == 3 && s >= 1 && bluestein_runs_fused(n, s, bluestein_fused_env()); }
int dfft_rfft_cols_fused_applies(long long n, long long s, int dtype) { return valid_dtype(dtype) && s > 1 && real_cols_fused(n, s, dtype); }
int dfft_r2r_fused_applies(long long n, long long s, int dtype, int kind, int vec) {
    if (!valid_dtype(dtype) || kind < DFFT_R2R_DCT2 || kind > DFFT_R2R_DST3 || n < 1 || s < 1) return 0;
    return r2r_fused_env() && r2r_fused(n, s, dtype, kind, vec != 0);
}
int dfft_rconv1d_fused_applies(long long n, long long m, int dtype, int filter_kind, int vec) {
    if (!valid_dtype(dtype)) return 0;
    return rconv_fused_env() && rconv_fused(n, m, dtype, filter_kind, vec != 0);
}
long long dfft_rconv1d_length(long long at_least) { return rconv_length(at_least); }
int dfft_rconv1d_os_fused_applies(long long m, int dtype) { return valid_dtype(dtype) && rconv_fused_env() && osconv_fused(m, dtype); }
int dfft_rconv1d_os_block(long long taps, long long n_out, int dtype, long long* m, long long* discard) {
    if (!m || !discard || taps < 1 || n_out < 1 || !valid_dtype(dtype)) return fail(DFFT_EINVAL, "dfft_rconv1d_os_block: bad arguments");
    if (!osconv_block(taps, n_out, dtype, m, discard))
        return fail(DFFT_EUNSUPPORTED, "dfft_rconv1d_os_block: taps = " + std::to_string(taps) + " -- no block length leaves room for more than 8191 taps "
                                       "(four-step and Bluestein halves are not built)");
    return DFFT_OK;
}
int dfft_conv_fused_applies(int dtype, long long n0, long long rows, long long ncols, long long plane, long long pitch, int rot, const void* in,
                            const void* out) {
    if (!valid_dtype(dtype) || n0 < 1 || n0 > 4096 || rows < 1 || ncols < 1 || plane < 1 || pitch < 1 || rot < 0) return 0;
    ConvLaunch L;
    std::memset(&L, 0, sizeof(L));
    L.dtype = dtype;
    L.n0 = (int)n0;
    L.rows = rows;
    L.ncols = ncols;
    L.plane = plane;
    L.pitch = pitch;
    L.rot = rot;
    L.in = in;
    L.out = const_cast<void*>(out);
    return conv_fused_applies(L) ? 1 : 0;
}

// The extent rule of dfft_fft1d_cols (include/dfft.h; any_extent_ok above).  `pairs`: both pointers are 16-byte aligned.
int dfft_cols_extent_supported(long long n, long long width, int dtype, int pairs) {
    if (n < 1 || width < 1 || !valid_dtype(dtype) || length_kind(n) == 0 || length_kind(n) == 3) return 0;
    return cols_extent_ok(n, width, dtype, pairs != 0, pairs != 0) ? 1 : 0;
}
// The ticket base of a plan's X pass (dfft_plan_impl.h, x_ticket) after `launches` launches, stepped exactly as launch_variant steps it.
// Not part of the C-ABI of include/dfft.h: exported for tests/test_x_ticket_host.py only, which binds it itself.
unsigned dfft_x_ticket_base_after(unsigned base, long long ntiles, long long grid, long long launches) {
    for (long long g = 0; g < launches; ++g) base += x_ticket_count((unsigned)ntiles, (unsigned)grid);
    return base;
}
// The same for dfft_fft1d_any along the middle axis of [batch][n][s], every kind of length; in16 / out16: that pointer is 16-byte aligned.
int dfft_fft1d_any_extent_supported(long long n, long long s, int dtype, int in16, int out16) {
    if (n < 1 || s < 1 || !valid_dtype(dtype) || length_kind(n) == 0) return 0;
    return any_extent_ok(n, s, dtype, in16 != 0, out16 != 0) ? 1 : 0;
}

// Scratch bytes a plan-less call leases from the per-(device, stream) buffer (0: none), by the routines' own rules and without a device:
// the sizes depend on a Bluestein length's n, M and dtype only, so tables without device arrays stand in for the cached ones.
static void scratch_tables(BluesteinTables* T, long long n, int dtype, int dir) {
    T->n = n;
    T->M = bluestein_padded_length(n);
    T->dtype = dtype;
    T->dir = dir;
}
unsigned long long dfft_fft1d_any_scratch_bytes(long long n, long long s, long long batch, int dtype) {
    const int kind = length_kind(n);
    if (!valid_dtype(dtype) || s < 1 || batch < 1 || kind < 2) return 0;
    if (kind == 2) return (unsigned long long)batch * n * s * elem_bytes(dtype);
    if (!bluestein_extent_ok(n, s, dtype)) return 0;  // refused before any lease
    BluesteinTables T;
    scratch_tables(&T, n, dtype, DFFT_FORWARD);
    return bluestein_scratch_bytes(T, s, batch, bluestein_fused_env(), chunk_cap_env());
}
unsigned long long dfft_rfft1d_strided_scratch_bytes(long long n, long long s, long long batch, int dtype) {
    const int kind = length_kind(n);
    if (!valid_dtype(dtype) || s < 2 || batch < 1 || kind == 0) return 0;
    BluesteinTables T;
    scratch_tables(&T, n, dtype, DFFT_FORWARD);
    return real_cols_scratch_bytes(n, s, batch, dtype, kind == 3 ? &T : nullptr, bluestein_fused_env(), chunk_cap_env());
}
unsigned long long dfft_r2r1d_strided_scratch_bytes(long long n, long long s, long long batch, int dtype, int kind, int vec) {
    const int lk = length_kind(n);
    if (!valid_dtype(dtype) || kind < DFFT_R2R_DCT2 || kind > DFFT_R2R_DST3 || s < 1 || batch < 1 || lk == 0) return 0;
    BluesteinTables T;
    scratch_tables(&T, n, dtype, DFFT_FORWARD);
    R2rLaunch L;
    std::memset(&L, 0, sizeof(L));
    L.dtype = dtype;
    L.kind = kind;
    L.n = n;
    L.s = s;
    L.batch = batch;
    L.in = L.out = (void*)(uintptr_t)(vec ? 64 : elem_bytes(dtype) / 2);  // r2r_vec looks at the alignment only
    return r2r_scratch_bytes(L, r2r_fused_env(), lk == 3 ? &T : nullptr, bluestein_fused_env(), chunk_cap_env());
}

unsigned long long dfft_rconv1d_scratch_bytes(long long n, long long m, long long channels, long long batch, int dtype) {
    if (!valid_dtype(dtype) || n < 1 || m < n || channels < 1 || batch < 1 || channels >= (1ll << 31) || batch >= (1ll << 31) ||
        batch * channels >= (1ll << 31) || real_form(m) != 1)
        return 0;
    RconvLaunch L;
    std::memset(&L, 0, sizeof(L));
    L.dtype = dtype;
    L.n = n;
    L.m = m;
    L.channels = channels;
    L.batch = batch;
    return rconv_scratch_bytes(L, rconv_fused_env(), chunk_cap_env());  // (the route depends on neither the filter kind nor the alignment)
}

unsigned long long dfft_rconv1d_os_scratch_bytes(long long n_out, long long m, long long discard, long long channels, long long batch, int dtype) {
    if (!valid_dtype(dtype) || n_out < 1 || discard < 0 || m <= discard || real_form(m) != 1) return 0;
    OsconvLaunch L;
    std::memset(&L, 0, sizeof(L));
    L.dtype = dtype;
    L.n = n_out;  // the lease does not depend on n: any n the entry point accepts with this n_out
    L.n_out = n_out;
    L.m = m;
    L.discard = discard;
    L.channels = channels;
    L.batch = batch;
    return osconv_scratch_bytes(L, rconv_fused_env(), chunk_cap_env());  // (0 for refused sizes; the route depends on neither the filter kind nor the alignment)
}

int dfft_proper_device_count(const long long N[3], int ini_devices_in_rank, int nranks, int rank, int real_devices,
                             int* new_total, int* new_in_rank) {
    if (!N || !new_total || !new_in_rank || nranks < 1 || rank < 0 || rank >= nranks || ini_devices_in_rank < 1)
        return fail(DFFT_EINVAL, "dfft_proper_device_count: bad arguments");
    int ini = ini_devices_in_rank;
    if (real_devices >= 0 && ini > real_devices) ini = real_devices;  // fft_mpi_3d_api.cpp:236-239
    if (ini < 1) return fail(DFFT_ENOGPU, "dfft_proper_device_count: no device available");
    int total = ini * nranks, in_rank = ini;
    if (N[0] % total != 0) {  // :244-259
        const long long per = N[0] / total + 1;
        total = (int)(N[0] / per);
        if (N[0] % per != 0) total += 1;
        in_rank = total / nranks;
        const int rem = total % nranks;
        if (rem != 0 && rank < rem) in_rank += 1;
    }
    *new_total = total;
    *new_in_rank = in_rank;
    if (in_rank == 0) return fail(DFFT_EINVAL, "could not support this distribution of data");  // :266-269
    return DFFT_OK;
}

long long dfft_local_count(const long long N[3], int total_devices, int global_idx) {
    if (!N || total_devices < 1 || global_idx < 0 || global_idx >= total_devices) return -1;
    const Slab sx = make_slab(N[0], total_devices);
    return sx.size(global_idx) * N[1] * N[2];
}

long long dfft_max_count(long long n0, long long n1, long long n2, int total_devices, int is_last_device) {
    if (total_devices < 1) return -1;
    const Slab      sx = make_slab(n0, total_devices), sy = make_slab(n1, total_devices);
    const int       g = is_last_device ? total_devices - 1 : 0;
    const long long a = sx.size(g) * n1 * n2, b = n0 * sy.size(g) * n2;
    return a > b ? a : b;
}

int dfft_local_size(long long n0, long long n1, long long n2, int total_devices, int global_idx, long long* local_n0,
                    long long* local_0_start, long long* local_n1, long long* local_1_start) {
    (void)n2;
    if (total_devices < 1 || global_idx < 0 || global_idx >= total_devices)
        return fail(DFFT_EINVAL, "dfft_local_size: bad arguments");
    const Slab sx = make_slab(n0, total_devices), sy = make_slab(n1, total_devices);
    if (local_n0) *local_n0 = sx.size(global_idx);
    if (local_0_start) *local_0_start = sx.start(global_idx);
    if (local_n1) *local_n1 = sy.size(global_idx);
    if (local_1_start) *local_1_start = sy.start(global_idx);
    return DFFT_OK;
}

// the exchange of device `global_idx` of a fp64 plan of this shape, as a plan would fill it in; fn: the caller, for the message
static int layout_exchange(const char* fn, long long n0, long long n1, long long n2, int total_devices, int global_idx, int direction, ExchangeDesc* x) {
    const long long shape[3] = {n0, n1, n2};
    const std::unique_ptr<dfft_plan_s> tmp(plan_new(shape, DFFT_F64, direction, total_devices, global_idx, nullptr, 0));
    if (tmp->sx.size(total_devices - 1) < 1 || tmp->sy.size(total_devices - 1) < 1) return fail(DFFT_EINVAL, std::string(fn) + ": last slab would be empty");
    fill_exchange(tmp.get(), *x, direction);
    return DFFT_OK;
}

int dfft_exchange_layout(long long n0, long long n1, long long n2, int total_devices, int global_idx, int direction,
                         long long* scount, long long* soffset, long long* rcount, long long* roffset) {
    if (total_devices < 1 || global_idx < 0 || global_idx >= total_devices || !valid_direction(direction))
        return fail(DFFT_EINVAL, "dfft_exchange_layout: bad arguments");
    ExchangeDesc xd;
    DFFT_TRY(layout_exchange("dfft_exchange_layout", n0, n1, n2, total_devices, global_idx, direction, &xd));
    for (int q = 0; q < total_devices; ++q) {
        if (scount) scount[q] = xd.scount[q];
        if (soffset) soffset[q] = xd.soffset[q];
        if (rcount) rcount[q] = xd.rcount[q];
        if (roffset) roffset[q] = xd.roffset[q];
    }
    return DFFT_OK;
}

int dfft_exchange_part_layout(long long n0, long long n1, long long n2, int total_devices, int global_idx, int direction,
                              long long part_planes, int part, int ycuts, int ycut, int max_msgs, int* peer,
                              long long* soffset, long long* scount, long long* roffset, long long* rcount) {
    if (total_devices < 1 || global_idx < 0 || global_idx >= total_devices || part_planes < 1 || part < 0 || ycuts < 1 ||
        ycut >= ycuts || max_msgs < 0 || !valid_direction(direction))
        return fail(DFFT_EINVAL, "dfft_exchange_part_layout: bad arguments");
    if (ycuts > 1 && (n0 % total_devices != 0 || n1 % total_devices != 0 || (n1 / total_devices) % ycuts != 0))
        return fail(DFFT_EINVAL, "dfft_exchange_part_layout: Y sub-blocks need even X and Y splits divisible by ycuts");
    ExchangeDesc xd;
    DFFT_TRY(layout_exchange("dfft_exchange_part_layout", n0, n1, n2, total_devices, global_idx, direction, &xd));
    xd.ycuts = ycuts;
    std::vector<int>       pe;
    std::vector<long long> so, sc, ro, rc;
    comm_part_messages(xd, part, part_planes, ycut, pe, so, sc, ro, rc);
    const int n = (int)pe.size();
    if (n > max_msgs) return fail(DFFT_EINVAL, "dfft_exchange_part_layout: more messages than max_msgs");
    for (int i = 0; i < n; ++i) {
        if (peer) peer[i] = pe[i];
        if (soffset) soffset[i] = so[i];
        if (scount) scount[i] = sc[i];
        if (roffset) roffset[i] = ro[i];
        if (rcount) rcount[i] = rc[i];
    }
    return n;
}

int dfft_r2c_counts(long long n0, long long n1, long long n2, int total_devices, int global_idx, long long* real_count, long long* complex_count) {
    if (n0 < 1 || n1 < 1 || n2 < 2 || total_devices < 1 || global_idx < 0 || global_idx >= total_devices)
        return fail(DFFT_EINVAL, "dfft_r2c_counts: bad arguments");
    const Slab      sx = make_slab(n0, total_devices), sy = make_slab(n1, total_devices);
    const long long nh = n2 / 2 + 1, xs = sx.size(global_idx), ys = sy.size(global_idx);
    if (xs < 0 || sy.size(total_devices - 1) < 1 || sx.size(total_devices - 1) < 1)
        return fail(DFFT_EINVAL, "dfft_r2c_counts: slab decomposition leaves the last device empty");
    // complex side: the transposed result [ys][nh][N0], and -- forward plans with an exchange -- the packed send layout [d][xs][yl_d][nh]
    // the Y pass writes into the same buffer (the offsets of dfft_exchange_layout at width nh)
    const long long send = (long long)(total_devices - 1) * xs * sy.blk * nh + xs * sy.size(total_devices - 1) * nh;
    if (real_count) *real_count = xs * n1 * n2;
    if (complex_count) *complex_count = std::max(ys * nh * n0, total_devices > 1 ? send : 0ll);
    return DFFT_OK;
}

long long dfft_conv_filter_count(long long n0, long long n1, long long n2, int total_devices, int global_idx) {
    if (n0 < 1 || n1 < 1 || n2 < 1 || total_devices < 1 || global_idx < 0 || global_idx >= total_devices) return -1;
    return make_slab(n1, total_devices).size(global_idx) * n2 * n0;
}

long long dfft_conv_real_filter_count(long long n0, long long n1, long long n2, int total_devices, int global_idx) {
    if (n0 < 1 || n1 < 1 || n2 < 1 || total_devices < 1 || global_idx < 0 || global_idx >= total_devices) return -1;
    return make_slab(n1, total_devices).size(global_idx) * (n2 / 2 + 1) * n0;
}

void* dfft_alloc(long long count, int dtype, int flag) {
    if (count < 0 || !valid_dtype(dtype)) {
        set_error("dfft_alloc: bad arguments");
        return nullptr;
    }
    const size_t bytes = (size_t)count * elem_bytes(dtype);
    void*        p = nullptr;
    if (flag == DFFT_ALLOC_HOST) {
        p = malloc(bytes ? bytes : 1);
    } else if (flag == DFFT_ALLOC_DEV) {
        hipError_t e = hipMalloc(&p, bytes ? bytes : 16);
        if (e != hipSuccess) {
            set_error(std::string("hipMalloc failed: ") + hipGetErrorString(e));
            return nullptr;
        }
    } else {
        set_error("Fail to allocate memory!");  // fft_mpi_3d_api.cpp:226
    }
    return p;
}

int dfft_free(void* p, int flag) {
    if (!p) return DFFT_OK;
    if (flag == DFFT_ALLOC_HOST) {
        free(p);
        return DFFT_OK;
    }
    DFFT_HIP_TRY(hipFree(p));
    return DFFT_OK;
}

}  // extern "C"
