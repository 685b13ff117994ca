// dfft_plan_impl.h -- what the host units behind the C-ABI share (not installed): the plan object and the helpers of
//   dfft_core.cpp       last error, twiddle cache, length / extent rules, the query-only entry points
//   dfft_passes.cpp     row and Bluestein passes, the executing-plan context
//   dfft_plan.cpp       C2C slab plans: create, the execute sequences, describe / sync / times / destroy
//   dfft_plan_tune.cpp  placement of the hand-over and receive buffers
//   dfft_plan_r2c.cpp   R2C / C2R plans
//   dfft_plan_conv.cpp  spectral-filter plans
//   dfft_batch.cpp      the plan-less batched entry points
#pragma once
#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "dfft_bluestein.h"
#include "dfft_conv.h"
#include "dfft_conv_multi.h"
#include "dfft_internal.h"
#include "dfft_long.h"
#include "dfft_zy.h"

#define DFFT_TRY(stmt)        \
    do {                      \
        int rc_ = (stmt);     \
        if (rc_) return rc_;  \
    } while (0)

namespace dfft {

// ---- dfft_core.cpp ---------------------------------------------------------------------------------------------------------------
const std::string& last_error();  // this thread's dfft_last_error()
inline bool valid_dtype(int dtype) { return dtype == DFFT_F64 || dtype == DFFT_F32; }
inline bool valid_direction(int direction) { return direction == DFFT_FORWARD || direction == DFFT_BACKWARD; }
// dfft_length_kind without the range checks' cost on the hot path: single-pass lengths answer at the first test
int length_kind(long long n);
// dfft_real_form: 1 the half-length kernels of dfft_real.hip (n even, n/2 single-pass); 2 two-for-one pairs on an n-point single-pass
// transform (the odd 7-smooth n <= 4096, and n = 2); 3 two-for-one pairs on the n-point four-step or Bluestein transform; 0 none
int real_form(long long n);
// supported extent of the column transforms (include/dfft.h, "Supported extent"); in16 / out16: that pointer is 16-byte aligned
bool aligned16(const void* p);
bool scratch16();  // the leased scratch is 16-byte aligned
bool cols_extent_ok(long long n, long long width, int dtype, bool in16, bool out16);
bool bluestein_extent_ok(long long n, long long s, int dtype);
bool any_extent_ok(long long n, long long s, int dtype, bool in16, bool out16);
std::string extent_message(const char* fn, long long n, long long s);
// the byte ranges [a, a + ab) and [b, b + bb) overlap (or start at the same address)
inline bool ranges_overlap(const void* a, uintptr_t ab, const void* b, uintptr_t bb) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 == b0 || (a0 < b0 + bb && b0 < a0 + ab);
}
// The complex entry points and plans run out of place or exactly in place: two different pointers whose `bytes`-long ranges overlap
// would have one pass read what another has already overwritten.
inline bool partly_overlap(const void* in, const void* out, uintptr_t bytes) { return in != out && ranges_overlap(in, bytes, out, bytes); }

// Where the rows of an [x][y][z] slab sit: elements between consecutive rows and between consecutive planes.  The natural
// layout is {N2, N1*N2}; the plan's padded work buffer (dfft_plan_s::wbuf) uses {N2 + one line, N1*pitch + one line}.
struct SlabLayout {
    long long pitch, plane;
};

// Bluestein axes of a plan: the tables of its kind-3 axes, built when the plan was created, and the plan's scratch for the multi-pass
// form -- so that an execute allocates nothing
struct PlanBluestein {
    std::vector<BluesteinTablesPtr> tables;
    void*                           scratch = nullptr;
    size_t                          bytes = 0;
    bool                            fused = true;  // DFFT_BLUESTEIN_FUSED when the plan was created
};

// The per-(device, stream) scratch of callers without a plan (dfft_long.h), held for one scope.  The lease is not re-entrant: no call
// that leases by itself (dfft_fft1d_rows / _cols / _any, fft_rows without a scratch of its own) may run while one is held.
class ScratchLease {
public:
    ScratchLease() = default;
    ScratchLease(ScratchLease&& o) noexcept : lease_(o.lease_), buf_(o.buf_) { o.lease_ = o.buf_ = nullptr; }
    ScratchLease(const ScratchLease&) = delete;
    ScratchLease& operator=(const ScratchLease&) = delete;
    ~ScratchLease() { release(); }
    bool acquire(size_t bytes, hipStream_t stream) {  // false: nothing could be allocated (and nothing is leased)
        release();
        buf_ = long_scratch(bytes, stream, &lease_);
        return buf_ != nullptr;
    }
    void* get() const { return buf_; }
    void  release() {
        long_scratch_release(lease_);
        lease_ = buf_ = nullptr;
    }

private:
    LongScratchLease lease_ = nullptr;
    void*            buf_ = nullptr;
};

}  // namespace dfft

// ---------------------------------------------------------------------------------------------------------------
struct dfft_plan_s {
    long long   N[3] = {0, 0, 0};
    int         dtype = DFFT_F64, direction = DFFT_FORWARD;
    int         P = 1, me = 0;
    unsigned    flags = 0;
    bool        inplace = false, is_last = false;
    double      scale = 1.0;  // folded into the X pass (dfft_plan_set_scale)
    bool        exch = false;  // t2 runs: P > 1, or DFFT_FORCE_EXCHANGE=1 with an RCCL communicator (single-GPU tests)
    long long   max_count = 0;
    dfft::Slab  sx{0, 1, 0}, sy{0, 1, 0};  // X slabs (before), Y slabs (after)
    long long   xs = 0, ys = 0;            // this device's extents
    void *      in = nullptr, *out = nullptr, *buf1 = nullptr, *buf2 = nullptr;
    dfft_comm_t comm = nullptr;
    int         device = 0;
    hipStream_t stream = nullptr;
    hipEvent_t  ev[6] = {};  // [0..4] stage boundaries, [5] between the two FFT kernels of the YZ stage
    double      host_t[4] = {0, 0, 0, 0};
    bool        host_timed = false;
    bool        timed = true;  // the last execute recorded its stage events (false: DFFT_EXEC_NO_TIMING)
    dfft::ExchangeDesc xd;
    dfft::ExchangeDesc xd2;        // DFFT_PLAN_NATURAL: the second (Y -> X) exchange
    long long   chunk_planes = 0;  // planes per Z+Y chunk (Infinity-Cache blocking); 0 = whole slab in one launch pair
    // DFFT_PLAN_OVERLAP (forward, P > 1): exchange parts on a second stream behind the plane-chunked Z+Y passes
    long long               part_planes = 0;  // planes per exchange part, identical on every rank; 0 = overlap off
    hipStream_t             stream2 = nullptr;
    void*                   rbuf = nullptr;  // dedicated receive buffer of the overlapped exchange
    hipEvent_t              join_ev = nullptr;
    std::vector<hipEvent_t> part_ev;
    // t2/t3 overlap inside DFFT_PLAN_OVERLAP: the Y range of every destination is cut into `ycuts` sub-blocks; the last
    // X-plane part is exchanged sub-block by sub-block and the X pass of sub-block k runs while sub-block k+1 is in flight
    int                     ycuts = 1;
    std::vector<hipEvent_t> y_ev;
    // Padded work buffer for the Z <-> Y (and, on a single GPU, Y <-> X) intermediate of the fused pipeline: rows one
    // cache line longer than N2 and planes one more line apart, so that the column kernels' 128-byte segments -- N1 of
    // them one row pitch apart (Y pass), N0 of them one plane apart (X pass) -- do not all fall on the same memory
    // channels.  With power-of-two extents the natural strides (8 KiB, 4 MiB at 512^3 fp64) cost 11-15 % of the passes'
    // data rate (tools/membench4.hip, profiles/r02/README.md section 1).  Caller-visible buffers keep the reference layouts.
    void*                   wbuf = nullptr;
    dfft::SlabLayout        wl{0, 0};
    // an axis beyond the single-pass range (> 4096 points, dfft_long.hip): the plan runs the un-fused stage structure (only
    // contiguous rows and natural-layout columns need the four-step form then) and owns the scratch slab it needs
    bool                    long_axis = false;
    void*                   lbuf = nullptr;
    // axes of dfft_length_kind 3 (DFFT_PLAN_ANY_LENGTH): Bluestein transforms on the un-fused structure, tables and scratch owned here
    dfft::PlanBluestein     bs;
    // Placement of the hand-over buffer (dfft_plan_tune).  The X pass runs 5-8 % faster when the buffer it reads and the
    // buffer it writes lie in different regions of the device's physical memory (regions are 4 ... 70 GiB long, consecutive
    // allocations usually share one; profiles/r03/README.md section 1, tools/xprobe.hip), so tuning times the X-pass kernel
    // alone on candidate allocations made one after the other -- all kept alive, so that each moves the next one on -- until
    // one behaves differently, and keeps the one on which it ran fastest.
    // t0 as one persistent launch (dfft_zy.hip) instead of two launches per cache chunk: single-GPU fused plans in fp64 whose Y and
    // Z lengths the kernel is built for.  zy_ctl: its control block (ticket counter, per-plane counters, error word).
    dfft::ZyCtl*            zy_ctl = nullptr;
    // the plan's shape and flags select the one-launch stage (whether or not THIS device could allocate its control block): the same
    // on every device of a communicator, so it -- and not zy_ctl -- decides who takes part in the agreement round of dfft_execute
    bool                    zy_eligible = false;
    unsigned*               zy_err = nullptr;   // pinned host word the kernel writes ZY_ERR_* to when it gives up (read without a copy)
    unsigned                zy_spin_polls = 0;  // bound of a consumer unit's wait (polls; DFFT_ZY_SPIN_POLLS)
    int                     zy_fault = 0;       // DFFT_ZY_FAULT=n (test hook): launch number n of the stage waits for producers that never come
    unsigned                zy_launches = 0;
    bool                    zy_on = false;
    unsigned                zy_ticket = 0;  // value of the control block's ticket counter when the next launch starts
    unsigned                zy_execs = 0, zy_cur = 0;  // executes that have used the stage; index of the current one (per-plane counters)
    // overlapped forward plans: ONE launch of the stage over the whole slab that counts, per X-plane part, the column units whose results
    // are in memory (dfft_zy.hip, SIG); the exchange stream waits for a part's count and ships it while the launch computes the next part
    unsigned*               zy_part_done = nullptr;    // device: one counter per part (never reset: targets run on from execute to execute)
    unsigned                zy_sig_execs = 0;
    bool                    zy_lazy = false;           // lazy-publish form of the one-launch kernel (un-packed launches; DFFT_ZY_LAZY=0: eager)
    bool                    zy_inv_rows_first = true;  // backward single-GPU plans: inverse stage rows first (DFFT_ZY_INV_ROWS_FIRST=0: columns first)
    int                     x_hints = 0;               // DFFT_X_VARIANT when the plan was created: FFT_HINT_HALF_PREFETCH / _EARLY_WAIT / _LATE_WAIT / _STATIC_TILES
    // Forward fp64 plans with a 512-point X axis: the X pass hands its tiles out by ticket (TuneTransposedStoreTicket, dfft_fft_impl.h).
    // x_ticket_ctr: the counter in device memory, zeroed once and never reset; x_ticket: its value when the next launch starts -- every
    // whole-slab launch_x (executes and the probe launches of dfft_plan_tune alike) reads it and moves it on.  The host steps the base in
    // the order it queues launches on the plan's stream: a plan executed from two streams or threads at once is outside the contract
    // anyway, and here it would hand the tiles of one launch to the other.
    // The base is a kernel ARGUMENT, fixed when the launch is queued: an execute captured into a hipGraph and replayed would replay a stale
    // base -- every ticket would decode past the last tile and the output would be left unwritten.  The library has no graph path and
    // plans must not be captured (the one-launch YZ stage steps its ticket and done bases the same way).
    unsigned*               x_ticket_ctr = nullptr;
    unsigned                x_ticket = 0;
    int                     x_form = 0;  // X_FORM_* of the kernel the last whole-slab X pass ran on (before the first one: will run on); 0: another kernel
    int                     grid_x = 0, grid_y = 0, grid_z = 0;  // DFFT_X_GRID / DFFT_Y_GRID / DFFT_Z_GRID when the plan was created (0 = no cap)
    // Rows of the exchange buffers rotated by rot_elems elements per X plane (RotMap, dfft_kernels.h): P > 1 fused plans whose
    // received planes are a power-of-two distance apart.  0 = off.
    int                     rot_elems = 0;
    // real-to-complex / complex-to-real plans (dfft_plan_create_r2c): N[2] is the COMPLEX width n2/2 + 1 -- what the Y pass, the exchange
    // and the X pass see -- and n2r the real length.  The Z rows run into / out of the plan's own complex intermediate cbuf ([xs][N1][cl.pitch],
    // rows padded to whole cache lines; also the send buffer of the backward exchange): an R2C row is wider on output than on input.
    bool                    r2c = false;
    long long               n2r = 0;
    void*                   cbuf = nullptr;
    dfft::SlabLayout        cl{0, 0};
    // dfft_plan_create_r2c_any: the form of the real axis (dfft_real_form; 1 = exactly dfft_plan_create_r2c's plan) and, forms 2 / 3, the
    // two-for-one rows' Bluestein tables (Bluestein n2r only) and scratch, sized for one cache chunk of rows (dfft_real_pair.hip)
    bool                    real_any = false;
    int                     real_form = 1;
    dfft::BluesteinTablesPtr rtab;
    bool                    rfused = true;  // DFFT_BLUESTEIN_FUSED when the plan was created
    size_t                  rcap = dfft::kScratchCap;  // chunk_cap_env() when the plan was created: what sized rscratch cuts every execute
    void*                   rscratch = nullptr;
    size_t                  rscratch_bytes = 0;
    // spectral-filter plans (dfft_plan_create_conv).  The handle the caller holds has `conv` set and owns two HALF plans: a forward plan
    // that stops in front of its X pass and a backward plan that starts behind its inverse X pass (conv_half; the stage code of
    // execute_forward / execute_backward, minus launch_x), which share the stream and the hand-over buffer; the X stage in between is
    // dfft_conv.hip's.  conv_no_rot: a half plan whose X stage takes the multi route keeps plain rows in its exchange buffers (the in-place
    // C2C column kernels exist for plain rows only).  borrowed: stream and hand-over buffer belong to the other half.
    // Real-field plans (dfft_plan_create_conv_real) are the same handle over an R2C and a C2R half plan (create_r2c / execute_r2c with
    // conv_half set: no X pass, nothing captured at plan time, N[2] = the plan's private complex width Nc >= n2r/2 + 1); there `borrowed`
    // covers the stream and the complex intermediate cbuf.
    struct ConvState*       conv = nullptr;
    bool                    conv_half = false, conv_no_rot = false, borrowed = false;
    bool                    own_cbuf = false;  // a borrowed half of a multi-output plan that owns its intermediate all the same
    std::vector<float>      w_ms;            // report: X-pass time of every candidate tried (w_ms[w_kept] is the kept one)
    int                     w_kept = -1;
    float                   w_final_ms = 0.f;  // the kept candidate re-timed after the others were freed
};

// state of a spectral-filter plan (dfft_plan_s::conv)
struct ConvState {
    dfft_plan_s *f = nullptr, *b = nullptr;  // the forward / backward half plans
    void*        sbuf = nullptr;             // send buffer of the forward exchange (plans with a communicator)
    void*        filt = nullptr;             // the filter copy, in the hand-over slab's physical layout
    size_t       filt_bytes = 0;
    int          kind = -1;                  // DFFT_FILTER_*; -1: no filter yet
    bool         fused = false;              // xconv_cols_kernel (else the multi route)
    dfft::ConvLaunch L{};                    // the X stage's slab: buffers, strides, rotation
    long long    slab_elems = 0;             // elements of the slab, padding included (= elements of the filter copy)
    double       x_host = 0;                 // host-timed X stage of the last DFFT_EXEC_SYNC_STAGES execute
    bool         real = false;               // dfft_plan_create_conv_real: R2C / C2R halves, the slab is the half spectrum at width L.ncols
    long long    nh = 0;                     // real-field plans: N2/2 + 1, the bins per row the caller's filter has
    // multi-output real-field plans (dfft_plan_create_conv_real_multi): nout > 0 outputs, one C2R half per output (bk[0] == b), the slabs
    // the X stage writes (M.out[0] == L.in; M.out[k >= 1]: the intermediate of bk[k] at P = 1, a send buffer of the plan's own -- xslab[k] --
    // at P > 1) and the factor tables: `fact` holds a table of ones and, per output, na + nrow + L.ncols elements (a, this device's part
    // of b, zero-padded c); M.ax / by / cz point at the ones until dfft_conv_set_factors gives something else
    int           nout = 0;
    dfft_plan_s*  bk[dfft::CONV_MAX_OUTPUTS] = {};
    void*         xslab[dfft::CONV_MAX_OUTPUTS] = {};
    void*         fact = nullptr;
    long long     fa = 0, fb = 0;            // elements reserved for a and b per output (even: every table starts on a 16-byte boundary)
    dfft::ConvMultiArgs M{};
    bool          unit[dfft::CONV_MAX_OUTPUTS] = {};  // all three factors of output k are ones
    int           backs() const { return nout > 0 ? nout : 1; }
    dfft_plan_s*  back(int k) const { return nout > 0 ? bk[k] : b; }
};

namespace dfft {

// ---- dfft_passes.cpp -------------------------------------------------------------------------------------------------------------
// the three passes are address maps of the one FFT kernel template: n points `stride` apart, columns `cstride` apart
AxisMap plain_axis(long long n, long long stride, long long cstride);
int check_launch(hipError_t e, const char* what);
// Length-n Bluestein transforms of data[batch][n][s] (dfft_bluestein.hip): with the executing plan's tables and scratch, or -- plan-less
// callers -- the cached tables and the per-(device, stream) scratch lease of the four-step transforms
int bluestein_pass(const void* in, void* out, long long n, long long s, long long batch, int dtype, int dir, double scale, hipStream_t st);
// contiguous rows: `rows` FFTs of length n; row pitch n, or (lin/lout given) rows_per_plane rows per plane in the given layouts
int fft_rows(const void* in, void* out, int n, long long rows, int dtype, int dir, hipStream_t s, long long first_row = 0, int hints = 0,
             double scale = 1.0, const SlabLayout* lin = nullptr, const SlabLayout* lout = nullptr, long long rows_per_plane = 0,
             void* long_scratch_buf = nullptr, int grid_limit = 0);
// While one is alive the passes above run with the plan's own scratch slab, row-grid cap and Bluestein tables (dfft_execute)
struct ExecutingPlan {
    explicit ExecutingPlan(const dfft_plan_s* p);
    ~ExecutingPlan();
    ExecutingPlan(const ExecutingPlan&) = delete;
    ExecutingPlan& operator=(const ExecutingPlan&) = delete;
};

// ---- plan creation (dfft_plan.cpp) -----------------------------------------------------------------------------------------------
// The argument checks every plan-creating entry point starts with, in this order: plan / in, sizes, dtype, direction (`direction`
// given), device index, communicator and its size; then -- where the rules ask for them -- out of place, and no flag outside the mask.
struct PlanArgRules {
    const int*  direction = nullptr;       // tested when given
    const char* out_of_place = nullptr;    // text behind "<fn>: " when out is NULL or `in`
    unsigned    flags_allowed = ~0u;
    const char* flags_text = nullptr;      // text behind "<fn>: " when a flag outside flags_allowed is set
};
int check_plan_args(const std::string& fn, const void* plan, const void* in, const void* out, long long n0, long long n1, long long n2, int dtype,
                    dfft_comm_t comm, int global_idx, int total_devices, unsigned flags, const PlanArgRules& rules);
// A plan with its geometry filled in: shape, precision, direction, the slabs of device `me` of `P`, communicator, flags and the grid
// caps (DFFT_X_GRID / DFFT_Y_GRID / DFFT_Z_GRID).  It owns nothing yet; the create function sets what is its own.
dfft_plan_s* plan_new(const long long shape[3], int dtype, int direction, int P, int me, dfft_comm_t comm, unsigned flags);
// Owner of a half-built plan of any kind: leaving a create function early destroys the plan and keeps the failure's message
struct PlanDeleter {
    void operator()(dfft_plan_s* p) const;
};
typedef std::unique_ptr<dfft_plan_s, PlanDeleter> PlanOwner;
// in-process multi-GPU (the reference's thread-per-GPU model): let `device` push straight into its peers' receive buffers over xGMI
// instead of staging peer copies through the host
void enable_peer_access(int device);
// The evened-out cache chunk: the largest whole number of planes that fits `mb` MiB, one plane less from 8 MiB planes on, evened out
// over the chunks (measurements: dfft_plan_create)
inline long long evened_chunk_planes(long long planes, long long plane_bytes, long long mb) {
    long long fit = std::max(1ll, (mb << 20) / plane_bytes);
    if (plane_bytes >= (8ll << 20) && fit > 1) --fit;
    const long long nchunks = std::max(1ll, (planes + fit - 1) / fit);
    return (planes + nchunks - 1) / nchunks;
}
// Planes per Z+Y chunk of a plan's slab (0: the whole slab): `rule_planes` when the caller's own rule gave a size, else the evened-out
// chunk of DFFT_CHUNK_MB (default `default_mb`; 0 disables); DFFT_CHUNK_PLANES=n overrides either
long long cache_chunk_planes(long long planes, long long plane_bytes, long long default_mb, long long rule_planes = 0);
// conv_half: 0 = dfft_plan_create; 1 / 2 = a half plan of dfft_plan_create_conv (2: plain rows in the exchange buffers)
int plan_create_impl(dfft_plan_t* plan, long long n0, long long n1, long long n2, int dtype, int direction, void* in, void* out, dfft_comm_t comm,
                     int global_idx, int total_devices, unsigned flags, int conv_half);
int fill_exchange(dfft_plan_s* p, ExchangeDesc& x, int direction);

// ---- stages (dfft_plan.cpp) ------------------------------------------------------------------------------------------------------
struct StageClock {
    dfft_plan_s* p;
    bool         sync;
    int          idx = 0;
    std::chrono::steady_clock::time_point t;
    int begin();
    int end_stage();
};
// Y pass.  Natural side: [xs][N1][N2].  Packed side: [d][xs][yl_d][N2].
// lay_in / lay_out: layout of the natural side(s) (nullptr = {N2, N1*N2}); ignored for a packed side.
int launch_y(dfft_plan_s* p, const void* in, void* out, bool packed_side_is_out, bool use_packed, long long x0, long long nx, int hints = 0,
             const SlabLayout* lay_in = nullptr, const SlabLayout* lay_out = nullptr);
// X pass.  Slab side: [N0][ys][N2] (x slowest).  Transposed side: [ys][N2][N0] (kx fastest).
// keep_slab: store [x][ys][N2] again instead of the transposed [ys][N2][kx] (natural-order plans)
// ys_part > 0: only a [N0][ys_part][N2] sub-slab (in/out already point at it)
// slab_lay: layout of the slab side when it is the plan's padded work buffer (single GPU: ys == N1), else [x][ys][N2]
int launch_x(dfft_plan_s* p, const void* in, void* out, bool keep_slab = false, long long ys_part = 0, const SlabLayout* slab_lay = nullptr);
int zy_check(dfft_plan_s* p);

// ---- the other kinds of plan -----------------------------------------------------------------------------------------------------
int execute_r2c(dfft_plan_s* p, bool sync);                                    // dfft_plan_r2c.cpp
int place_recv_buffer(dfft_plan_s* p);                                         // dfft_plan_tune.cpp
size_t recv_buffer_bytes(const dfft_plan_s* p);
int conv_execute(dfft_plan_s* p, unsigned exec_flags);                         // dfft_plan_conv.cpp
int conv_describe(const dfft_plan_s* p, char* buf, int len);
int conv_sync(dfft_plan_s* p);
int conv_stage_times(dfft_plan_s* p, double t[4]);
int conv_destroy(dfft_plan_s* p);
// A half plan of dfft_plan_create_conv_real: the plan's complex width, and the forward half whose stream and intermediate the backward
// half borrows (nullptr: this IS the forward half)
// Multi-output plans: C2R half `output` >= 1 borrows the stream but has a receive buffer of its own (the output index goes into the pool
// key: peers push into it while this rank may still unpack the previous output's) and, with own_cbuf, an intermediate of its own -- slab
// `output` of the X stage at P = 1
struct R2cHalf {
    long long    nc;
    dfft_plan_s* share;
    int          output = 0;
    bool         own_cbuf = false;
};
// dfft_plan_create_r2c (any = false) and dfft_plan_create_r2c_any (any = true: the real axis of any dfft_real_form != 0); half != nullptr:
// a half plan of dfft_plan_create_conv_real, which has checked the arguments (`in` / `out`: the real slabs the R2C half reads / the C2R
// half writes; the forward half's `out` is the plan's send buffer, NULL without an exchange)
int create_r2c(dfft_plan_t* plan, long long n0, long long n1, long long n2, int dtype, int direction, void* in, void* out, dfft_comm_t comm,
               int global_idx, int total_devices, unsigned flags, bool any, const R2cHalf* half = nullptr);
// Elements of the two receive buffers of a real-field spectral-filter plan at complex width nc -- the forward one holds [N0][ys][nc], the
// backward one the packed [q][xs][yl_q][nc] -- as a bound that is the same on every rank (pooled buffers are matched by size)
inline long long conv_real_recv_count(long long n0, long long n1, long long nc, int P) {
    const Slab sx = make_slab(n0, P), sy = make_slab(n1, P);
    return std::max(n0 * sy.blk, (long long)P * sx.blk * sy.blk) * nc;
}

}  // namespace dfft
