// dfft_plan_r2c.cpp -- real-to-complex / complex-to-real slab plans: create, the Z rows on the real side, the execute sequence.
#include "dfft_plan_impl.h"
#include "dfft_real.h"
#include "dfft_real_pair.h"

namespace dfft {

// ---- real-to-complex / complex-to-real plans -------------------------------------------------------------------------------------
// The Z rows of planes [x0, x0 + nx): R2C real slab `in` ([x][N1][n2r] reals) -> intermediate, or C2R intermediate -> real slab `out`.
static int real_rows(dfft_plan_s* p, const void* in, void* out, int dir, long long x0, long long nx) {
    const long long n1 = p->N[1];
    const size_t    cs = elem_bytes(p->dtype), rs = cs / 2;
    if (p->real_form != 1) {  // two-for-one pairs (rows pair up across plane boundaries)
        RealPairLaunch R;
        std::memset(&R, 0, sizeof(R));
        R.dtype = p->dtype;
        R.n = p->n2r;
        R.dir = dir;
        const size_t roff = (size_t)x0 * n1 * p->n2r * rs, coff = (size_t)x0 * p->cl.plane * cs;
        R.in = (const char*)in + (dir > 0 ? roff : coff);
        R.out = (char*)out + (dir > 0 ? coff : roff);
        R.rows = nx * n1;
        R.rows_per_plane = n1;
        R.rpitch = p->n2r;
        R.rplane = n1 * p->n2r;
        R.cpitch = p->cl.pitch;
        R.cplane = p->cl.plane;
        return real_pair_rows(R, p->rtab.get(), p->rfused, p->rcap, p->rscratch, p->rscratch_bytes, p->stream);
    }
    RealLaunch      L;
    std::memset(&L, 0, sizeof(L));
    L.dtype = p->dtype;
    L.n2 = (int)p->n2r;
    L.dir = dir;
    const size_t roff = (size_t)x0 * n1 * p->n2r * rs, coff = (size_t)x0 * p->cl.plane * cs;
    L.in = (const char*)in + (dir > 0 ? roff : coff);
    L.out = (char*)out + (dir > 0 ? coff : roff);
    L.rows = nx * n1;
    L.rows_per_plane = n1;
    L.rpitch = p->n2r;
    L.rplane = n1 * p->n2r;
    L.cpitch = p->cl.pitch;
    L.cplane = p->cl.plane;
    L.scale = 1.0;  // dfft_plan_set_scale: folded into the X pass, as in C2C plans
    return check_launch(launch_real_rows(L, p->stream), dir > 0 ? "R2C rows" : "C2R rows");
}

// Forward: R2C rows -> intermediate, Y columns (in place, or packing into the send buffer `out`) per cache chunk | exchange into
// bufferDev1 | X pass -> out.  Backward: inverse X pass (into the intermediate, or the send buffer = the intermediate) | exchange into
// bufferDev1 | per cache chunk: Y columns (in place, or unpacking bufferDev1 into the intermediate), then C2R rows -> out -- Z last, as
// numpy's irfftn (inverse C2C along X and Y, then C2R along Z).
int execute_r2c(dfft_plan_s* p, bool sync) {
    StageClock      clk{p, sync};
    DFFT_TRY(clk.begin());
    const void*     src = (p->flags & DFFT_PLAN_INPUT_FROM_IN) ? p->in : p->buf1;
    const long long cp = p->chunk_planes > 0 ? p->chunk_planes : p->xs;
    const bool      chunked = cp < p->xs;
    const SlabLayout* lc = &p->cl;
    if (p->direction == DFFT_FORWARD) {
        for (long long x0 = 0; x0 < p->xs; x0 += cp) {
            const long long nx = std::min(cp, p->xs - x0);
            DFFT_TRY(real_rows(p, src, p->cbuf, +1, x0, nx));
            if (p->exch) DFFT_TRY(launch_y(p, p->cbuf, p->buf2, true, true, x0, nx, chunked ? FFT_HINT_STREAM_OUT : 0, lc));
            else DFFT_TRY(launch_y(p, p->cbuf, p->cbuf, true, false, x0, nx, 0, lc, lc));
        }
        DFFT_TRY(clk.end_stage());
        DFFT_TRY(clk.end_stage());  // t1 folded into t0
        if (p->exch) DFFT_TRY(comm_exchange(p->comm, p->xd, p->stream));
        DFFT_TRY(clk.end_stage());
        // (half plans of a real-field spectral-filter plan: the X stage works in place on what t0 / t2 left -- conv_x_stage -- and has
        // left its result where the inverse X pass would have: the intermediate, or the send buffer of the backward exchange)
        if (!p->conv_half) DFFT_TRY(launch_x(p, p->exch ? p->buf1 : p->cbuf, p->buf2, false, 0, p->exch ? nullptr : lc));
        DFFT_TRY(clk.end_stage());
        return DFFT_OK;
    }
    if (!p->conv_half) DFFT_TRY(launch_x(p, src, p->cbuf, false, 0, p->exch ? nullptr : lc));
    DFFT_TRY(clk.end_stage());
    if (p->exch) DFFT_TRY(comm_exchange(p->comm, p->xd, p->stream));
    DFFT_TRY(clk.end_stage());
    DFFT_TRY(clk.end_stage());  // unpack folded into the Y pass
    for (long long x0 = 0; x0 < p->xs; x0 += cp) {
        const long long nx = std::min(cp, p->xs - x0);
        if (p->exch) DFFT_TRY(launch_y(p, p->buf1, p->cbuf, false, true, x0, nx, chunked ? FFT_HINT_STREAM_IN : 0, nullptr, lc));
        else DFFT_TRY(launch_y(p, p->cbuf, p->cbuf, false, false, x0, nx, 0, lc, lc));
        DFFT_TRY(real_rows(p, p->cbuf, p->buf2, -1, x0, nx));
    }
    DFFT_TRY(clk.end_stage());
    return DFFT_OK;
}

int create_r2c(dfft_plan_t* plan, long long n0, long long n1, long long n2, int dtype, int direction, void* in, void* out, dfft_comm_t comm,
               int global_idx, int total_devices, unsigned flags, bool any, const R2cHalf* half) {
    const std::string fn = any ? "dfft_plan_create_r2c_any" : "dfft_plan_create_r2c";
    PlanArgRules rules;
    rules.direction = &direction;
    if (!half) rules.out_of_place = "real-to-complex plans are out of place (out != NULL, out != in)";
    rules.flags_allowed = DFFT_PLAN_INPUT_FROM_IN;
    rules.flags_text = "only DFFT_PLAN_DEFAULT and DFFT_PLAN_INPUT_FROM_IN are supported (no OVERLAP, NATURAL or UNFUSED real-to-complex plans)";
    DFFT_TRY(check_plan_args(fn, plan, in, out, n0, n1, n2, dtype, comm, global_idx, total_devices, flags, rules));
    const int form = any ? real_form(n2) : 1;
    if (any && form == 0)
        return fail(DFFT_EUNSUPPORTED, fn + ": N2 = " + std::to_string(n2) + " -- no real form (at most 2^23, or a four-step length)");
    if (!any && !real_length_supported(n2))
        return fail(DFFT_EUNSUPPORTED, fn + ": N2 = " + std::to_string(n2) +
                                           " -- the real axis must be even with N2/2 a supported length of at most 4096");
    for (long long n : {n0, n1})
        if (n > 4096 || !dfft_length_supported(n))
            return fail(DFFT_EUNSUPPORTED, fn + ": FFT length " + std::to_string(n) +
                                               " -- N0 and N1 must be single-pass lengths (products of 2, 3, 5, 7 up to 4096)");
    long long rc_n = 0, cc_n = 0, rc_last = 0, cc_last = 0;
    if (int rc = dfft_r2c_counts(n0, n1, n2, total_devices, global_idx, &rc_n, &cc_n)) return rc;
    if (int rc = dfft_r2c_counts(n0, n1, n2, total_devices, total_devices - 1, &rc_last, &cc_last)) return rc;
    long long rc0 = 0, cc0 = 0;
    (void)dfft_r2c_counts(n0, n1, n2, total_devices, 0, &rc0, &cc0);
    if (std::max(cc0, cc_last) >= (1ll << 31)) return fail(DFFT_EUNSUPPORTED, fn + ": more than 2^31 complex elements per device");
    if (dfft_device_count() < 1) return fail(DFFT_ENOGPU, fn + ": no HIP device visible (no CPU fallback)");

    const long long nh = half ? half->nc : n2 / 2 + 1;  // the complex width: what the Y pass, the exchange and the X stage see
    trace("dfft_plan_create_r2c", n0 * 1000000 + n1 * 1000 + n2 % 1000, (long long)flags * 100 + total_devices);
    const long long shape[3] = {n0, n1, nh};
    PlanOwner       owner(plan_new(shape, dtype, direction, total_devices, global_idx, comm, flags));
    dfft_plan_s*    p = owner.get();
    p->r2c = true;
    p->conv_half = half != nullptr;
    p->borrowed = half && half->share;
    p->own_cbuf = p->borrowed && half->own_cbuf;
    p->n2r = n2;
    p->real_any = any;
    p->real_form = form;
    p->exch = total_devices > 1;
    p->max_count = cc_n;
    p->in = in;
    p->out = out;
    p->buf2 = out;
    const size_t cs = elem_bytes(dtype), rs = cs / 2;
    // the intermediate: rows of nh bins padded to whole 128-byte lines (a pitch of nh alone puts the rows off line alignment)
    const long long line = 128 / (long long)cs;
    p->cl.pitch = (nh + line - 1) / line * line;
    p->cl.plane = n1 * p->cl.pitch;
    hipError_t e = hipGetDevice(&p->device);
    if (e == hipSuccess && comm && comm_kind(comm) == 0 && total_devices > 1) enable_peer_access(p->device);
    // bufferDev1: the real slab (R2C) or the complex input (C2R), and the receive buffer of the exchange -- the same size on every rank
    // (pooled receive buffers of IPC communicators are matched by key and size)
    // (half plans: a receive buffer alone, and only with a communicator)
    const size_t b1 = half ? (size_t)conv_real_recv_count(n0, n1, nh, total_devices) * cs : (size_t)std::max({rc0 * rs, cc0 * cs, rc_last * rs, cc_last * cs});
    const std::string rkey = std::string(half ? "convr:" : "r2c:") + std::to_string(n0) + "x" + std::to_string(n1) + "x" + std::to_string(n2) + ":" +
                             std::to_string(dtype) + ":" + std::to_string(total_devices) +
                             (half && half->output > 0 ? ":o" + std::to_string(half->output) : std::string());
    if (e == hipSuccess && (!half || comm) && comm_recv_alloc(comm, rkey + ":b1", b1, &p->buf1) != DFFT_OK) e = hipErrorOutOfMemory;
    // the intermediate, also the send buffer of the backward exchange ([N0][ys][nh])
    const size_t cbytes = (size_t)(half ? p->xs * p->cl.plane : std::max(p->xs * p->cl.plane, n0 * p->ys * nh)) * cs;
    if (p->borrowed) {
        p->cbuf = half->share->cbuf;
        p->stream = half->share->stream;
        if (p->own_cbuf) {
            p->cbuf = nullptr;
            if (e == hipSuccess) e = hipMalloc(&p->cbuf, cbytes);
        }
    } else {
        if (e == hipSuccess) e = hipMalloc(&p->cbuf, cbytes);
        if (e == hipSuccess) e = hipStreamCreateWithFlags(&p->stream, hipStreamNonBlocking);
    }
    // input captured at plan time, on the plan's stream (see dfft_plan_create); exactly the caller's elements, nothing beyond them
    const size_t ibytes = direction == DFFT_FORWARD ? (size_t)rc_n * rs : (size_t)(p->ys * nh * n0) * cs;
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess && !half) e = hipMemcpyAsync(p->buf1, in, ibytes, hipMemcpyDeviceToDevice, p->stream);
    // (half plans capture nothing.  Their intermediate is cleared ONCE: its columns n2/2 + 1 .. nc - 1 and its row padding are never
    // written with anything but zeros afterwards -- the argument is at the top of dfft_conv_real.hip)
    if (e == hipSuccess && half && (!p->borrowed || p->own_cbuf)) e = hipMemsetAsync(p->cbuf, 0, cbytes, p->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(p->stream);
    for (auto& ev : p->ev)
        if (e == hipSuccess) e = hipEventCreate(&ev);
    if (e != hipSuccess) return fail(DFFT_EHIP, fn + ": " + hipGetErrorString(e));
    fill_exchange(p, p->xd, direction);  // at width nh
    p->xd.sendbuf = direction == DFFT_FORWARD ? p->buf2 : p->cbuf;
    p->xd.recvbuf = p->buf1;
    if (comm) DFFT_TRY(comm_register(comm, global_idx, p->xd.recvbuf, p->device, &p->xd.slot));
    // Z+Y blocking for the 256 MiB Infinity Cache, sized on the intermediate's planes (the rule of two-launch C2C plans)
    p->chunk_planes = cache_chunk_planes(p->xs, p->cl.plane * (long long)cs, 256);
    if (form != 1) {
        // the two-for-one rows: Bluestein tables (n2 of kind 3) and the scratch of one cache chunk of rows
        p->rfused = bluestein_fused_env();
        p->rcap = chunk_cap_env();
        if (length_kind(n2) == 3) DFFT_TRY(bluestein_tables(n2, dtype, direction, &p->rtab));
        const long long rows = (p->chunk_planes > 0 ? p->chunk_planes : p->xs) * n1;
        p->rscratch_bytes = real_pair_scratch_bytes(n2, dtype, rows, p->rtab.get(), p->rfused, p->rcap);
        if (p->rscratch_bytes && (e = hipMalloc(&p->rscratch, p->rscratch_bytes)) != hipSuccess)
            return fail(DFFT_EHIP, fn + ": scratch of the real rows: " + hipGetErrorString(e));
    }
    // warm the twiddle caches so execute never allocates (form 3: the Bluestein tables above; four-step factors on first use)
    std::vector<long long> warm{n0, n1};
    if (form == 1) warm.insert(warm.end(), {n2 / 2, n2});
    if (form == 2) warm.push_back(n2);
    for (long long n : warm) {
        const void* tw;
        DFFT_TRY(get_twiddles((int)n, dtype, &tw));
    }
    *plan = owner.release();
    return DFFT_OK;
}

}  // namespace dfft

using namespace dfft;

extern "C" {

int dfft_plan_create_r2c(dfft_plan_t* plan, long long n0, long long n1, long long n2, int dtype, int direction, void* in, void* out,
                         dfft_comm_t comm, int global_idx, int total_devices, unsigned flags) {
    return create_r2c(plan, n0, n1, n2, dtype, direction, in, out, comm, global_idx, total_devices, flags, false);
}

int dfft_plan_create_r2c_any(dfft_plan_t* plan, long long n0, long long n1, long long n2, int dtype, int direction, void* in, void* out,
                             dfft_comm_t comm, int global_idx, int total_devices, unsigned flags) {
    return create_r2c(plan, n0, n1, n2, dtype, direction, in, out, comm, global_idx, total_devices, flags, true);
}

}  // extern "C"
