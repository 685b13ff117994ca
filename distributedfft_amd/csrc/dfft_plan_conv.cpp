// dfft_plan_conv.cpp -- spectral-filter (FFT convolution) plans: the complex, real-field and multi-output real-field forms.
#include "dfft_conv_real.h"
#include "dfft_plan_impl.h"
#include "dfft_real.h"

namespace dfft {

// ---- spectral-filter (FFT convolution) plans ---------------------------------------------------------------------------------------
// y = ifftn(fftn(x) . H): forward half plan (YZ stage, exchange) -> X stage in place on the slab it leaves (dfft_conv.hip: forward X
// transform, multiply by the filter copy, inverse X transform) -> backward half plan (exchange, inverse YZ stage).
static int conv_alloc_filter(dfft_plan_s* p, int kind) {
    ConvState*   c = p->conv;
    const size_t need = (size_t)c->slab_elems * elem_bytes(p->dtype) / (kind == DFFT_FILTER_REAL ? 2 : 1);
    if (c->filt && c->filt_bytes >= need) {
        // (real-field plans: the forward-only X stage of dfft_conv_set_kernel writes the columns below the plan's width only, and a copy
        // that held reals before is re-read as complex elements -- whatever it does not write must read as zero)
        if (c->real) {
            DFFT_HIP_TRY(hipStreamSynchronize(p->stream));
            DFFT_HIP_TRY(hipMemsetAsync(c->filt, 0, c->filt_bytes, p->stream));
        }
        return DFFT_OK;
    }
    DFFT_HIP_TRY(hipStreamSynchronize(p->stream));  // an execute that still reads the old copy
    if (c->filt) (void)hipFree(c->filt);
    c->filt = nullptr;
    c->filt_bytes = 0;
    c->kind = -1;
    DFFT_HIP_TRY(hipMalloc(&c->filt, need));
    c->filt_bytes = need;
    DFFT_HIP_TRY(hipMemsetAsync(c->filt, 0, need, p->stream));  // the padding of the layout is read (and multiplied into padding)
    return DFFT_OK;
}

// The X stage on the plan's stream.  to_filter: the forward transform alone, times `scale`, into the filter copy (dfft_conv_set_kernel).
static int conv_x_stage(dfft_plan_s* p, bool to_filter, double scale) {
    ConvState* c = p->conv;
    ConvLaunch L = c->L;
    DFFT_TRY(get_twiddles(L.n0, p->dtype, &L.tw));
    L.filt = c->filt;
    L.filter_real = (!to_filter && c->kind == DFFT_FILTER_REAL) ? 1 : 0;
    if (c->nout > 0 && !to_filter) {
        if (c->fused) return check_launch(launch_conv_multi_fused(L, c->M, c->nout, p->stream), "X stage of the multi-output spectral-filter plan");
        // multi route: forward columns and the multiply by the filter copy in place, ONCE; per output the factors out of place into slab k
        // and the inverse columns there; output 0 last, in place over the product
        FftLaunch X;
        std::memset(&X, 0, sizeof(X));
        X.dtype = p->dtype;
        X.n = L.n0;
        X.dir = DFFT_FORWARD;
        X.cols = 1;
        X.in = L.in;
        X.out = const_cast<void*>(L.in);
        X.tw = L.tw;
        X.imap = X.omap = plain_axis(L.n0, L.plane, 1);
        X.itile = X.otile = TileMap{L.pitch, 1};
        X.na = L.rows;
        X.ncols = (int)L.ncols;
        X.scale = 1.0;
        X.grid_limit = p->grid_x;
        DFFT_TRY(check_launch(launch_fft(X, p->stream), "X stage of the multi-output spectral-filter plan (forward columns)"));
        DFFT_TRY(check_launch(launch_conv_mul(p->dtype, L.filter_real, const_cast<void*>(L.in), c->filt, c->slab_elems, p->stream),
                              "X stage of the multi-output spectral-filter plan (multiply)"));
        X.dir = DFFT_BACKWARD;
        for (int i = 0; i < c->nout; ++i) {
            const int k = i + 1 < c->nout ? i + 1 : 0;
            void*     slab = c->M.out[k];
            if (k > 0 || !c->unit[k])
                DFFT_TRY(check_launch(launch_conv_factor_mul(L, L.in, slab, c->M.ax[k], c->M.by[k], c->M.cz[k], p->stream),
                                      "X stage of the multi-output spectral-filter plan (factors)"));
            X.in = X.out = slab;
            DFFT_TRY(check_launch(launch_fft(X, p->stream), "X stage of the multi-output spectral-filter plan (inverse columns)"));
        }
        return DFFT_OK;
    }
    if (c->fused) {
        if (to_filter) {
            L.forward_only = 1;
            L.out = c->filt;
            L.scale = scale;
        }
        return check_launch(launch_conv_fused(L, p->stream), "X stage of the spectral-filter plan");
    }
    // multi route: the C2C column kernels in place along X, the multiply, the inverse column kernels into the slab the backward half reads
    FftLaunch X;
    std::memset(&X, 0, sizeof(X));
    X.dtype = p->dtype;
    X.n = L.n0;
    X.dir = DFFT_FORWARD;
    X.cols = 1;
    X.in = L.in;
    X.out = to_filter ? c->filt : const_cast<void*>(L.in);
    X.tw = L.tw;
    X.imap = X.omap = plain_axis(L.n0, L.plane, 1);
    X.itile = X.otile = TileMap{L.pitch, 1};
    X.na = L.rows;
    X.ncols = (int)L.ncols;
    X.scale = to_filter ? scale : 1.0;
    X.grid_limit = p->grid_x;
    DFFT_TRY(check_launch(launch_fft(X, p->stream), "X stage of the spectral-filter plan (forward columns)"));
    if (to_filter) return DFFT_OK;
    DFFT_TRY(check_launch(launch_conv_mul(p->dtype, L.filter_real, const_cast<void*>(L.in), c->filt, c->slab_elems, p->stream),
                          "X stage of the spectral-filter plan (multiply)"));
    X.dir = DFFT_BACKWARD;
    X.out = L.out;
    return check_launch(launch_fft(X, p->stream), "X stage of the spectral-filter plan (inverse columns)");
}

int conv_execute(dfft_plan_s* p, unsigned exec_flags) {
    ConvState* c = p->conv;
    if (c->kind < 0) return fail(DFFT_EINVAL, "dfft_execute: this spectral-filter plan has no filter yet (dfft_conv_set_filter / dfft_conv_set_kernel)");
    const bool     sync = (exec_flags & DFFT_EXEC_SYNC_STAGES) != 0;
    const unsigned half_flags = exec_flags & ~DFFT_EXEC_PRINT;
    p->host_timed = sync;
    p->timed = sync || !(exec_flags & DFFT_EXEC_NO_TIMING);
    // a half that fails on this device alone must not leave the peers waiting in the other half's exchange: with a communicator the
    // sequence is queued to its end and the first failure is the return code
    int         rc = dfft_execute(c->f, half_flags);
    std::string msg = rc ? last_error() : std::string();
    if (rc && !p->exch) return rc;
    const auto t0 = std::chrono::steady_clock::now();
    int        rx = conv_x_stage(p, false, 1.0);
    if (rx == DFFT_OK && sync) {
        const hipError_t e = hipStreamSynchronize(p->stream);
        if (e != hipSuccess) rx = fail(DFFT_EHIP, std::string("X stage of the spectral-filter plan: ") + hipGetErrorString(e));
        c->x_host = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    }
    if (rx && !rc) {
        rc = rx;
        msg = last_error();
    }
    if (rc && !p->exch) return rc;
    for (int k = 0; k < c->backs(); ++k) {  // one after another on the one stream
        const int rb = dfft_execute(c->back(k), half_flags);
        if (rb && !rc) {
            rc = rb;
            msg = last_error();
            if (!p->exch) return rc;
        }
    }
    if (rc) return fail(rc, msg);
    return DFFT_OK;
}

int conv_describe(const dfft_plan_s* p, char* buf, int len) {
    const ConvState* c = p->conv;
    char             half[512] = "";
    (void)dfft_plan_describe(c->f, half, (int)sizeof(half));
    const char* yz = strstr(half, "yz_stage=");
    char        yzs[64] = "yz_stage=?";
    if (yz) sscanf(yz, "%63s", yzs);
    if (c->real && c->nout > 0) {
        snprintf(buf, (size_t)len, "pipeline=conv-real-multi outputs=%d xconv=%s filter=%s width=%lld bins=%lld pitch=%lld handover=%s chunk_planes=%lld",
                 c->nout, c->fused ? "fused" : "multi", c->kind == DFFT_FILTER_REAL ? "real" : (c->kind == DFFT_FILTER_COMPLEX ? "complex" : "unset"),
                 c->L.ncols, c->nh, c->L.pitch, p->exch ? "receive-buffer" : "intermediate", c->f->chunk_planes);
        return DFFT_OK;
    }
    if (c->real) {
        snprintf(buf, (size_t)len, "pipeline=conv-real xconv=%s filter=%s width=%lld bins=%lld pitch=%lld handover=%s chunk_planes=%lld",
                 c->fused ? "fused" : "multi", c->kind == DFFT_FILTER_REAL ? "real" : (c->kind == DFFT_FILTER_COMPLEX ? "complex" : "unset"),
                 c->L.ncols, c->nh, c->L.pitch, p->exch ? "receive-buffer" : "intermediate", c->f->chunk_planes);
        return DFFT_OK;
    }
    snprintf(buf, (size_t)len, "pipeline=conv xconv=%s filter=%s %s handover=%s rotated_exchange_rows=%d", c->fused ? "fused" : "multi",
             c->kind == DFFT_FILTER_REAL ? "real" : (c->kind == DFFT_FILTER_COMPLEX ? "complex" : "unset"), yzs,
             (!p->exch && c->f->wbuf) ? "padded-buffer" : (p->exch ? "receive-buffer" : "bufferDev1"), c->L.rot);
    return DFFT_OK;
}

int conv_sync(dfft_plan_s* p) {
    ConvState* c = p->conv;
    DFFT_HIP_TRY(hipStreamSynchronize(p->stream));
    DFFT_TRY(zy_check(c->f));
    for (int k = 0; k < c->backs(); ++k) DFFT_TRY(zy_check(c->back(k)));
    if (p->comm) return comm_check(p->comm);
    return DFFT_OK;
}

// t = forward YZ stage (with the packing), both exchanges, the X stage, inverse YZ stage (with the unpacking)
int conv_stage_times(dfft_plan_s* p, double t[4]) {
    ConvState* c = p->conv;
    DFFT_TRY(conv_sync(p));
    if (!p->timed) return fail(DFFT_EINVAL, "dfft_stage_times: the last execute ran with DFFT_EXEC_NO_TIMING");
    const dfft_plan_s *f = c->f, *b = c->back(0);
    if (p->host_timed) {
        t[0] = f->host_t[0] + f->host_t[1];
        t[1] = f->host_t[2];
        t[2] = f->host_t[3] + c->x_host;
        t[3] = 0;
        for (int k = 0; k < c->backs(); ++k) {  // (multi-output plans: all 1 + K exchanges, the sum of the K inverse stages)
            const dfft_plan_s* bk = c->back(k);
            t[1] += bk->host_t[1];
            t[2] += bk->host_t[0];
            t[3] += bk->host_t[2] + bk->host_t[3];
        }
        return DFFT_OK;
    }
    auto ms = [](hipEvent_t a, hipEvent_t z, double* out) {
        float v = 0;
        DFFT_HIP_TRY(hipEventElapsedTime(&v, a, z));
        *out = v * 1e-3;
        return (int)DFFT_OK;
    };
    double x1 = 0, x2 = 0;
    DFFT_TRY(ms(f->ev[0], f->ev[2], &t[0]));
    DFFT_TRY(ms(f->ev[2], f->ev[3], &x1));
    DFFT_TRY(ms(b->ev[1], b->ev[2], &x2));
    t[1] = x1 + x2;
    DFFT_TRY(ms(f->ev[3], b->ev[1], &t[2]));
    DFFT_TRY(ms(b->ev[2], b->ev[4], &t[3]));
    for (int k = 1; k < c->backs(); ++k) {
        const dfft_plan_s* bk = c->back(k);
        DFFT_TRY(ms(bk->ev[1], bk->ev[2], &x1));
        DFFT_TRY(ms(bk->ev[2], bk->ev[4], &x2));
        t[1] += x1;
        t[3] += x2;
    }
    return DFFT_OK;
}

int conv_destroy(dfft_plan_s* p) {
    ConvState* c = p->conv;
    if (p->stream) (void)hipStreamSynchronize(p->stream);
    int rc = DFFT_OK;
    for (int k = CONV_MAX_OUTPUTS - 1; k >= 1; --k) {  // multi-output plans: the halves of outputs K-1 .. 1, their slabs, the factor tables
        if (c->bk[k]) {
            const int r = dfft_plan_destroy(c->bk[k]);
            if (!rc) rc = r;
        }
        if (c->xslab[k]) (void)hipFree(c->xslab[k]);
    }
    if (c->fact) (void)hipFree(c->fact);
    if (c->b) {  // (the stream and the hand-over buffer are the forward half's)
        const int r = dfft_plan_destroy(c->b);
        if (!rc) rc = r;
    }
    if (c->f) {
        const int r = dfft_plan_destroy(c->f);
        if (!rc) rc = r;
    }
    if (c->sbuf) (void)hipFree(c->sbuf);
    if (c->filt) (void)hipFree(c->filt);
    delete c;
    delete p;
    return rc;
}

}  // namespace dfft

using namespace dfft;

// the argument rules of the three spectral-filter create entry points
static PlanArgRules conv_arg_rules() {
    PlanArgRules r;
    r.flags_allowed = DFFT_PLAN_DEFAULT;
    r.flags_text = "only DFFT_PLAN_DEFAULT is supported (no OVERLAP, NATURAL, UNFUSED, INPUT_FROM_IN -- which is implied -- or ANY_LENGTH spectral-filter plans)";
    return r;
}
// The handle the caller holds: geometry, the caller's buffers and an empty ConvState; the half plans own everything else
static dfft_plan_s* conv_new(long long n0, long long n1, long long n2, int dtype, void* in, void* out, dfft_comm_t comm, int global_idx, int total_devices,
                             unsigned flags) {
    const long long shape[3] = {n0, n1, n2};
    dfft_plan_s*    p = plan_new(shape, dtype, DFFT_FORWARD, total_devices, global_idx, comm, flags);
    p->conv = new ConvState;
    p->inplace = out == nullptr || out == in;
    p->in = in;
    p->out = p->inplace ? in : out;
    return p;
}

extern "C" {

int dfft_plan_create_conv(dfft_plan_t* plan, long long n0, long long n1, long long n2, int dtype, void* in, void* out, dfft_comm_t comm,
                          int global_idx, int total_devices, unsigned flags) {
    const std::string fn = "dfft_plan_create_conv";
    DFFT_TRY(check_plan_args(fn, plan, in, out, n0, n1, n2, dtype, comm, global_idx, total_devices, flags, conv_arg_rules()));
    for (long long n : {n0, n1, n2})
        if (length_kind(n) != 1)
            return fail(DFFT_EUNSUPPORTED, fn + ": FFT length " + std::to_string(n) + " -- every axis must be a single-pass length (products of 2, 3, 5, 7 up to 4096)");
    const Slab sx = make_slab(n0, total_devices), sy = make_slab(n1, total_devices);
    if (sx.size(total_devices - 1) < 1 || sy.size(total_devices - 1) < 1) return fail(DFFT_EINVAL, fn + ": slab decomposition leaves the last device empty");
    // (the X slabs the caller's buffers hold: dfft_local_count elements)
    if (out && partly_overlap(in, out, (uintptr_t)(sx.size(global_idx) * n1 * n2) * elem_bytes(dtype)))
        return fail(DFFT_EINVAL, fn + ": in and out overlap partly (a plan runs out of place or exactly in place)");
    if (dfft_device_count() < 1) return fail(DFFT_ENOGPU, fn + ": no HIP device visible (no CPU fallback)");

    const char* fe = getenv("DFFT_CONV_FUSED");  // A/B switch, read here once
    // fp32 runs the fused kernel on column PAIRS: an even N2 (every other stride of the slab is then even too)
    const bool  want_fused = !(fe && *fe == '0') && conv_fused_length((int)n0) && (dtype == DFFT_F64 || n2 % 2 == 0);
    trace("dfft_plan_create_conv", n0 * 1000000 + n1 * 1000 + n2 % 1000, total_devices);
    PlanOwner    owner(conv_new(n0, n1, n2, dtype, in, out, comm, global_idx, total_devices, flags));
    dfft_plan_s* p = owner.get();
    ConvState*   c = p->conv;
    p->max_count = dfft_max_count(n0, n1, n2, total_devices, p->is_last);
    if (comm) {  // the forward half packs into a send buffer of the plan's own: `in` is left alone, and `out` may be `in`
        const hipError_t e = hipMalloc(&c->sbuf, (size_t)p->max_count * elem_bytes(dtype));
        if (e != hipSuccess) return fail(DFFT_EHIP, fn + ": send buffer: " + hipGetErrorString(e));
    }
    const int mode = want_fused ? 1 : 2;
    DFFT_TRY(plan_create_impl(&c->f, n0, n1, n2, dtype, DFFT_FORWARD, in, c->sbuf, comm, global_idx, total_devices, DFFT_PLAN_INPUT_FROM_IN, mode));
    DFFT_TRY(plan_create_impl(&c->b, n0, n1, n2, dtype, DFFT_BACKWARD, c->f->buf1, p->out, comm, global_idx, total_devices, DFFT_PLAN_DEFAULT, mode));
    dfft_plan_s *f = c->f, *b = c->b;
    // one stream, one hand-over buffer
    (void)hipStreamSynchronize(b->stream);
    (void)hipStreamDestroy(b->stream);
    if (b->wbuf) (void)slab_free(b->wbuf);
    b->stream = f->stream;
    b->wbuf = f->wbuf;
    b->wl = f->wl;
    b->borrowed = true;
    p->stream = f->stream;
    p->device = f->device;
    p->exch = f->exch;
    if (f->exch != b->exch || f->rot_elems != b->rot_elems) return fail(DFFT_EINVAL, fn + ": internal: the two halves disagree about the exchange");
    ConvLaunch& L = c->L;
    L.dtype = dtype;
    L.n0 = (int)n0;
    L.ncols = n2;
    L.scale = 1.0;
    if (p->exch) {
        // the forward exchange's receive layout [x][yl][N2] IS the backward exchange's send layout (fill_exchange, uneven splits included):
        // the X stage works in place on the forward half's receive buffer and the backward half sends from it
        for (int q = 0; q < p->P; ++q)
            if (f->xd.roffset[q] != b->xd.soffset[q] || f->xd.rcount[q] != b->xd.scount[q])
                return fail(DFFT_EINVAL, fn + ": internal: forward receive pieces and backward send pieces differ");
        b->xd.sendbuf = f->buf1;
        L.in = L.out = f->buf1;
        L.plane = p->ys * n2;
        L.pitch = n2;
        L.rows = p->ys;
        L.rot = f->rot_elems;
        c->slab_elems = n0 * p->ys * n2;
    } else if (f->wbuf) {
        L.in = L.out = f->wbuf;
        L.plane = f->wl.plane;
        L.pitch = f->wl.pitch;
        L.rows = n1;
        c->slab_elems = p->xs * f->wl.plane;
    } else {  // natural layout: out of bufferDev1 of the forward half into the result buffer, where the inverse YZ stage works in place
        L.in = f->buf1;
        L.out = b->buf2;
        L.plane = n1 * n2;
        L.pitch = n2;
        L.rows = n1;
        c->slab_elems = n0 * n1 * n2;
    }
    c->fused = want_fused && conv_fused_applies(L);
    if (!c->fused && L.rot > 0) return fail(DFFT_EINVAL, fn + ": internal: rotated rows without the fused X stage");
    *plan = owner.release();
    return DFFT_OK;
}

// dfft_plan_create_conv_real (nout == 0: one output `out`, NULL or `in` for in place) and dfft_plan_create_conv_real_multi (nout >= 1
// outputs outs[0 .. nout))
static int conv_real_create(const std::string& fn, dfft_plan_t* plan, long long n0, long long n1, long long n2, int dtype, void* in, void* out,
                            void* const* outs, int nout, dfft_comm_t comm, int global_idx, int total_devices, unsigned flags) {
    if (!plan || !in) return fail(DFFT_EINVAL, fn + ": null plan/in");
    if (outs || nout) {
        if (!outs || nout < 1 || nout > DFFT_CONV_MAX_OUTPUTS)
            return fail(DFFT_EINVAL, fn + ": noutputs must be 1 .. " + std::to_string(DFFT_CONV_MAX_OUTPUTS) + " and outs not NULL");
        for (int k = 0; k < nout; ++k) {
            if (!outs[k]) return fail(DFFT_EINVAL, fn + ": outs[" + std::to_string(k) + "] is NULL");
            for (int q = 0; q < k; ++q)
                if (outs[q] == outs[k]) return fail(DFFT_EINVAL, fn + ": outs[" + std::to_string(q) + "] and outs[" + std::to_string(k) + "] are the same buffer");
        }
        out = outs[0];
    }
    DFFT_TRY(check_plan_args(fn, plan, in, out, n0, n1, n2, dtype, comm, global_idx, total_devices, flags, conv_arg_rules()));
    for (long long n : {n0, n1})
        if (length_kind(n) != 1)
            return fail(DFFT_EUNSUPPORTED, fn + ": FFT length " + std::to_string(n) + " -- N0 and N1 must be single-pass lengths (products of 2, 3, 5, 7 up to 4096)");
    if (!real_length_supported(n2))
        return fail(DFFT_EUNSUPPORTED, fn + ": N2 = " + std::to_string(n2) + " -- the real axis must be of dfft_real_form 1 (even, N2/2 a single-pass length)");
    const Slab sx = make_slab(n0, total_devices), sy = make_slab(n1, total_devices);
    if (sx.size(total_devices - 1) < 1 || sy.size(total_devices - 1) < 1) return fail(DFFT_EINVAL, fn + ": slab decomposition leaves the last device empty");
    const long long nh = n2 / 2 + 1, nc = conv_real_width(nh, dtype);
    const long long line = 128 / (long long)elem_bytes(dtype), pitch1 = (nc + line - 1) / line * line;
    if (std::max(conv_real_recv_count(n0, n1, nc, total_devices), sx.blk * n1 * pitch1) >= (1ll << 31))
        return fail(DFFT_EUNSUPPORTED, fn + ": more than 2^31 complex elements per device");
    if (dfft_device_count() < 1) return fail(DFFT_ENOGPU, fn + ": no HIP device visible (no CPU fallback)");

    const char* fe = getenv("DFFT_CONV_FUSED");  // A/B switch, read here once
    const bool  want_fused = !(fe && *fe == '0') && conv_fused_length((int)n0);
    trace("dfft_plan_create_conv_real", n0 * 1000000 + n1 * 1000 + n2 % 1000, total_devices * 100 + nout);
    // (N[2] is the REAL length -- 1 / (N0 N1 N2) in the filter copy; the halves carry the complex width)
    PlanOwner    owner(conv_new(n0, n1, n2, dtype, in, out, comm, global_idx, total_devices, flags));
    dfft_plan_s* p = owner.get();
    ConvState*   c = p->conv;
    c->real = true;
    c->nh = nh;
    c->nout = nout;
    p->max_count = p->xs * n1 * pitch1;
    const size_t cs = elem_bytes(dtype);
    if (total_devices > 1) {  // the forward half packs [d][xs][yl_d][Nc] into a send buffer of the plan's own
        const hipError_t e = hipMalloc(&c->sbuf, (size_t)total_devices * p->xs * sy.blk * nc * cs);
        if (e != hipSuccess) return fail(DFFT_EHIP, fn + ": send buffer: " + hipGetErrorString(e));
    }
    R2cHalf hf{nc, nullptr};
    DFFT_TRY(create_r2c(&c->f, n0, n1, n2, dtype, DFFT_FORWARD, in, c->sbuf, comm, global_idx, total_devices, DFFT_PLAN_INPUT_FROM_IN, false, &hf));
    R2cHalf hb{nc, c->f};
    DFFT_TRY(create_r2c(&c->b, n0, n1, n2, dtype, DFFT_BACKWARD, in, p->out, comm, global_idx, total_devices, DFFT_PLAN_DEFAULT, false, &hb));
    c->bk[0] = c->b;
    // outputs 1 .. K-1: a C2R half each, on the same stream.  P = 1: its intermediate (cleared once, like the forward half's) is slab k of
    // the X stage.  P > 1: it unpacks into the shared intermediate out of a receive buffer of its own and sends from slab k, a buffer of
    // the plan's in the received slab's layout [N0][y_local][Nc].
    for (int k = 1; k < nout; ++k) {
        R2cHalf hk{nc, c->f, k, total_devices == 1};
        DFFT_TRY(create_r2c(&c->bk[k], n0, n1, n2, dtype, DFFT_BACKWARD, in, outs[k], comm, global_idx, total_devices, DFFT_PLAN_DEFAULT, false, &hk));
        if (total_devices > 1) {
            const size_t     bytes = (size_t)(n0 * p->ys * nc) * cs;
            const hipError_t e = hipMalloc(&c->xslab[k], bytes);
            if (e != hipSuccess || hipMemset(c->xslab[k], 0, bytes) != hipSuccess) return fail(DFFT_EHIP, fn + ": slab of output " + std::to_string(k));
        }
    }
    dfft_plan_s *f = c->f, *b = c->b;
    p->stream = f->stream;
    p->device = f->device;
    p->exch = f->exch;
    ConvLaunch& L = c->L;
    L.dtype = dtype;
    L.n0 = (int)n0;
    L.ncols = nc;
    L.scale = 1.0;
    L.rot = 0;
    if (p->exch) {
        // as in dfft_plan_create_conv: the forward exchange's receive layout [x][yl][Nc] IS the backward exchange's send layout, so the X
        // stage works in place on the forward half's receive buffer and the backward half sends from it
        for (int q = 0; q < p->P; ++q)
            if (f->xd.roffset[q] != b->xd.soffset[q] || f->xd.rcount[q] != b->xd.scount[q])
                return fail(DFFT_EINVAL, fn + ": internal: forward receive pieces and backward send pieces differ");
        b->xd.sendbuf = f->buf1;
        L.in = L.out = f->buf1;
        L.plane = p->ys * nc;
        L.pitch = nc;
        L.rows = p->ys;
        c->slab_elems = n0 * p->ys * nc;
    } else {  // the intermediate [N0][N1][pitch], rows padded to whole lines
        L.in = L.out = f->cbuf;
        L.plane = f->cl.plane;
        L.pitch = f->cl.pitch;
        L.rows = n1;
        c->slab_elems = p->xs * f->cl.plane;
    }
    c->fused = want_fused && conv_fused_applies(L);
    if (nout > 0) {
        c->M.out[0] = const_cast<void*>(L.in);
        for (int k = 1; k < nout; ++k) {
            dfft_plan_s* bk = c->bk[k];
            if (p->exch) {
                for (int q = 0; q < p->P; ++q)
                    if (f->xd.roffset[q] != bk->xd.soffset[q] || f->xd.rcount[q] != bk->xd.scount[q])
                        return fail(DFFT_EINVAL, fn + ": internal: forward receive pieces and backward send pieces differ");
                bk->xd.sendbuf = c->xslab[k];
                c->M.out[k] = c->xslab[k];
            } else {
                if (bk->cl.plane != f->cl.plane || bk->cl.pitch != f->cl.pitch) return fail(DFFT_EINVAL, fn + ": internal: the slabs' layouts differ");
                c->M.out[k] = bk->cbuf;
            }
        }
        // the factor tables: ones (as long as the longest factor), then per output a | b (this device's rows) | c (Nc wide)
        c->fa = (n0 + 1) / 2 * 2;
        c->fb = (L.rows + 1) / 2 * 2;
        const long long ones = std::max({c->fa, c->fb, L.ncols}), total = ones + nout * (c->fa + c->fb + L.ncols);
        hipError_t      e = hipMalloc(&c->fact, (size_t)total * cs);
        if (e == hipSuccess) e = hipMemset(c->fact, 0, (size_t)total * cs);
        std::vector<char> host((size_t)ones * cs, 0);
        for (long long i = 0; i < ones; ++i) {
            if (dtype == DFFT_F64) reinterpret_cast<double*>(host.data())[2 * i] = 1.0;
            else reinterpret_cast<float*>(host.data())[2 * i] = 1.f;
        }
        if (e == hipSuccess) e = hipMemcpy(c->fact, host.data(), host.size(), hipMemcpyHostToDevice);
        if (e != hipSuccess) return fail(DFFT_EHIP, fn + ": factor tables: " + hipGetErrorString(e));
        for (int k = 0; k < nout; ++k) {
            c->M.ax[k] = c->M.by[k] = c->M.cz[k] = c->fact;
            c->unit[k] = true;
        }
        // the fused K-output kernel stores fp32 column pairs into every slab (16-byte accesses, like conv_fused_applies asks of L.in)
        for (int k = 0; k < nout && dtype == DFFT_F32; ++k)
            if ((uintptr_t)c->M.out[k] & 15) c->fused = false;
    }
    *plan = owner.release();
    return DFFT_OK;
}

int dfft_plan_create_conv_real(dfft_plan_t* plan, long long n0, long long n1, long long n2, int dtype, void* in, void* out, dfft_comm_t comm,
                               int global_idx, int total_devices, unsigned flags) {
    return conv_real_create("dfft_plan_create_conv_real", plan, n0, n1, n2, dtype, in, out, nullptr, 0, comm, global_idx, total_devices, flags);
}

int dfft_plan_create_conv_real_multi(dfft_plan_t* plan, long long n0, long long n1, long long n2, int dtype, void* in, void* const* outs,
                                     int noutputs, dfft_comm_t comm, int global_idx, int total_devices, unsigned flags) {
    if (!outs) return fail(DFFT_EINVAL, "dfft_plan_create_conv_real_multi: outs is NULL");
    if (noutputs < 1 || noutputs > DFFT_CONV_MAX_OUTPUTS)
        return fail(DFFT_EINVAL, "dfft_plan_create_conv_real_multi: noutputs must be 1 .. " + std::to_string(DFFT_CONV_MAX_OUTPUTS));
    if (!plan || !in) return fail(DFFT_EINVAL, "dfft_plan_create_conv_real_multi: null plan/in");
    return conv_real_create("dfft_plan_create_conv_real_multi", plan, n0, n1, n2, dtype, in, nullptr, outs, noutputs, comm, global_idx,
                            total_devices, flags);
}

// The separable factors of output k (device pointers to the plan's complex type; NULL: ones): ax[N0], ay[N1] -- the whole vector, the
// plan takes rows y0 .. y0 + y_local --, az[N2/2 + 1].  Private copies; az zero-padded to the plan's width.
int dfft_conv_set_factors(dfft_plan_t plan, int k, const void* ax, const void* ay, const void* az) {
    if (!plan || !plan->conv || plan->conv->nout < 1) return fail(DFFT_EINVAL, "dfft_conv_set_factors: not a multi-output spectral-filter plan");
    ConvState* c = plan->conv;
    if (k < 0 || k >= c->nout) return fail(DFFT_EINVAL, "dfft_conv_set_factors: output " + std::to_string(k) + " of " + std::to_string(c->nout));
    DFFT_HIP_TRY(hipDeviceSynchronize());  // whatever stream produced the vectors, and this plan's executes that read the old tables
    const size_t    cs = elem_bytes(plan->dtype);
    const long long ones = std::max({c->fa, c->fb, c->L.ncols}), per = c->fa + c->fb + c->L.ncols;
    char* const     ta = (char*)c->fact + (size_t)(ones + k * per) * cs;
    char* const     tb = ta + (size_t)c->fa * cs;
    char* const     tc = tb + (size_t)c->fb * cs;
    if (ax) DFFT_HIP_TRY(hipMemcpyAsync(ta, ax, (size_t)plan->N[0] * cs, hipMemcpyDeviceToDevice, plan->stream));
    if (ay)
        DFFT_HIP_TRY(hipMemcpyAsync(tb, (const char*)ay + (size_t)plan->sy.start(plan->me) * cs, (size_t)plan->ys * cs, hipMemcpyDeviceToDevice,
                                    plan->stream));
    if (az) {
        DFFT_HIP_TRY(hipMemsetAsync(tc, 0, (size_t)c->L.ncols * cs, plan->stream));
        DFFT_HIP_TRY(hipMemcpyAsync(tc, az, (size_t)c->nh * cs, hipMemcpyDeviceToDevice, plan->stream));
    }
    DFFT_HIP_TRY(hipStreamSynchronize(plan->stream));
    c->M.ax[k] = ax ? ta : c->fact;
    c->M.by[k] = ay ? tb : c->fact;
    c->M.cz[k] = az ? tc : c->fact;
    c->unit[k] = !ax && !ay && !az;
    return DFFT_OK;
}

static int conv_check_handle(dfft_plan_t plan, const char* fn) {
    if (!plan || !plan->conv) return fail(DFFT_EINVAL, std::string(fn) + ": not a spectral-filter plan");
    return DFFT_OK;
}

int dfft_conv_set_filter(dfft_plan_t plan, const void* h, int kind) {
    DFFT_TRY(conv_check_handle(plan, "dfft_conv_set_filter"));
    if (!h || (kind != DFFT_FILTER_COMPLEX && kind != DFFT_FILTER_REAL)) return fail(DFFT_EINVAL, "dfft_conv_set_filter: null filter or bad kind");
    ConvState* c = plan->conv;
    DFFT_HIP_TRY(hipDeviceSynchronize());  // whatever stream produced `h`, and this plan's executes that read the old copy
    DFFT_TRY(conv_alloc_filter(plan, kind));
    ConvLaunch R = c->L;
    R.filter_real = kind == DFFT_FILTER_REAL;
    R.scale = plan->scale / ((double)plan->N[0] * (double)plan->N[1] * (double)plan->N[2]);
    if (c->real) DFFT_TRY(check_launch(launch_conv_real_relayout(R, c->nh, h, c->filt, plan->stream), "dfft_conv_set_filter: re-layout"));
    else DFFT_TRY(check_launch(launch_conv_relayout(R, h, c->filt, plan->stream), "dfft_conv_set_filter: re-layout"));
    DFFT_HIP_TRY(hipStreamSynchronize(plan->stream));
    c->kind = kind;
    return DFFT_OK;
}

int dfft_conv_set_kernel(dfft_plan_t plan, const void* k) {
    DFFT_TRY(conv_check_handle(plan, "dfft_conv_set_kernel"));
    if (!k) return fail(DFFT_EINVAL, "dfft_conv_set_kernel: null kernel");
    ConvState* c = plan->conv;
    DFFT_HIP_TRY(hipDeviceSynchronize());
    int arc = conv_alloc_filter(plan, DFFT_FILTER_COMPLEX);
    if (arc && !plan->exch) return arc;
    // the plan's own forward half on `k` (collective like an execute), then the forward X transform of the slab it leaves, times
    // scale / N, straight into the filter copy: the slab's layout is the copy's
    void* const user_in = c->f->in;
    c->f->in = const_cast<void*>(k);
    int rc = dfft_execute(c->f, DFFT_EXEC_NO_TIMING);
    c->f->in = user_in;
    if (!rc) rc = arc;
    if (!rc) rc = conv_x_stage(plan, true, plan->scale / ((double)plan->N[0] * (double)plan->N[1] * (double)plan->N[2]));
    if (rc) return rc;
    DFFT_TRY(conv_sync(plan));
    c->kind = DFFT_FILTER_COMPLEX;
    return DFFT_OK;
}

}  // extern "C"
