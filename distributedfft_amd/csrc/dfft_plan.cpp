// dfft_plan.cpp -- C2C slab plans behind the C-ABI (include/dfft.h): create, the t0..t3 execute sequences, describe / sync / times /
// destroy.  The plan object and what the other host units share with this one: dfft_plan_impl.h.
//
// Reference being replaced (behaviour, not code): /root/reference/3dmpifft_opt/include/fft_mpi_3d_api.cpp
//   fft_mpi_init :3-39, fft_mpi_plan_dft_c2c_3d :41-141, fft_mpi_destroy_plan :143-179,
//   fft_mpi_execute_dft_3d_c2c :181-214, getProperDeviceNum :232-272, getDataCountForNode :274-287,
//   getMaxDataCount :289-316, fftZY :466-522, fftX :524-573, localTransposeUneven :575-608, slabAlltoall :610-672.
//
// MI355X-first differences (DESIGN.md has the full list):
//   * t0 is two launches over the WHOLE slab (Z rows, Y columns), not 2*xl per-plane launches;
//   * fused mode: the Y pass stores straight into the packed [dest][xl][yl][N2] send layout (t1 disappears) and the
//     X pass loads [x][yl][N2] column tiles and stores [yl][N2][kx] (the 16x16 tile transpose disappears):
//     6*S bytes per element of HBM traffic for the local pipeline instead of the reference's 10*S;
//   * P == 1 short-circuits the exchange (the reference does a full-size self copy);
//   * everything is enqueued on one HIP stream, stage boundaries are HIP events; host-blocking per-stage timing is
//     opt-in (DFFT_EXEC_SYNC_STAGES) for drop-in comparability with the reference's MPI_Wtime brackets.
#include <cstdio>
#include <numeric>

#include "dfft_plan_impl.h"

namespace dfft {

int fill_exchange(dfft_plan_s* p, ExchangeDesc& x, int direction) {
    const int       P = p->P, me = p->me;
    const long long n2 = p->N[2];
    x.dtype = p->dtype;
    x.direction = direction;
    x.P = P;
    x.me = me;
    x.scount.assign(P, 0);
    x.soffset.assign(P, 0);
    x.rcount.assign(P, 0);
    x.roffset.assign(P, 0);
    x.doffset.assign(P, 0);
    x.xsize.assign(P, 0);
    x.ysize.assign(P, 0);
    x.n2 = n2;
    for (int q = 0; q < P; ++q) {
        x.xsize[q] = p->sx.size(q);
        x.ysize[q] = p->sy.size(q);
    }
    for (int q = 0; q < P; ++q) {
        if (direction == DFFT_FORWARD) {
            // chunk(me -> q) = x in me's slab, y in q's slab          
            x.scount[q] = p->sx.size(me) * p->sy.size(q) * n2;
            x.soffset[q] = (long long)q * p->sx.size(me) * p->sy.blk * n2;   // packed [d][xl][yl_d][N2]
            x.rcount[q] = p->sx.size(q) * p->sy.size(me) * n2;
            x.roffset[q] = p->sx.start(q) * p->sy.size(me) * n2;              // [x][yl_me][N2], x = q*xl + xi
            x.doffset[q] = p->sx.start(me) * p->sy.size(q) * n2;
        } else {
            // chunk(me -> q) = x in q's slab, y in me's slab
            x.scount[q] = p->sx.size(q) * p->sy.size(me) * n2;
            x.soffset[q] = p->sx.start(q) * p->sy.size(me) * n2;
            x.rcount[q] = p->sx.size(me) * p->sy.size(q) * n2;
            x.roffset[q] = (long long)q * p->sx.size(me) * p->sy.blk * n2;
            x.doffset[q] = (long long)me * p->sx.size(q) * p->sy.blk * n2;
        }
    }
    return DFFT_OK;
}

// The packed side of the Y pass: [d][xs][yl_d][N2]; with Y sub-blocks (ycuts > 1, even X and Y splits only) [k][d][xs][yl/ycuts][N2]:
// sub-block k of the send buffer is exactly the region the X pass of sub-block k overwrites with its result, so a result never
// lands on send data that is still in flight (execute_forward).  tile->a_stride = distance between consecutive X planes in a block.
static void packed_map(const dfft_plan_s* p, AxisMap* packed, TileMap* tile) {
    const long long n2 = p->N[2];
    const long long ysub = p->sy.blk / p->ycuts;
    packed->blk = (int)ysub;
    packed->nblk = p->P * p->ycuts;
    packed->blk_stride = p->xs * ysub * n2;
    packed->sub = p->ycuts;
    packed->sub_stride = (long long)p->P * p->xs * ysub * n2;
    packed->stride = n2;
    packed->cstride = 1;
    packed->last_delta = p->ycuts > 1 ? 0 : (p->sy.size(p->P - 1) - p->sy.blk) * n2;
    *tile = TileMap{ysub * n2, 1};
}

int launch_y(dfft_plan_s* p, const void* in, void* out, bool packed_side_is_out, bool use_packed, long long x0, long long nx, int hints,
             const SlabLayout* lay_in, const SlabLayout* lay_out) {
    const int       n1 = (int)p->N[1];
    const long long n2 = p->N[2];
    if (length_kind(n1) == 3) {  // Bluestein: natural layout on both sides only (such plans run un-fused)
        auto natural = [&](const SlabLayout* l) { return !l || (l->pitch == n2 && l->plane == (long long)n1 * n2); };
        if (use_packed || !natural(lay_in) || !natural(lay_out)) return fail(DFFT_EINVAL, "Y pass: a Bluestein axis needs the natural layout");
        const size_t off = (size_t)x0 * n1 * n2 * elem_bytes(p->dtype);
        return bluestein_pass((const char*)in + off, (char*)out + off, n1, n2, nx, p->dtype, p->direction, 1.0, p->stream);
    }
    if (n1 > 4096) {  // four-step form: natural layout on both sides only (long-axis plans run un-fused)
        auto natural = [&](const SlabLayout* l) { return !l || (l->pitch == n2 && l->plane == (long long)n1 * n2); };
        if (use_packed || !natural(lay_in) || !natural(lay_out)) return fail(DFFT_EINVAL, "Y pass: a long axis needs the natural layout");
        const size_t off = (size_t)x0 * n1 * n2 * elem_bytes(p->dtype);
        return long_fft((const char*)in + off, (char*)out + off, n1, n2, nx, p->dtype, p->direction, 1.0, p->lbuf, p->stream);
    }
    const void*     tw = nullptr;
    int             rc = get_twiddles(n1, p->dtype, &tw);
    if (rc) return rc;
    FftLaunch L;
    std::memset(&L, 0, sizeof(L));
    L.dtype = p->dtype;
    L.n = n1;
    L.dir = p->direction;
    L.cols = 1;
    L.in = in;
    L.out = out;
    L.tw = tw;
    const SlabLayout nat{n2, (long long)n1 * n2};
    const SlabLayout li = lay_in ? *lay_in : nat, lo = lay_out ? *lay_out : nat;
    AxisMap packed;
    TileMap pk_tile;
    packed_map(p, &packed, &pk_tile);
    L.imap = plain_axis(n1, li.pitch, 1);
    L.itile = TileMap{li.plane, 1};
    L.omap = plain_axis(n1, lo.pitch, 1);
    L.otile = TileMap{lo.plane, 1};
    if (use_packed) {
        if (packed_side_is_out) {
            L.omap = packed;
            L.otile = pk_tile;
        } else {
            L.imap = packed;
            L.itile = pk_tile;
        }
    }
    L.na = nx;
    L.a_first = x0;
    L.hints = hints;
    L.ncols = (int)n2;
    if (use_packed && p->rot_elems > 0) {  // the packed side's rows are rotated by the plane's global index
        L.rot.rot = p->rot_elems;
        L.rot.mask = (int)n2 - 1;
        L.rot.a0 = (int)p->sx.start(p->me);
        (packed_side_is_out ? L.rot.out_mode : L.rot.in_mode) = 1;
    }
    L.grid_limit = p->grid_y;
    return check_launch(launch_fft(L, p->stream), "Y pass");
}

int launch_x(dfft_plan_s* p, const void* in, void* out, bool keep_slab, long long ys_part, const SlabLayout* slab_lay) {
    const int       n0 = (int)p->N[0];
    const long long n2 = p->N[2];
    const long long ys = ys_part > 0 ? ys_part : p->ys;
    const void*     tw = nullptr;
    int             rc = get_twiddles(n0, p->dtype, &tw);
    if (rc) return rc;
    FftLaunch L;
    std::memset(&L, 0, sizeof(L));
    L.dtype = p->dtype;
    L.n = n0;
    L.dir = p->direction;
    L.cols = 1;
    L.in = in;
    L.out = out;
    L.tw = tw;
    AxisMap slab = plain_axis(n0, slab_lay ? slab_lay->plane : ys * n2, 1);
    TileMap slab_tile{slab_lay ? slab_lay->pitch : n2, 1};
    AxisMap tr = plain_axis(n0, 1, n0);
    TileMap tr_tile{n2 * (long long)n0, (long long)n0};
    if (keep_slab) {
        L.imap = L.omap = slab;
        L.itile = L.otile = slab_tile;
    } else if (p->direction == DFFT_FORWARD) {
        L.imap = slab;
        L.itile = slab_tile;
        L.omap = tr;
        L.otile = tr_tile;
    } else {
        L.imap = tr;
        L.itile = tr_tile;
        L.omap = slab;
        L.otile = slab_tile;
    }
    L.na = ys;
    L.scale = p->scale;
    L.ncols = (int)n2;
    if (p->rot_elems > 0 && p->exch && !keep_slab && !slab_lay) {  // the slab side is an exchange buffer with rotated rows
        L.rot.rot = p->rot_elems;
        L.rot.mask = (int)n2 - 1;
        (p->direction == DFFT_FORWARD ? L.rot.in_mode : L.rot.out_mode) = 2;
    }
    L.grid_limit = p->grid_x;
    L.hints |= p->x_hints;
    if (p->x_ticket_ctr && ys_part <= 0 && !keep_slab) {  // whole-slab launches draw their tiles from the plan's counter (dfft_plan_impl.h)
        L.x_ticket = p->x_ticket_ctr;
        L.x_ticket_base = &p->x_ticket;
    }
    if (ys_part <= 0) {
        p->x_form = 0;
        L.x_form = &p->x_form;
    }
    return check_launch(launch_fft(L, p->stream), "X pass");
}

int StageClock::begin() {
    if (sync) {
        DFFT_HIP_TRY(hipStreamSynchronize(p->stream));
        t = std::chrono::steady_clock::now();
    } else if (p->timed) {
        DFFT_HIP_TRY(hipEventRecord(p->ev[0], p->stream));
    }
    return DFFT_OK;
}
int StageClock::end_stage() {
    if (sync) {
        DFFT_HIP_TRY(hipStreamSynchronize(p->stream));
        auto now = std::chrono::steady_clock::now();
        p->host_t[idx] = std::chrono::duration<double>(now - t).count();
        t = now;
    } else if (p->timed) {
        DFFT_HIP_TRY(hipEventRecord(p->ev[idx + 1], p->stream));
    }
    ++idx;
    return DFFT_OK;
}

// Planes per phase of the one-launch YZ stage for a slab (or part) of nx planes: one that fits the 256 MiB Infinity Cache is ONE
// phase; larger ones are cut into equal phases of at most 230 MiB -- head-room instead of the largest possible size, see
// dfft_plan_create; a short last phase costs more than it saves.  DFFT_CHUNK_PLANES overrides.
// Forward PACKED launches (P > 1: the column units stream their results into the send buffer, so a phase is only READ from the cache) fill
// the cache instead -- 256 MiB: every phase boundary costs about 30 us of a rank's stage whatever the phase size (per rank at 512^3 fp64,
// P = 4, 128 planes: 2 phases of 64 planes 0.304 ms, 3 x 43 0.319, 4 x 32 0.394, 8 x 16 0.50, one phase of 512 MiB 0.377;
// profiles/r06/experiments/packed_phase_curve_512_P4.log), so fewer phases win as long as one still fits: 512^3 per rank at P = 2
// 5 x 52 -> 4 x 64 planes 0.597 -> 0.579 ms, at P = 4 3 x 43 -> 2 x 64 0.312 -> 0.300; config 4 at P = 2 14 -> 13 phases 2.03 -> 1.98.
// (What a boundary costs is the window in which row and column units run side by side: an interleaved ticket order -- rows of phase s
// alternating plane by plane with the columns of phase s - 1, no boundaries at all -- was built and measured at 0.335-0.46 ms against 0.309
// there, 1.42-1.82 against 1.155 on one GPU; profiles/r06/experiments/zy_interleaved_order.log.  Homogeneous phases, as few as fit.)
static long long zy_phase_planes(const dfft_plan_s* p, long long nx, bool packed_fwd = false) {
    static const long long forced = [] {
        const char* e = getenv("DFFT_CHUNK_PLANES");
        return e ? atoll(e) : 0ll;
    }();
    const long long plane_b = p->N[1] * p->N[2] * (long long)elem_bytes(p->dtype);
    if (forced > 0) return std::min(forced, nx);
    if (nx * plane_b <= (256ll << 20)) return nx;
    const long long fit = std::max(1ll, ((packed_fwd ? 256ll : 230ll) << 20) / plane_b), nch = (nx + fit - 1) / fit;
    return (nx + nch - 1) / nch;
}

// t0 (or its inverse) of planes [x0, x0 + nx) as one launch (dfft_zy.hip).
//   forward : Z rows src -> w, Y columns w -> w in place, or (packed) w -> the packed send layout in `other`
//   backward: Y columns w -> w in place, or (packed) the packed receive layout in `other` -> w; then Z rows w -> dst
// structure: 0 = the plan's direction; +1 on a backward plan = the inverse stage rows first (src = the hand-over buffer, w = the result buffer)
static int launch_zy_stage(dfft_plan_s* p, const void* src, void* w, long long w_plane, void* dst, void* other, bool packed, long long x0,
                           long long nx, int structure = 0, bool sig = false) {
    if (nx <= 0) return DFFT_OK;
    const void *twz = nullptr, *twy = nullptr;
    DFFT_TRY(get_twiddles((int)p->N[2], p->dtype, &twz));
    DFFT_TRY(get_twiddles((int)p->N[1], p->dtype, &twy));
    ZyLaunch L;
    std::memset(&L, 0, sizeof(L));
    L.dtype = p->dtype;
    L.n1 = (int)p->N[1];
    L.n2 = (int)p->N[2];
    L.dir = structure ? structure : p->direction;
    L.sign = p->direction;
    L.src = src;
    L.w = w;
    L.dst = dst;
    L.src_plane = L.dst_plane = p->N[1] * p->N[2];
    if (structure > 0 && p->direction < 0) L.src_plane = p->wl.plane;  // rows read the (plane-padded) hand-over buffer
    L.w_plane = w_plane;
    L.plane0 = x0;
    L.nplanes = nx;
    L.chunk = zy_phase_planes(p, nx, packed && p->direction == DFFT_FORWARD);
    L.ctl = p->zy_ctl;
    L.twz = twz;
    L.twy = twy;
    L.lazy = p->zy_lazy ? 1 : 0;
    L.spin_polls = p->zy_spin_polls;
    if (hipHostGetDevicePointer((void**)&L.err_host, p->zy_err, 0) != hipSuccess) return fail(DFFT_EHIP, "one-launch YZ stage: no device pointer for the error word");
    if (packed) {
        TileMap tile;
        packed_map(p, &L.pk, &tile);
        L.packed = 1;
        L.pk_plane = tile.a_stride;
        if (p->direction == DFFT_FORWARD) L.dst = other;
        else L.src = other;
        if (p->rot_elems > 0) {
            L.rot.rot = p->rot_elems;
            L.rot.mask = (int)p->N[2] - 1;
            L.rot.a0 = (int)p->sx.start(p->me);
        }
    }
    // the control block's counters run on from launch to launch (no reset between transforms): the ticket counter by what every
    // launch consumes, the per-plane counters by the producers of one plane per execute
    unsigned producers = 0;
    (void)zy_units_per_plane(L.n1, L.n2, L.dir, L.packed, &producers);
    if (x0 == 0) p->zy_cur = p->zy_execs++;
    L.ticket_base = p->zy_ticket;
    L.done_base = p->zy_cur * producers;
    if (sig) {  // whole-slab launch of the overlapped pipeline: count finished column units per X-plane part
        L.part_done = p->zy_part_done;
        L.part_planes = p->part_planes;
    }
    if (p->zy_fault > 0 && ++p->zy_launches == (unsigned)p->zy_fault) L.fault = 1;  // test hook: this launch's consumers can never start
    p->zy_ticket += zy_tickets(L.n1, L.n2, L.dir, L.packed, L.nplanes, L.chunk);
    return check_launch(launch_zy(L, p->stream), "one-launch YZ stage");
}

// Did a launch of the one-launch stage give up (a consumer unit exhausted its polls, or a launch found the control block's counters
// out of step)?  The kernel writes the reason to a pinned host word, so this costs one host load and can run anywhere -- before
// an execute is queued, after a drained one, in sync / stage_times / destroy.  The word is sticky on the device side (every later
// launch on the block returns at once), so nothing computed after the failure can pass for a result; the stage is switched off for
// good here and the plan continues on two launches per chunk.
int zy_check(dfft_plan_s* p) {
    if (!p->zy_on || !p->zy_err) return DFFT_OK;
    const unsigned err = *(volatile unsigned*)p->zy_err;
    if (err == 0) return DFFT_OK;
    p->zy_on = false;  // two launches per chunk from now on
    return fail(DFFT_EHIP, std::string("the one-launch YZ stage gave up (") +
                               (err == ZY_ERR_TIMEOUT ? "a column / row unit exhausted its polls waiting for its plane's producers"
                                                      : "its ticket counter was out of step with the host's") +
                               "); the results of that execute and of every execute queued behind it are invalid, later executes of this plan "
                               "use the two-launch stage (DFFT_T0_ONE_LAUNCH=0 selects it from the start)");
}

static int execute_forward(dfft_plan_s* p, bool sync) {
    const bool      fused = !(p->flags & DFFT_PLAN_UNFUSED);
    const long long n1 = p->N[1], n2 = p->N[2], n0 = p->N[0];
    StageClock      clk{p, sync};
    DFFT_TRY(clk.begin());
    // ---- t0: 2D YZ FFT of every owned plane ----
    // The Z and Y passes run chunk by chunk over groups of planes that fit the 256 MiB Infinity Cache, so the Y pass
    // reads what the Z pass just wrote from cache instead of HBM (measured 1.73 -> 1.31..1.44 ms at 512^3 fp64).
    const void*     zsrc = (p->flags & DFFT_PLAN_INPUT_FROM_IN) ? p->in : p->buf1;
    const bool      y_packs = fused && p->exch;
    // where the Z pass puts its rows for the Y pass: the padded work buffer when the plan has one (fused pipelines)
    const SlabLayout nat{n2, n1 * n2};
    void*            zdst = (fused && p->wbuf) ? p->wbuf : p->buf1;
    const SlabLayout zl = (fused && p->wbuf) ? p->wl : nat;
    const SlabLayout *lz = (fused && p->wbuf) ? &zl : nullptr, *lnat = lz ? &nat : nullptr;  // row launches: layouts only when padded
    if (y_packs && (p->flags & DFFT_PLAN_OVERLAP) && p->part_planes > 0) {
        // ---- t0 pipelined against t2: the exchange of plane part k (stream2) runs while the Z+Y passes of part k+1
        // (stream) compute.  Any X-plane sub-range of the packed send layout is contiguous on both sides, so the parts
        // need no extra packing (dfft_exchange.cpp).  All ranks cut their slabs with the same part size.
        const bool rccl = comm_is_async(p->comm);
        const int  K = (int)((p->sx.blk + p->part_planes - 1) / p->part_planes);
        const int  YK = p->ycuts;
        // One launch of the YZ stage for ALL parts (round 6): the phases of the serial plan, no launch boundary and no 32-plane phase
        // per part; the stage counts, per part, the column units whose results are in memory, and the exchange stream waits for a
        // part's count (zy_part_wait_kernel) instead of an event behind a per-part launch.
        const bool one_for_all = p->zy_on && p->zy_part_done != nullptr;
        unsigned   sig_exec = 0, sig_units = 0;
        if (one_for_all) {
            unsigned producers = 0;
            sig_units = zy_units_per_plane((int)n1, (int)n2, +1, 1, &producers) - producers;  // column units per plane
            sig_exec = p->zy_sig_execs++;
            DFFT_TRY(launch_zy_stage(p, zsrc, zdst, zl.plane, nullptr, p->buf2, true, 0, p->xs, 0, true));
        }
        for (int k = 0; k < K; ++k) {
            long long x0, nx;
            part_range(p->xs, p->part_planes, k, &x0, &nx);
            if (one_for_all) {
                // (nothing to launch: the part is being computed by the launch above)
            } else if (nx > 0 && p->zy_on) {  // Z rows + packing Y columns of the part in one launch
                DFFT_TRY(launch_zy_stage(p, zsrc, zdst, zl.plane, nullptr, p->buf2, true, x0, nx));
            } else if (nx > 0) {
                DFFT_TRY(fft_rows(zsrc, zdst, (int)n2, nx * n1, p->dtype, p->direction, p->stream, x0 * n1,
                                  zsrc != zdst ? FFT_HINT_STREAM_IN : 0, 1.0, lnat, lz, lz ? n1 : 0));
                DFFT_TRY(launch_y(p, zdst, p->buf2, true, true, x0, nx, FFT_HINT_STREAM_OUT, &zl));
            }
            hipStream_t xs_ = rccl ? p->stream2 : p->stream;  // LOCAL: host-synchronising, same call sequence
            if (rccl && one_for_all) {
                // every execute adds nx * sig_units to the part's counter (all executes of a plan cut the same parts)
                unsigned* errw = nullptr;
                if (hipHostGetDevicePointer((void**)&errw, p->zy_err, 0) != hipSuccess) return fail(DFFT_EHIP, "one-launch YZ stage: no device pointer for the error word");
                // (no event between the streams: the wait kernel polls the counter, and the count can only be reached by THIS execute's
                // launch, which runs behind the previous execute's X pass on p->stream)
                if (nx > 0)
                    DFFT_TRY(check_launch(launch_zy_part_wait(p->zy_part_done + k, (sig_exec + 1u) * (unsigned)nx * sig_units, p->zy_ctl, errw, p->stream2),
                                          "part wait of the one-launch YZ stage"));
            } else if (rccl) {
                DFFT_HIP_TRY(hipEventRecord(p->part_ev[k], p->stream));
                DFFT_HIP_TRY(hipStreamWaitEvent(p->stream2, p->part_ev[k], 0));
            }
            if (k + 1 < K || YK == 1) {
                DFFT_TRY(comm_exchange_part(p->comm, p->xd, k, p->part_planes, xs_));
            } else {
                // last part: one exchange per Y sub-block, so the X pass can start on sub-block 0 while the others fly
                for (int y = 0; y < YK; ++y) {
                    DFFT_TRY(comm_exchange_part(p->comm, p->xd, k, p->part_planes, xs_, y));
                    if (rccl) DFFT_HIP_TRY(hipEventRecord(p->y_ev[y], p->stream2));
                }
            }
        }
        DFFT_TRY(clk.end_stage());
        DFFT_TRY(clk.end_stage());  // t1 folded into t0
        if (YK == 1) {
            if (rccl) {
                DFFT_HIP_TRY(hipEventRecord(p->join_ev, p->stream2));
                DFFT_HIP_TRY(hipStreamWaitEvent(p->stream, p->join_ev, 0));
            }
            DFFT_TRY(clk.end_stage());  // t2 = the part of the exchange that was not hidden behind t0
            DFFT_TRY(launch_x(p, p->rbuf, p->buf2));
        } else {
            // t3 pipelined against the tail of t2: sub-block y of the receive buffer is a complete [N0][ysub][N2] slab
            const long long ysub = p->ys / YK;
            const size_t    sub = (size_t)n0 * ysub * n2 * elem_bytes(p->dtype);
            for (int y = 0; y < YK; ++y) {
                if (rccl) DFFT_HIP_TRY(hipStreamWaitEvent(p->stream, p->y_ev[y], 0));
                if (y == 0) DFFT_TRY(clk.end_stage());  // t2 = exposed wait for the first sub-block
                DFFT_TRY(launch_x(p, (const char*)p->rbuf + y * sub, (char*)p->buf2 + y * sub, false, ysub));
            }
        }
        DFFT_TRY(clk.end_stage());
        return DFFT_OK;
    }
    const long long cp = p->chunk_planes > 0 ? p->chunk_planes : p->xs;
    // streaming hints whenever the stage works on cache-sized pieces of a slab too big to be cache-resident as a whole
    const bool      chunked = cp < p->xs || p->xs * n1 * n2 * (long long)elem_bytes(p->dtype) >= (64ll << 20);
    const bool      one_launch = p->zy_on && fused;
    if (one_launch) {  // the same chunk phases inside ONE persistent launch (dfft_zy.hip); P > 1: the Y side packs into the send buffer
        DFFT_TRY(launch_zy_stage(p, zsrc, zdst, zl.plane, nullptr, y_packs ? p->buf2 : nullptr, y_packs, 0, p->xs));
    }
    for (long long x0 = 0; !one_launch && x0 < p->xs; x0 += cp) {
        const long long nx = std::min(cp, p->xs - x0);
        DFFT_TRY(fft_rows(zsrc, zdst, (int)n2, nx * n1, p->dtype, p->direction, p->stream, x0 * n1,
                          (chunked && zsrc != zdst) ? FFT_HINT_STREAM_IN : 0, 1.0, lnat, lz, lz ? n1 : 0));
        if (!sync && p->timed && cp >= p->xs) DFFT_HIP_TRY(hipEventRecord(p->ev[5], p->stream));
        if (y_packs) DFFT_TRY(launch_y(p, zdst, p->buf2, true, true, x0, nx, chunked ? FFT_HINT_STREAM_OUT : 0, &zl));  // Y FFT + pack in one pass
        else DFFT_TRY(launch_y(p, zdst, zdst, true, false, x0, nx, 0, &zl, &zl));
    }
    if (y_packs) {
        DFFT_TRY(clk.end_stage());
        DFFT_TRY(clk.end_stage());  // t1 folded into t0
    } else {
        DFFT_TRY(clk.end_stage());
        // ---- t1: pack ----
        if (!fused) {
            hipError_t e = launch_pack(p->dtype, +1, p->buf1, p->buf2, (int)p->xs, (int)n1, (int)n2, (int)p->sy.blk,
                                       (int)p->sy.size(p->P - 1), p->P, p->stream);
            if (e != hipSuccess) return fail(DFFT_EHIP, std::string("pack: ") + hipGetErrorString(e));
        }
        DFFT_TRY(clk.end_stage());
    }
    // ---- t2: exchange ----
    const void* xsrc = p->exch ? p->buf1 : zdst;  // single GPU: the X pass reads what the Y pass left (possibly padded)
    if (p->exch) {
        DFFT_TRY(comm_exchange(p->comm, p->xd, p->stream));
    } else if (!fused) {
        // reference structure: full-size self copy bufferDev2 -> bufferDev1 (fft_mpi_3d_api.cpp:613-630)
        DFFT_HIP_TRY(hipMemcpyAsync(p->buf1, p->buf2, (size_t)p->xs * n1 * n2 * elem_bytes(p->dtype),
                                    hipMemcpyDeviceToDevice, p->stream));
    }
    DFFT_TRY(clk.end_stage());
    // ---- t3: X FFT (+ transpose to [yl][N2][N0]) ----
    if (p->conv_half) {
        // (spectral-filter plans: the X stage works in place on what t0 / t2 left -- dfft_conv.hip, conv_x_stage)
    } else if (fused) {
        DFFT_TRY(launch_x(p, xsrc, p->buf2, false, 0, (!p->exch && p->wbuf) ? &zl : nullptr));
    } else {
        hipError_t e = launch_transpose(p->dtype, p->buf1, p->buf2, n0, p->ys * n2, p->stream);
        if (e != hipSuccess) return fail(DFFT_EHIP, std::string("transpose: ") + hipGetErrorString(e));
        DFFT_TRY(fft_rows(p->buf2, p->buf2, (int)n0, p->ys * n2, p->dtype, p->direction, p->stream, 0, 0, p->scale));
    }
    DFFT_TRY(clk.end_stage());
    return DFFT_OK;
}

// DFFT_PLAN_NATURAL: input AND output are the caller's natural X-slab layout [xs][N1][N2] (the un-transposed output the
// reference declares but never implements, fft_mpi_local_size_3d / SURVEY 8f-2).  The same sequence serves both
// directions (the kernels take the sign): Z, Y(+pack) | exchange X->Y | X in slab layout | exchange Y->X | unpack.
static int execute_natural(dfft_plan_s* p, bool sync) {
    const long long n1 = p->N[1], n2 = p->N[2];
    StageClock      clk{p, sync};
    DFFT_TRY(clk.begin());
    const void*     zsrc = (p->flags & DFFT_PLAN_INPUT_FROM_IN) ? p->in : p->buf1;
    const long long cp = p->chunk_planes > 0 ? p->chunk_planes : p->xs;
    const bool      hinted = cp < p->xs || p->xs * n1 * n2 * (long long)elem_bytes(p->dtype) >= (64ll << 20);
    for (long long x0 = 0; x0 < p->xs; x0 += cp) {
        const long long nx = std::min(cp, p->xs - x0);
        DFFT_TRY(fft_rows(zsrc, p->buf1, (int)n2, nx * n1, p->dtype, p->direction, p->stream, x0 * n1,
                          (hinted && zsrc != p->buf1) ? FFT_HINT_STREAM_IN : 0));
        if (p->exch) DFFT_TRY(launch_y(p, p->buf1, p->buf2, true, true, x0, nx, hinted ? FFT_HINT_STREAM_OUT : 0));
        else DFFT_TRY(launch_y(p, p->buf1, p->buf1, true, false, x0, nx));
    }
    DFFT_TRY(clk.end_stage());
    DFFT_TRY(clk.end_stage());
    if (p->exch) DFFT_TRY(comm_exchange(p->comm, p->xd, p->stream));  // buf2 -> peers' buf1 = [x][ys][N2]
    DFFT_TRY(clk.end_stage());
    DFFT_TRY(launch_x(p, p->buf1, p->buf2, true));                      // [x][ys][N2] -> [kx][ys][N2]
    if (p->exch) {
        DFFT_TRY(comm_exchange(p->comm, p->xd2, p->stream));            // buf2 -> peers' rbuf = [src][xs][yl_src][N2]
        hipError_t e = launch_pack(p->dtype, -1, p->rbuf, p->buf2, (int)p->xs, (int)n1, (int)n2, (int)p->sy.blk,
                                   (int)p->sy.size(p->P - 1), p->P, p->stream);
        if (e != hipSuccess) return fail(DFFT_EHIP, std::string("unpack: ") + hipGetErrorString(e));
    }
    DFFT_TRY(clk.end_stage());
    return DFFT_OK;
}

static int execute_backward(dfft_plan_s* p, bool sync) {
    const bool      fused = !(p->flags & DFFT_PLAN_UNFUSED);
    const long long n1 = p->N[1], n2 = p->N[2], n0 = p->N[0];
    StageClock      clk{p, sync};
    DFFT_TRY(clk.begin());
    const void* src = (p->flags & DFFT_PLAN_INPUT_FROM_IN) ? p->in : p->buf1;
    // where the inverse Y pass leaves its columns for the inverse Z pass: the padded work buffer when the plan has one
    const SlabLayout nat{n2, n1 * n2};
    void*            ydst = (fused && p->wbuf) ? p->wbuf : p->buf2;
    const SlabLayout yl = (fused && p->wbuf) ? p->wl : nat;
    const SlabLayout *ly = (fused && p->wbuf) ? &yl : nullptr, *lnat = ly ? &nat : nullptr;
    if (fused && p->exch && (p->flags & DFFT_PLAN_OVERLAP) && p->part_planes > 0) {
        // ---- mirror image of the overlapped forward pipeline: the inverse X pass runs Y sub-block by sub-block into the
        // send buffer [k][x all][y in k][N2] and sub-block k is exchanged (stream2) while sub-block k+1 is transformed;
        // the last sub-block is exchanged X-plane part by part, and the Y+Z passes of part i start when part i has landed.
        const bool      rccl = comm_is_async(p->comm);
        const int       I = (int)((p->sx.blk + p->part_planes - 1) / p->part_planes);
        const int       YK = p->ycuts;
        const long long ysub = p->ys / YK;
        const size_t    sub = (size_t)n0 * ysub * n2 * elem_bytes(p->dtype);
        hipStream_t     xs_ = rccl ? p->stream2 : p->stream;  // LOCAL: host-synchronising, same call sequence
        for (int y = 0; y < YK; ++y) {
            if (YK == 1) DFFT_TRY(launch_x(p, src, p->rbuf));
            else DFFT_TRY(launch_x(p, (const char*)src + y * sub, (char*)p->rbuf + y * sub, false, ysub));
            if (rccl) {
                hipEvent_t done = YK == 1 ? p->join_ev : p->y_ev[y];
                DFFT_HIP_TRY(hipEventRecord(done, p->stream));
                DFFT_HIP_TRY(hipStreamWaitEvent(p->stream2, done, 0));
            }
            if (y + 1 < YK) {
                DFFT_TRY(comm_exchange_part(p->comm, p->xd, 0, p->sx.blk, xs_, y));  // all X planes of sub-block y
            } else {
                for (int i = 0; i < I; ++i) {
                    DFFT_TRY(comm_exchange_part(p->comm, p->xd, i, p->part_planes, xs_, YK == 1 ? -1 : y));
                    if (rccl) DFFT_HIP_TRY(hipEventRecord(p->part_ev[i], p->stream2));
                }
            }
        }
        DFFT_TRY(clk.end_stage());  // inverse X passes (the exchange of the earlier sub-blocks runs underneath)
        for (int i = 0; i < I; ++i) {
            if (rccl) DFFT_HIP_TRY(hipStreamWaitEvent(p->stream, p->part_ev[i], 0));
            if (i == 0) {
                DFFT_TRY(clk.end_stage());  // exposed part of the exchange
                DFFT_TRY(clk.end_stage());  // unpack folded into the Y pass
            }
            long long x0, nx;
            part_range(p->xs, p->part_planes, i, &x0, &nx);
            if (nx > 0 && p->zy_on) {  // unpacking Y columns + Z rows of the part in one launch
                DFFT_TRY(launch_zy_stage(p, nullptr, ydst, yl.plane, p->buf2, p->buf1, true, x0, nx));
            } else if (nx > 0) {
                DFFT_TRY(launch_y(p, p->buf1, ydst, false, true, x0, nx, FFT_HINT_STREAM_IN, nullptr, &yl));
                DFFT_TRY(fft_rows(ydst, p->buf2, (int)n2, nx * n1, p->dtype, p->direction, p->stream, x0 * n1, 0, 1.0, ly, lnat, ly ? n1 : 0));
            }
        }
        DFFT_TRY(clk.end_stage());
        return DFFT_OK;
    }
    // ---- inverse X FFT: [ys][N2][kx] -> [x][ys][N2] ----
    // (single GPU: straight into the padded work buffer -- the plane-strided 128-byte stores are the scattered side here)
    const bool xw = fused && !p->exch && p->wbuf;
    if (p->conv_half) {
        // (spectral-filter plans: the X stage has left its result where the inverse X pass would have -- the hand-over buffer, the result
        // buffer, or the send buffer of the exchange, which conv plans point at the forward half's receive buffer)
    } else if (fused) {
        DFFT_TRY(launch_x(p, src, xw ? p->wbuf : p->buf2, false, 0, xw ? &yl : nullptr));
    } else {
        DFFT_TRY(fft_rows(src, p->buf1, (int)n0, p->ys * n2, p->dtype, p->direction, p->stream, 0, 0, p->scale));
        hipError_t e = launch_transpose(p->dtype, p->buf1, p->buf2, p->ys * n2, n0, p->stream);
        if (e != hipSuccess) return fail(DFFT_EHIP, std::string("transpose: ") + hipGetErrorString(e));
    }
    DFFT_TRY(clk.end_stage());
    // ---- exchange back ----
    void* ybuf = p->buf2;  // where the Y/Z passes run
    if (p->exch) {
        DFFT_TRY(comm_exchange(p->comm, p->xd, p->stream));  // buf2 -> peers' buf1 (packed [d][xs][yl_d][N2])
    } else if (!fused) {
        DFFT_HIP_TRY(hipMemcpyAsync(p->buf1, p->buf2, (size_t)p->xs * n1 * n2 * elem_bytes(p->dtype),
                                    hipMemcpyDeviceToDevice, p->stream));
    }
    DFFT_TRY(clk.end_stage());
    // ---- unpack + inverse Y, inverse Z ----
    if (fused) {
        DFFT_TRY(clk.end_stage());  // unpack folded into the Y pass
    } else {
        hipError_t e = launch_pack(p->dtype, -1, p->buf1, p->buf2, (int)p->xs, (int)n1, (int)n2, (int)p->sy.blk,
                                   (int)p->sy.size(p->P - 1), p->P, p->stream);
        if (e != hipSuccess) return fail(DFFT_EHIP, std::string("unpack: ") + hipGetErrorString(e));
        DFFT_TRY(clk.end_stage());
    }
    const bool      y_unpacks = fused && p->exch;
    const long long cp = p->chunk_planes > 0 ? p->chunk_planes : p->xs;
    // streaming hints whenever the stage works on cache-sized pieces of a slab too big to be cache-resident as a whole
    const bool      chunked = cp < p->xs || p->xs * n1 * n2 * (long long)elem_bytes(p->dtype) >= (64ll << 20);
    const bool one_launch = p->zy_on && fused;
    // Y columns (in place on the intermediate, or unpacking the receive buffer into it), then Z rows into the result: one launch
    // single-GPU plans with a hand-over buffer: rows first (dfft_zy.hip, SIGN) -- Z rows hand-over buffer -> result buffer, Y columns in place
    // on the result buffer; the transform is the same, its strided side moves from HBM reads to the cache-resident chunk
    // (the kernel's row-producing source path reads rows n2 apart: a hand-over buffer with padded ROWS keeps columns first)
    if (one_launch && p->zy_inv_rows_first && xw && p->zy_lazy && p->wl.pitch == n2) DFFT_TRY(launch_zy_stage(p, p->wbuf, ybuf, n1 * n2, nullptr, nullptr, false, 0, p->xs, +1));
    else if (one_launch) DFFT_TRY(launch_zy_stage(p, nullptr, fused ? ydst : ybuf, yl.plane, ybuf, y_unpacks ? p->buf1 : nullptr, y_unpacks, 0, p->xs));
    for (long long x0 = 0; !one_launch && x0 < p->xs; x0 += cp) {  // Y then Z per cache-sized chunk of planes (see execute_forward)
        const long long nx = std::min(cp, p->xs - x0);
        // single-GPU plans with a hand-over buffer, slab cut into cache chunks: Z rows first, like the one-launch stage above (round 6, last
        // session) -- rows hand-over buffer (HBM, contiguous) -> result buffer (natural layout, left in the Infinity Cache), then Y columns in
        // place on the result buffer: the strided side moves from HBM reads to the cache-resident chunk.  Inverse YZ stage 1024^3 fp32
        // 7.10 -> 5.93 ms, 2048 x 1024 x 512 fp64 13.08 -> 11.16, 512^3 fp32 0.89 -> 0.71; whole backward transform -7 ... -14 %
        // (profiles/r06/experiments/lib_ab_inverse_rows_first_chunks.log).  Same switches as the one-launch stage: DFFT_ZY_INV_ROWS_FIRST=0
        // or DFFT_ZY_LAZY=0 (the forms the bit-identity tests compare with each other) keep columns first.
        if (xw && cp < p->xs && p->zy_inv_rows_first && p->zy_lazy) {
            DFFT_TRY(fft_rows(p->wbuf, ybuf, (int)n2, nx * n1, p->dtype, p->direction, p->stream, x0 * n1, FFT_HINT_STREAM_IN, 1.0, ly, lnat, n1));
            DFFT_TRY(launch_y(p, ybuf, ybuf, false, false, x0, nx));
            continue;
        }
        if (y_unpacks) DFFT_TRY(launch_y(p, p->buf1, fused ? ydst : ybuf, false, true, x0, nx, chunked ? FFT_HINT_STREAM_IN : 0, nullptr, &yl));
        else if (xw) DFFT_TRY(launch_y(p, p->wbuf, p->wbuf, false, false, x0, nx, 0, &yl, &yl));
        else DFFT_TRY(launch_y(p, p->buf2, ybuf, false, false, x0, nx));
        if (!sync && p->timed && cp >= p->xs) DFFT_HIP_TRY(hipEventRecord(p->ev[5], p->stream));
        if (fused && p->wbuf) DFFT_TRY(fft_rows(ydst, ybuf, (int)n2, nx * n1, p->dtype, p->direction, p->stream, x0 * n1, 0, 1.0, ly, lnat, n1));
        else DFFT_TRY(fft_rows(ybuf, ybuf, (int)n2, nx * n1, p->dtype, p->direction, p->stream, x0 * n1));
    }
    DFFT_TRY(clk.end_stage());
    return DFFT_OK;
}

// ---- plan creation: what the four kinds of plan share -------------------------------------------------------------------------
int check_plan_args(const std::string& fn, const void* plan, const void* in, const void* out, long long n0, long long n1, long long n2, int dtype,
                    dfft_comm_t comm, int global_idx, int total_devices, unsigned flags, const PlanArgRules& rules) {
    if (!plan || !in) return fail(DFFT_EINVAL, fn + ": null plan/in");
    if (n0 < 1 || n1 < 1 || n2 < 1) return fail(DFFT_EINVAL, fn + ": sizes must be positive");
    if (!valid_dtype(dtype)) return fail(DFFT_EINVAL, fn + ": dtype");
    if (rules.direction && !valid_direction(*rules.direction)) return fail(DFFT_EINVAL, fn + ": direction");
    if (total_devices < 1 || global_idx < 0 || global_idx >= total_devices) return fail(DFFT_EINVAL, fn + ": device index");
    if (total_devices > 1 && !comm) return fail(DFFT_EINVAL, fn + ": a communicator is required for P > 1");
    if (comm && comm_size(comm) != total_devices) return fail(DFFT_EINVAL, fn + ": communicator size != P");
    if (rules.out_of_place && (out == nullptr || out == in)) return fail(DFFT_EINVAL, fn + ": " + rules.out_of_place);
    if (flags & ~rules.flags_allowed) return fail(DFFT_EUNSUPPORTED, fn + ": " + rules.flags_text);
    return DFFT_OK;
}

// experiment knobs: DFFT_Z_GRID / DFFT_Y_GRID / DFFT_X_GRID cap the persistent grid of the respective pass -- a tuning knob and the
// tests' way to give a workgroup many tiles.  Read ONCE per plan (plan_new), never on the launch path: getenv is not safe
// against a concurrent setenv of another device thread.
static int env_grid(const char* name) {
    const char* e = getenv(name);
    return e ? atoi(e) : 0;
}

dfft_plan_s* plan_new(const long long shape[3], int dtype, int direction, int P, int me, dfft_comm_t comm, unsigned flags) {
    dfft_plan_s* p = new dfft_plan_s;
    for (int a = 0; a < 3; ++a) p->N[a] = shape[a];
    p->dtype = dtype;
    p->direction = direction;
    p->P = P;
    p->me = me;
    p->flags = flags;
    p->is_last = me == P - 1;
    p->sx = make_slab(shape[0], P);
    p->sy = make_slab(shape[1], P);
    p->xs = p->sx.size(me);
    p->ys = p->sy.size(me);
    p->comm = comm;
    p->grid_x = env_grid("DFFT_X_GRID");
    p->grid_y = env_grid("DFFT_Y_GRID");
    p->grid_z = env_grid("DFFT_Z_GRID");
    return p;
}

// (dfft_plan_destroy reports a one-launch YZ stage that gave up, and a communicator may report while it unregisters: neither may
// replace the message of the failure that ended the create function)
void PlanDeleter::operator()(dfft_plan_s* p) const {
    const std::string msg = last_error();
    (void)dfft_plan_destroy(p);
    set_error(msg);
}

void enable_peer_access(int device) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess) return;
    for (int d = 0; d < ndev; ++d) {
        int can = 0;
        if (d == device || hipDeviceCanAccessPeer(&can, device, d) != hipSuccess || !can) continue;
        if (hipDeviceEnablePeerAccess(d, 0) != hipSuccess) (void)hipGetLastError();  // already enabled / not supported: copies still work
    }
}

long long cache_chunk_planes(long long planes, long long plane_bytes, long long default_mb, long long rule_planes) {
    const char*     ce = getenv("DFFT_CHUNK_MB");
    const long long mb = ce ? atoll(ce) : default_mb;
    long long       cp = rule_planes > 0 ? rule_planes : (mb > 0 ? evened_chunk_planes(planes, plane_bytes, mb) : 0);
    const char*     cpe = getenv("DFFT_CHUNK_PLANES");
    if (cpe && atoll(cpe) > 0) cp = atoll(cpe);
    return cp >= planes ? 0 : cp;
}

int plan_create_impl(dfft_plan_t* plan, long long n0, long long n1, long long n2, int dtype, int direction, void* in, void* out, dfft_comm_t comm,
                     int global_idx, int total_devices, unsigned flags, int conv_half) {
    PlanArgRules rules;
    rules.direction = &direction;
    DFFT_TRY(check_plan_args("dfft_plan_create", plan, in, out, n0, n1, n2, dtype, comm, global_idx, total_devices, flags, rules));
    if (dfft_device_count() < 1) return fail(DFFT_ENOGPU, "dfft_plan_create: no HIP device visible (no CPU fallback)");
    bool bluestein_axis = false;
    for (long long n : {n0, n1, n2}) {
        if ((flags & DFFT_PLAN_ANY_LENGTH) && length_kind(n) == 3) {
            bluestein_axis = true;
            continue;
        }
        if (!dfft_length_supported(n))
            return fail(DFFT_EUNSUPPORTED, "dfft_plan_create: FFT length " + std::to_string(n) + " has no gfx950 plan" +
                                               ((flags & DFFT_PLAN_ANY_LENGTH) ? "" : " (DFFT_PLAN_ANY_LENGTH accepts any length up to 2^23)"));
    }

    const bool long_axis = (n0 > 4096 && length_kind(n0) == 2) || (n1 > 4096 && length_kind(n1) == 2) || (n2 > 4096 && length_kind(n2) == 2);
    if (long_axis && (flags & DFFT_PLAN_NATURAL))
        return fail(DFFT_EUNSUPPORTED, "dfft_plan_create: natural-order plans need single-pass axis lengths (<= 4096)");
    if (bluestein_axis && (flags & DFFT_PLAN_NATURAL))
        return fail(DFFT_EUNSUPPORTED, "dfft_plan_create: natural-order plans need 7-smooth axis lengths (no Bluestein axis)");
    // the four-step and Bluestein axes run in the reference's stage structure
    if (long_axis || bluestein_axis) flags = (flags | DFFT_PLAN_UNFUSED) & ~DFFT_PLAN_OVERLAP;
    trace("dfft_plan_create", n0 * 1000000 + n1 * 1000 + n2 % 1000, (long long)flags * 100 + total_devices);
    // (refused while the plan owns nothing: from here on a failure destroys what has been built)
    const Slab sx = make_slab(n0, total_devices), sy = make_slab(n1, total_devices);
    if (sx.size(total_devices - 1) < 1 || sy.size(total_devices - 1) < 1)
        return fail(DFFT_EINVAL, "dfft_plan_create: slab decomposition leaves the last device empty");
    const long long max_count = dfft_max_count(n0, n1, n2, total_devices, global_idx == total_devices - 1);
    if (max_count >= (1ll << 31)) return fail(DFFT_EUNSUPPORTED, "dfft_plan_create: more than 2^31 elements per device");
    const bool inplace = (out == nullptr || out == in);  // fft_mpi_3d_api.cpp:68-75
    if (inplace && (flags & DFFT_PLAN_INPUT_FROM_IN) && !conv_half)  // (a forward half plan never writes its result buffer)
        return fail(DFFT_EINVAL, "dfft_plan_create: DFFT_PLAN_INPUT_FROM_IN needs an out-of-place plan");
    if ((flags & DFFT_PLAN_NATURAL) && (flags & DFFT_PLAN_UNFUSED))
        return fail(DFFT_EINVAL, "dfft_plan_create: DFFT_PLAN_NATURAL is a fused-pipeline option");
    const long long shape[3] = {n0, n1, n2};
    PlanOwner       owner(plan_new(shape, dtype, direction, total_devices, global_idx, comm, flags));
    dfft_plan_s*    p = owner.get();
    p->long_axis = long_axis;
    p->conv_half = conv_half != 0;
    p->conv_no_rot = conv_half == 2;
    {
        const char* fe = getenv("DFFT_FORCE_EXCHANGE");
        p->exch = total_devices > 1 || (comm && comm_kind(comm) == 1 && fe && *fe && *fe != '0');
    }
    p->max_count = max_count;
    p->in = in;
    p->out = out;
    p->inplace = inplace;
    p->buf2 = inplace ? in : out;
    const size_t bytes = (size_t)p->max_count * elem_bytes(dtype);
    hipError_t   e = hipGetDevice(&p->device);
    if (e == hipSuccess && comm && comm_kind(comm) == 0 && total_devices > 1) enable_peer_access(p->device);
    // buffers that are (or may be) registered as receive buffers come from the communicator (pooled per key by IPC communicators)
    const std::string rkey = std::to_string(n0) + "x" + std::to_string(n1) + "x" + std::to_string(n2) + ":" + std::to_string(dtype) + ":" +
                             std::to_string(total_devices);
    const size_t rbytes = recv_buffer_bytes(p);  // rank-symmetric (>= bytes)
    if (e == hipSuccess && comm_recv_alloc(comm, rkey + ":b1", rbytes, &p->buf1) != DFFT_OK) e = hipErrorOutOfMemory;
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&p->stream, hipStreamNonBlocking);
    // :77 input captured at plan time.  A device-to-device hipMemcpy on the null stream may return before the copy has run and is not
    // ordered with this plan's (non-blocking) stream -- and bufferDev1 is the RECEIVE buffer of the exchange: a copy that ran late
    // would overwrite data a peer had pushed already (round 5, tools/stall_hunt.py: the overlapped backward plan's first batch
    // differed from the serial result in 2 of 20 four-process runs).  So: everything the caller queued (whatever stream produced
    // `in`) is waited for, the copy runs on the plan's own stream, and plan creation returns when it has landed.
    if (e == hipSuccess) e = hipDeviceSynchronize();
    // (half plans of a spectral-filter plan capture nothing: their `in` holds dfft_local_count elements, not dfft_max_count)
    if (e == hipSuccess && !conv_half) e = hipMemcpyAsync(p->buf1, in, bytes, hipMemcpyDeviceToDevice, p->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(p->stream);
    for (auto& ev : p->ev)
        if (e == hipSuccess) e = hipEventCreate(&ev);
    // forward: always; backward: out-of-place plans that read the caller's `in` (the inverse X pass of sub-block k+1 must
    // not read a buffer the exchange of sub-block k is receiving into)
    if ((flags & DFFT_PLAN_OVERLAP) && p->exch && !(flags & (DFFT_PLAN_UNFUSED | DFFT_PLAN_NATURAL)) &&
        (direction == DFFT_FORWARD || (flags & DFFT_PLAN_INPUT_FROM_IN))) {
        // parts: DFFT_OVERLAP_PARTS (default 4) per slab, never larger than one Infinity-Cache chunk; derived from the
        // global block size ceil(N0/P) so that every rank cuts identically
        // How many: every part is a launch of its own (the one-launch YZ stage or a Z + Y pair) plus an exchange round, and short
        // launches pay their ramps -- four parts at every P taxed the local work of 512^3 fp64 by 30-40 % at P = 8, where a part was
        // 16 planes = 64 MiB = 40 us of work (t0 0.156 -> 0.207 ms per rank, profiles/r04/local_by_P.log), a third of what the overlap
        // can hide there.  So parts are sized, not counted: at least 128 MiB of slab each, between 2 and 4 of them (P = 8: 2 parts of
        // 128 MiB, P = 4 and below: 4), then capped by the cache chunk as before.  DFFT_OVERLAP_PARTS=n overrides.
        const long long plane_bytes = n1 * n2 * (long long)elem_bytes(dtype);
        long long       parts = std::min(4ll, std::max(2ll, (p->sx.blk * plane_bytes + (128ll << 20) - 1) / (128ll << 20)));
        const char*     pe = getenv("DFFT_OVERLAP_PARTS");
        if (pe && atoll(pe) > 0) parts = atoll(pe);
        long long pp = (p->sx.blk + parts - 1) / parts;
        const long long cache_planes = std::max(1ll, (256ll << 20) / plane_bytes);
        if (pp > cache_planes) pp = cache_planes;
        if (pp < 1) pp = 1;
        p->part_planes = pp;
        const int K = (int)((p->sx.blk + pp - 1) / pp);
        p->part_ev.assign(K, nullptr);
        if (e == hipSuccess) e = hipStreamCreateWithFlags(&p->stream2, hipStreamNonBlocking);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&p->join_ev, hipEventDisableTiming);
        for (auto& ev : p->part_ev)
            if (e == hipSuccess) e = hipEventCreateWithFlags(&ev, hipEventDisableTiming);
        // Y sub-blocks for the t2/t3 overlap (DFFT_OVERLAP_YPARTS, default 2; 1 = off): even Y split only
        long long   yk = 2;
        const char* ye = getenv("DFFT_OVERLAP_YPARTS");
        if (ye && atoll(ye) > 0) yk = atoll(ye);
        if (yk > 1 && n1 % total_devices == 0 && (n1 / total_devices) % yk == 0 && n0 % total_devices == 0) {
            p->ycuts = (int)yk;
            p->y_ev.assign(yk, nullptr);
            for (auto& ev : p->y_ev)
                if (e == hipSuccess) e = hipEventCreateWithFlags(&ev, hipEventDisableTiming);
        }
    }
    if (e != hipSuccess) return fail(DFFT_EHIP, std::string("dfft_plan_create: ") + hipGetErrorString(e));
    const bool natural = (flags & DFFT_PLAN_NATURAL) != 0;
    fill_exchange(p, p->xd, natural ? DFFT_FORWARD : direction);
    p->xd.sendbuf = p->buf2;
    p->xd.recvbuf = p->buf1;
    if (natural && p->exch) {
        // natural-order plans re-slab twice (X->Y for the X pass, Y->X to return to the caller's layout); the second
        // exchange receives the packed [src][xs][yl_src][N2] blocks into a buffer of its own and uses the other slot
        if (comm_recv_alloc(comm, rkey + ":nat", rbytes, &p->rbuf) != DFFT_OK)
            return fail(DFFT_EHIP, "dfft_plan_create: no memory for the second receive buffer");
        fill_exchange(p, p->xd2, DFFT_BACKWARD);
        p->xd2.sendbuf = p->buf2;
        p->xd2.recvbuf = p->rbuf;
        DFFT_TRY(comm_register(comm, global_idx, p->rbuf, p->device, &p->xd2.slot));
    }
    if (p->part_planes > 0) {
        // overlap mode: parts arrive while later planes are still being transformed in bufferDev1, so the exchange
        // needs a receive buffer of its own (one more slab in HBM; 288 GB makes that a non-issue)
        if (comm_recv_alloc(comm, rkey + ":rb", rbytes, &p->rbuf) != DFFT_OK)
            return fail(DFFT_EHIP, "dfft_plan_create: no memory for the receive buffer of the overlapped exchange");
        if (direction == DFFT_FORWARD) p->xd.recvbuf = p->rbuf;  // Y pass -> out (send) -> rbuf (receive) -> X pass -> out
        else p->xd.sendbuf = p->rbuf;                            // in -> X pass -> rbuf (send) -> bufferDev1 -> Y,Z -> out
        p->xd.ycuts = p->ycuts;
    }
    // (the receive buffer is registered with the communicator further down, once its placement has been decided)
    // padded work buffer (dfft_plan_s::wbuf): fused, non-natural pipelines whose rows are whole cache lines and whose three
    // lengths run on the tuned kernels (the run-time-scheduled kernel keeps plain rows).  DFFT_PAD=0 switches it off.
    {
        const char* pe = getenv("DFFT_PAD");
        const long long line = 128 / (long long)elem_bytes(dtype);
        // Only where it pays (profiles/r02/experiments/padding_sweep.log): planes a multiple of 1 MiB apart -- other strides
        // spread over the channels by themselves (384^3: no gain) -- and slabs larger than the 256 MiB Infinity Cache
        // (cache-resident problems do not reach HBM's channels: 256^3 is 6 % slower with the extra buffer).
        const long long plane_b = n1 * n2 * (long long)elem_bytes(dtype);
        const bool      pays = (pe && *pe == '1') || (plane_b % (1ll << 20) == 0 && p->xs * plane_b > (256ll << 20));
        // (single GPU only: with an exchange the X pass reads the receive buffer, whose layout is the wire format)
        if (!(pe && *pe == '0') && pays && !p->exch && !(flags & (DFFT_PLAN_UNFUSED | DFFT_PLAN_NATURAL)) && (n2 % line) == 0 &&
            fft_length_tuned((int)n0) && fft_length_tuned((int)n1) && fft_length_tuned((int)n2)) {
            // lines of padding per row / per plane (tuning knobs DFFT_PAD_ROW, DFFT_PAD_PLANE; measured: profiles/r02)
            const char* pr = getenv("DFFT_PAD_ROW");
            const char* pp = getenv("DFFT_PAD_PLANE");
            const long long row_lines = pr ? atoll(pr) : 0, plane_lines = pp ? atoll(pp) : 3;
            p->wl.pitch = n2 + row_lines * line;
            p->wl.plane = n1 * p->wl.pitch + plane_lines * line;
            if (p->xs * p->wl.plane < (1ll << 31)) {
                e = slab_alloc(&p->wbuf, (size_t)p->xs * p->wl.plane * elem_bytes(dtype));
                if (e != hipSuccess) {  // an optimisation, not a requirement: run the natural layout in bufferDev1 instead
                    (void)hipGetLastError();
                    p->wbuf = nullptr;
                    if (getenv("DFFT_DEBUG")) fprintf(stderr, "[dfft] no memory for the padded hand-over buffer (%s): natural layout\n", hipGetErrorString(e));
                    e = hipSuccess;
                }
                if (getenv("DFFT_DEBUG")) fprintf(stderr, "[dfft] plan buffers: in %p out %p bufferDev1 %p work %p\n", in, out, p->buf1, p->wbuf);
            }
        }
    }
    {
        // Rotated rows in the exchange buffers (dfft_plan_s::rot_elems): the same remedy for the P > 1 pipeline that the padded
        // hand-over buffer is for the single-GPU one.  Every rank derives it from (N, P, precision, flags) alone -- both ends of
        // every message must agree.  Where: fused, even splits, tuned kernels on all three axes, rows of whole lines and a
        // power-of-two length, received planes a multiple of 128 KiB apart (other strides spread over the channels by
        // themselves).  DFFT_ROT=0 / 1 forces it off / on (wherever it is possible).
        const char*     re = getenv("DFFT_ROT");
        const long long S = (long long)elem_bytes(dtype);
        const bool      possible = p->exch && !p->conv_no_rot && !(flags & (DFFT_PLAN_UNFUSED | DFFT_PLAN_NATURAL)) && !p->long_axis && n0 % total_devices == 0 &&
                              n1 % total_devices == 0 && (n2 & (n2 - 1)) == 0 && (n2 * S) % 128 == 0 && n2 * S >= 256 && n2 < (1ll << 30) &&
                              fft_length_tuned((int)n0) && fft_length_tuned((int)n1) && fft_length_tuned((int)n2);
        const long long ysub = p->ys / std::max(1, p->ycuts);
        // (round 6: 128 KiB, not 256 -- with received planes an odd multiple of 128 KiB apart the rotation is worth 7-10 % of the X pass in
        // five shapes of seven, nothing in one, -4 % in one: config 4's overlapped rank at P = 8, 384 KiB, 0.326 -> 0.299 ms;
        // profiles/r06/experiments/rot_pays_128k.log)
        const bool      pays = (ysub * n2 * S) % (128ll << 10) == 0;
        // How far: 3 cache lines per X plane (the pad of the single-GPU hand-over buffer, round 2) -- but 2 lines where the X axis is long
        // and the received planes lie at least 1 MiB apart.  Round 6 (profiles/r06/experiments/rot_lines_*.log, DFFT_ROT_LINES swept, four
        // plans per point): a tile of the X pass walks N0 segments (plane stride + rotation) apart; with 2048 planes 2 MiB apart (config 5's
        // rank at P = 8) 1 line 1.85 ms, 2 lines 1.67, 3 lines 1.89, 4 lines 1.98, 6 lines 1.67 -- odd multiples of 256 bytes spread the
        // walk over all channels, 384 bytes over two thirds of them, 512 over half.  2 against 3 lines: 1024^3 fp64 at P = 8 0.842 -> 0.737 ms,
        // 1024^3 fp32 at P = 4 0.801 -> 0.750, config 4 at P = 4 0.593 -> 0.569; no difference with 512 planes, and with planes
        // 512-768 KiB apart (512^3 overlapped at P = 4 / 8, config 4 at P = 8) 3 lines stay 2-10 % ahead.  DFFT_ROT_LINES=n overrides.
        if (possible && !(re && *re == '0') && (pays || (re && *re == '1'))) {
            int         lines = (n0 >= 1024 && ysub * n2 * S >= (1ll << 20)) ? 2 : 3;
            const char* rl = getenv("DFFT_ROT_LINES");
            if (rl && atoi(rl) > 0) lines = atoi(rl);
            p->rot_elems = (int)(lines * 128 / S);
        }
    }
    {
        // kernel-variant switches (A/B measurements; results are bit-identical either way), read when the plan is created:
        //   DFFT_X_VARIANT=half|full|fullearly  1024-point forward X pass: half-tile prefetch / whole-tile prefetch (default) / + early wait
        //   DFFT_X_VARIANT=early                512-point forward X pass: early wait for the prefetched tile (the default in fp64)
        //   DFFT_X_VARIANT=static|late|static-late  512-point forward X pass in fp64, whose default draws its tiles by ticket and waits
        //                                       early: the static grid-stride loop / the late wait / both (the form up to round 6)
        //   DFFT_ZY_LAZY=0                      one-launch YZ stage (P = 1): the eager-publish kernel instead of the lazy one
        const char* xv = getenv("DFFT_X_VARIANT");
        if (xv && !strcmp(xv, "half")) p->x_hints = FFT_HINT_HALF_PREFETCH;
        else if (xv && (!strcmp(xv, "fullearly") || !strcmp(xv, "early"))) p->x_hints = FFT_HINT_EARLY_WAIT;
        else if (xv && !strcmp(xv, "static")) p->x_hints = FFT_HINT_STATIC_TILES;
        else if (xv && !strcmp(xv, "late")) p->x_hints = FFT_HINT_LATE_WAIT;
        else if (xv && !strcmp(xv, "static-late")) p->x_hints = FFT_HINT_STATIC_TILES | FFT_HINT_LATE_WAIT;
        // the ticket counter of the X pass (dfft_plan_impl.h): single-GPU forward plans whose X pass is the 512-point fp64 staged store;
        // zeroed on the plan's stream and waited for, like the YZ stage's control block below
        if (dtype == F64 && n0 == 512 && direction == DFFT_FORWARD && n2 % 8 == 0 && !p->exch && !(flags & DFFT_PLAN_NATURAL) && !p->long_axis) {
            if (hipMalloc((void**)&p->x_ticket_ctr, sizeof(unsigned)) != hipSuccess || hipMemsetAsync(p->x_ticket_ctr, 0, sizeof(unsigned), p->stream) != hipSuccess ||
                hipStreamSynchronize(p->stream) != hipSuccess)
                return fail(DFFT_EHIP, "dfft_plan_create: no ticket counter for the X pass");
            // what the X pass will run on, until a launch has said so itself (dfft_plan_describe)
            p->x_form = X_FORM_512_F64 | ((p->x_hints & FFT_HINT_LATE_WAIT) ? 0 : X_FORM_EARLY) | ((p->x_hints & FFT_HINT_STATIC_TILES) ? 0 : X_FORM_TICKET);
        }
        const char* zl = getenv("DFFT_ZY_LAZY");
        p->zy_lazy = !(zl && *zl == '0');  // default on: t0 of 512^3 fp64 1.278 -> 1.163 ms (profiles/r03/experiments/variant_ab.log)
        const char* rf = getenv("DFFT_ZY_INV_ROWS_FIRST");
        p->zy_inv_rows_first = !(rf && *rf == '0');
    }
    if (comm) {
        // placement of the receive buffer (P > 1 twin of dfft_plan_tune), then its registration: after that the peers know the pointer
        DFFT_TRY(place_recv_buffer(p));
        DFFT_TRY(comm_register(comm, global_idx, p->xd.recvbuf, p->device, &p->xd.slot));  // nodeDataDev[loc] = bufferDev1, :80
    }
    {
        // one-launch t0 (dfft_zy.hip): where the kernel exists and the plan has the unpadded-row hand-over buffer it works on
        const char* oe = getenv("DFFT_T0_ONE_LAUNCH");
        const long long ysub = p->sy.blk / std::max(1, p->ycuts);
        const bool      single_ok = !p->exch && (!p->wbuf || p->wl.pitch == n2);
        const bool      multi_ok = p->exch && n0 % total_devices == 0 && n1 % total_devices == 0 && n1 >= 8 && ysub % zy_col_threads((int)n1, p->zy_lazy ? 1 : 0) == 0;  // even splits; a
                                   // destination block is a whole number of the column unit's strides (the threads of one column FFT)
        // Where the stage is used by itself (DFFT_T0_ONE_LAUNCH=0: never; =1: wherever the kernel exists on single-GPU plans; =all:
        // P > 1 plans too).  Round 3 used it for 512 x 512-point planes on a single GPU only; since round 4
        //  * un-packed launches with a 256-point Y axis take column tiles of two cache lines (ZyTile, dfft_zy.hip: 512-thread
        //    workgroups and 64 KiB units again), and the stage wins on every plane shape it is built for -- t0 / back-to-back ms per
        //    transform, two launches per chunk -> one launch: 256^3 (BASELINE config 2) 0.169 / 0.2445 -> 0.154 / 0.2350, 512 x 256 x 256
        //    0.357 / 0.510 -> 0.305 / 0.463, 256 x 256 x 512 0.349 / 0.509 -> 0.307 / 0.469, 256 x 512 x 256 0.355 / 0.528 -> 0.309 / 0.470
        //    (profiles/r04/experiments/variant_ab_256_wide_tiles.log; with one-line tiles it lost: 0.170 vs 0.216 at 256^3);
        //  * the packed launches of P > 1 plans run the lazy-publish form too (it measured equal to two launches while it published
        //    eagerly): per rank at 512^3 fp64, exchange switched off, t0 / back-to-back P = 2 0.690 / 1.052 -> 0.630 / 0.94, P = 4
        //    0.343 / 0.512 -> 0.32 / 0.492, P = 8 0.174 / 0.255 -> 0.157 / 0.248 (experiments/lib_ab_lazy_packed.log) -- used by itself
        //    for 512 x 512-point planes (packed tiles stay one line wide, so planes with a 256-point axis keep two launches).
        //  * round 5: planes with a 768-point Y axis (BASELINE config 4's 768 x 512 planes; 12 points x 64 threads, twiddle table of the Y
        //    axis in LDS like the two-launch kernel's).  t0 / back-to-back ms, two launches per chunk -> one launch, 1024 x 768 x 512 fp64:
        //    P = 1 4.49 / 7.23 -> 3.99 / 6.73, per rank at P = 4 (192-row destination blocks) 1.12 / 1.84 -> 1.06 / 1.74 -- but at P = 8
        //    (96-row blocks, two offset tables per thread half) 0.57-0.60 / 0.91-0.93 -> 0.62 / 0.94 whatever the phase size
        //    (profiles/r05/experiments/variant_ab_768_final.log, c4_p8_one_launch_sweep.log): used by itself where a destination block is
        //    whole 64-row strides of the column unit, i.e. up to P = 4 for this axis.
        //  * round 6, overlapped forward plans: the ONE launch for all parts (zy_part_done below) also pays on 96-row destination blocks --
        //    config 4 per rank at P = 4 (two Y sub-blocks of 96 rows), overlapped t0 1.16 -> 1.05 ms against 1.03 for the serial plan
        //    (profiles/r06/experiments/c4_overlap_one_launch.log): what it replaces there is one launch pair PER PART, not per cache chunk.
        const bool      parts_fwd = p->part_planes > 0 && direction == DFFT_FORWARD && p->zy_lazy;
        const bool      multi_on = (n1 == 512 && n2 == 512) || (n1 == 768 && n2 == 512 && (ysub % 64 == 0 || parts_fwd)) || (oe && !strcmp(oe, "all"));
        if (!(oe && *oe == '0') && (single_ok || (multi_ok && multi_on)) && !(flags & (DFFT_PLAN_UNFUSED | DFFT_PLAN_NATURAL)) && !p->long_axis &&
            zy_supported(dtype, (int)n1, (int)n2) && p->xs <= ZY_MAX_PLANES) {
            p->zy_eligible = true;
            // zeroed ON THE PLAN'S STREAM and waited for: a memset on the null stream is asynchronous to the host and not ordered
            // with a non-blocking stream -- the first launch could start on uninitialised counters (seen once in the full test
            // suite, on recycled memory)
            if (hipMalloc((void**)&p->zy_ctl, sizeof(ZyCtl)) == hipSuccess && hipMemsetAsync(p->zy_ctl, 0, sizeof(ZyCtl), p->stream) == hipSuccess &&
                hipStreamSynchronize(p->stream) == hipSuccess && hipHostMalloc((void**)&p->zy_err, 128, hipHostMallocMapped) == hipSuccess) {
                *p->zy_err = 0u;
                p->zy_on = true;
                // a consumer's wait is bounded in polls (1-3 us each under load): seconds by default, so that time-slicing with
                // other processes, a profiler or a debugger cannot produce a spurious time-out, while a real dead-lock still ends
                const char* sp = getenv("DFFT_ZY_SPIN_POLLS");
                p->zy_spin_polls = sp && atoll(sp) > 0 ? (unsigned)std::min(atoll(sp), 0xffffffffll) : (4u << 20);
                const char* fe = getenv("DFFT_ZY_FAULT");
                p->zy_fault = fe ? atoi(fe) : 0;
                // overlapped forward plans: one launch for all parts (per-part counters of finished column units; the kernel addresses the
                // packed layout of a slab with 32-bit byte offsets there).  DFFT_ZY_PARTS_ONE_LAUNCH=0: one launch per part (round 5's form).
                const char* oa = getenv("DFFT_ZY_PARTS_ONE_LAUNCH");
                const int   K = p->part_planes > 0 ? (int)((p->sx.blk + p->part_planes - 1) / p->part_planes) : 0;
                if (p->exch && direction == DFFT_FORWARD && K > 0 && p->zy_lazy && !(oa && *oa == '0') && (size_t)p->max_count * elem_bytes(dtype) < ((size_t)1 << 32)) {
                    if (hipMalloc((void**)&p->zy_part_done, (size_t)K * sizeof(unsigned)) != hipSuccess ||
                        hipMemsetAsync(p->zy_part_done, 0, (size_t)K * sizeof(unsigned), p->stream) != hipSuccess || hipStreamSynchronize(p->stream) != hipSuccess) {
                        (void)hipGetLastError();
                        if (p->zy_part_done) (void)hipFree(p->zy_part_done);
                        p->zy_part_done = nullptr;
                    }
                }
            } else {
                (void)hipGetLastError();
            }
        }
    }
    {
        // Z+Y blocking for the 256 MiB Infinity Cache (MI355X_MICROARCH.md): the largest whole number of NATURAL planes that
        // fits, evened out over the chunks -- 8 x 64 planes at 512^3 fp64.  With the padded work buffer such a chunk is a few
        // KiB larger than the cache; measured (profiles/r02/experiments/chunk_planes_sweep.log, two boxes) that is still the
        // best size: t0 1.37-1.38 ms against 1.40-1.42 for 9 x 57 (sized on the padded planes), 60 or 63 planes, and the X pass
        // runs no slower behind it.  t0 follows the chunk count (~9 us per Z+Y launch pair) and is worst just above a
        // power-of-two size (40 planes: 1.63 ms); chunks of whole grid-stride rounds (56 / 60 planes) gain nothing.
        // Planes of 8 MiB and more (1024-point Y columns) keep one plane of head-room: 1024^3 15 instead of 16 planes t0 12.6 ->
        // 12.4 ms, 2048 x 1024 x 512 31 instead of 32 planes 12.5 -> 12.1 ms; smaller planes want the full count (512^3 fp64 64
        // planes, fp32 128 planes 0.80 -> 0.74 ms, 384^3 4 x 96; profiles/r02/experiments/chunk_shapes.log).
        // DFFT_CHUNK_MB=0 disables, =k overrides the capacity; DFFT_CHUNK_PLANES=n sets the chunk size directly (experiments).
        // The one-launch stage (dfft_zy.hip) has no launch boundaries to amortise and wants head-room instead: 9 phases of 57 planes
        // (228 MiB) run t0 of 512^3 fp64 in 1.213-1.216 ms, 8 x 64 (256 MiB + padding) in 1.297, 10 x 52 in 1.238, and any
        // count that leaves a short last phase loses (56 -> 9 x 56 + 8: 1.284; 62: 1.341; profiles/r03/experiments/
        // chunk_planes_one_launch.log) -- so: 230 MiB, evened out over the phases as before.
        const long long default_mb = p->zy_on ? 230 : 256;
        const char*     ce = getenv("DFFT_CHUNK_MB");
        const long long mb = ce ? atoll(ce) : default_mb;
        long long       streamed = 0;  // the chunk of the rule for Y passes that stream their results out, where it applies
        const char* re = getenv("DFFT_CHUNK_RULE");  // 0: the rule of rounds 2-3 for every plan (A/B switch)
        const bool  y_streams_out = p->exch && !(flags & (DFFT_PLAN_UNFUSED | DFFT_PLAN_NATURAL));
        if (mb > 0 && !p->zy_on && y_streams_out && !(re && *re == '0')) {
            // Fused P > 1 plans on two launches per chunk (round 4, profiles/r04/experiments/chunk_rule.log): the Y pass packs its
            // results straight into the send buffer with streaming stores, so the chunk is only READ from the cache and may fill it
            // (no head-room), and the largest chunk whose column tiles are a whole number of grid rounds (one tile per CU and round)
            // beats evened-out chunks, a short last chunk included -- a launch's ramp is amortised over more bytes.  Per rank, t0 /
            // back-to-back ms: config 4 at P = 8 (128 planes of 6 MiB) 4 x 32 -> 3 x 40 + 8 planes 0.613 / 0.953 -> 0.585 / 0.924, at
            // P = 4 1.190 / 1.890 -> 1.150 / 1.848; config 5 at P = 8 (16 MiB planes) 15 -> 16 planes 3.298 / 5.157 -> 3.207 / 5.060;
            // 1024^3 fp64 at P = 8 1.602 / 2.563 -> 1.544 / 2.486.  Single-GPU plans, whose Y pass works in place on the chunk, lose
            // with it (512^3 on two launches 8 x 64 -> 9 x 60 planes t0 1.380 -> 1.405 ms, 512 x 2048 x 512 6.21 -> 6.80) and keep the
            // rule below.
            const long long eb = (long long)elem_bytes(dtype);
            long long       fit = std::max(1ll, (mb << 20) / (n1 * n2 * eb));
            const long long line = 128 / eb, cus = std::max(1ll, zy_grid());  // (CUs of the current device)
            if (n2 % line == 0) {
                const long long tiles_per_plane = n2 / line;
                const long long q = cus / std::gcd(cus, tiles_per_plane);  // planes per whole number of grid rounds
                if (q > 1 && fit >= 2 * q) fit -= fit % q;
            }
            streamed = fit;
            // Overlapped plans on two launches per PART (no one-launch stage for the shape): a part is one Z + Y launch pair, so the same
            // rule sizes it -- when that does not change the number of parts (the overlap's granularity): config 4 per rank at P = 8,
            // 4 x 32 -> 3 x 40 + 8 planes (a 32-plane launch pair runs at the rate of a 32-plane chunk: serial t0 0.547 ms with 40-plane
            // chunks, 0.59 with 32, 0.616 for the four 32-plane parts; profiles/r06/experiments/c4_overlap_one_launch.log).  Decided from
            // rank-symmetric data only (the shape predicate zy_eligible, the global block size): every rank cuts the same parts.
            const long long blk = p->sx.blk, pp = p->part_planes;
            if (pp > 0 && !p->zy_eligible && !getenv("DFFT_OVERLAP_PARTS") && !ce && fit > pp && fit < blk && (blk + fit - 1) / fit == (blk + pp - 1) / pp)
                p->part_planes = fit;
        }
        p->chunk_planes = cache_chunk_planes(p->xs, n1 * n2 * (long long)elem_bytes(dtype), default_mb, streamed);  // (else: evened out)
    }
    if (p->long_axis) {
        p->chunk_planes = 0;  // the four-step passes work on the whole slab
        e = hipMalloc(&p->lbuf, (size_t)p->max_count * elem_bytes(dtype));
        if (e != hipSuccess) return fail(DFFT_EHIP, std::string("dfft_plan_create: ") + hipGetErrorString(e));
    }
    if (bluestein_axis) {
        // the tables of every Bluestein axis, and the scratch of the passes that use the multi-pass form: Z rows (xs * N1 of them), Y columns
        // (N2 wide, xs planes), X rows of the un-fused X pass (ys * N2)
        p->chunk_planes = 0;
        p->bs.fused = bluestein_fused_env();
        const size_t cap = chunk_cap_env();  // read here only: the passes of every execute fit their chunks to the bytes sized with it
        const long long passes[3][3] = {{n0, 1, p->ys * n2}, {n1, n2, p->xs}, {n2, 1, p->xs * n1}};  // (n, s, batch) per axis
        size_t          need = 0;
        for (const auto& ps : passes) {
            if (length_kind(ps[0]) != 3) continue;
            BluesteinTablesPtr t;
            DFFT_TRY(bluestein_tables(ps[0], dtype, direction, &t));
            p->bs.tables.push_back(t);
            need = std::max(need, bluestein_scratch_bytes(*t, ps[1], ps[2], p->bs.fused, cap));
        }
        if (need) {
            e = hipMalloc(&p->bs.scratch, need);
            if (e != hipSuccess) return fail(DFFT_EHIP, std::string("dfft_plan_create: Bluestein scratch: ") + hipGetErrorString(e));
            p->bs.bytes = need;
        }
    }
    // warm the twiddle caches so execute never allocates
    for (long long n : {n0, n1, n2}) {
        if (n > 4096 || length_kind(n) == 3) continue;  // long axes: their factors' tables are built on first use; Bluestein axes: above
        const void* tw;
        DFFT_TRY(get_twiddles((int)n, dtype, &tw));
    }
    *plan = owner.release();
    return DFFT_OK;
}

}  // namespace dfft

using namespace dfft;

extern "C" {

int dfft_plan_create(dfft_plan_t* plan, long long n0, long long n1, long long n2, int dtype, int direction, void* in,
                     void* out, dfft_comm_t comm, int global_idx, int total_devices, unsigned flags) {
    // in place (out == NULL or out == in) or out of place: `in` and `out` of dfft_max_count elements each must not overlap partly
    if (plan && in && out && n0 >= 1 && n1 >= 1 && n2 >= 1 && (dtype == DFFT_F64 || dtype == DFFT_F32) && total_devices >= 1 && global_idx >= 0 &&
        global_idx < total_devices &&
        partly_overlap(in, out, (uintptr_t)dfft_max_count(n0, n1, n2, total_devices, global_idx == total_devices - 1) * elem_bytes(dtype)))
        return fail(DFFT_EINVAL, "dfft_plan_create: in and out overlap partly (a plan runs out of place or exactly in place)");
    return plan_create_impl(plan, n0, n1, n2, dtype, direction, in, out, comm, global_idx, total_devices, flags, 0);
}

int dfft_plan_set_scale(dfft_plan_t plan, double s) {
    if (!plan || !(s == s) || s == 0.0) return fail(DFFT_EINVAL, "dfft_plan_set_scale: bad arguments");
    plan->scale = s;
    return DFFT_OK;
}

void* dfft_plan_buffer1(dfft_plan_t plan) { return plan ? plan->buf1 : nullptr; }
void* dfft_plan_result(dfft_plan_t plan) { return plan ? plan->buf2 : nullptr; }
void* dfft_plan_stream(dfft_plan_t plan) { return plan ? (void*)plan->stream : nullptr; }
void* dfft_plan_workbuf(dfft_plan_t plan, long long* bytes) {
    if (!plan || !plan->wbuf) return nullptr;
    if (bytes) *bytes = plan->xs * plan->wl.plane * (long long)elem_bytes(plan->dtype);
    return plan->wbuf;
}

int dfft_execute(dfft_plan_t plan, unsigned exec_flags) {
    if (!plan) return fail(DFFT_EINVAL, "dfft_execute: null plan");
    if (plan->conv) return conv_execute(plan, exec_flags);
    const bool sync = (exec_flags & DFFT_EXEC_SYNC_STAGES) != 0;
    plan->host_timed = sync;
    plan->timed = sync || !(exec_flags & DFFT_EXEC_NO_TIMING);
    if (!plan->timed && (exec_flags & DFFT_EXEC_PRINT)) return fail(DFFT_EINVAL, "dfft_execute: PRINT needs stage timing");
    // an earlier execute of the one-launch YZ stage that gave up and that nobody synchronised through the library (the pinned error
    // word is readable at any time): report it before anything else is queued; the stage is off from here on.  A plan with an
    // exchange queues this execute all the same (on the two-launch stage) and reports afterwards: returning early on ONE rank would
    // leave its peers waiting in the exchange for a partner that never comes.
    const int   zrc0 = zy_check(plan);
    std::string zmsg0 = zrc0 ? last_error() : std::string();
    if (zrc0 && !plan->exch) return zrc0;
    auto run = [&]() {
        const ExecutingPlan scope(plan);  // the passes run with this plan's scratch, grid cap and Bluestein tables
        return plan->r2c ? execute_r2c(plan, sync)
               : (plan->flags & DFFT_PLAN_NATURAL) ? execute_natural(plan, sync)
               : plan->direction == DFFT_FORWARD ? execute_forward(plan, sync)
                                                 : execute_backward(plan, sync);
    };
    const bool zy_used = plan->zy_on;
    if (plan->P > 1) trace("dfft_execute", plan->direction, exec_flags);
    int        rc = run();
    // host-synchronised executes have drained the stream (the reference-named wrapper always executes this way): a one-launch YZ
    // stage that gave up is seen here, before any timing is printed or any result used.  Where the pipeline has not written its own
    // input -- fused single-GPU plans that read `in` or bufferDev1 and work in the hand-over buffer -- the transform is simply run
    // again on two launches per chunk (zy_check has switched the stage off); otherwise the failure is the return code.
    // Who takes part in the agreement round is decided by rank-symmetric data only: the shape / flag predicate that selects
    // the stage (zy_eligible), not this device's allocation result or history -- and a device whose run() failed locally still enters
    // the round (contributing "failed"), so its peers are never left waiting in a collective one rank has skipped.
    const bool agree = sync && plan->exch && plan->zy_eligible && plan->direction == DFFT_FORWARD;
    if (rc && !agree) return rc;
    if (agree) {
        // (backward plans run the stage AFTER their exchange: a failure there spoils only the failing rank's own result, which that
        // rank reports itself below -- no collective needed, none paid)
        // P > 1: the failure is rank-local knowledge, but the exchange has already shipped this rank's invalid data to every peer.
        // Every device of the communicator learns of it here, returns an error and continues on the two-launch stage, so no rank
        // ever returns DFFT_OK for an execute that any rank knows to be invalid.
        const int   run_rc = rc;
        std::string run_msg = run_rc ? last_error() : std::string();
        int         mine = (zrc0 || run_rc) ? 1 : 0;
        if (!mine && zy_used) {
            mine = zy_check(plan) ? 1 : 0;
            if (mine) zmsg0 = last_error();
        }
        int any = 0;
        rc = comm_agree_max(plan->comm, plan->me, mine, plan->stream, &any);
        if (run_rc) return fail(run_rc, run_msg);  // this device's own failure is its return code, whatever the round said
        if (rc) return rc;
        if (any) {
            plan->zy_on = false;
            return mine ? fail(DFFT_EHIP, zmsg0)
                        : fail(DFFT_EHIP, "the one-launch YZ stage gave up (or the execute failed) on another device of this communicator: the results of this "
                                          "execute are invalid on every device; later executes use the two-launch stage");
        }
    } else if (sync && zy_used) {
        rc = zy_check(plan);
        if (rc) {
            const void* src = (plan->flags & DFFT_PLAN_INPUT_FROM_IN) ? plan->in : plan->buf1;
            // (a backward half plan of a spectral-filter plan has no inverse X pass that would rebuild the hand-over buffer)
            const bool  input_intact = !plan->exch && plan->wbuf && src != plan->buf2 && !(plan->flags & (DFFT_PLAN_UNFUSED | DFFT_PLAN_NATURAL)) &&
                                      !(plan->conv_half && plan->direction == DFFT_BACKWARD);
            if (!input_intact) return rc;
            if (getenv("DFFT_DEBUG")) fprintf(stderr, "[dfft] %s -- running the transform again on the two-launch stage\n", dfft_last_error());
            rc = run();
            if (rc) return rc;
        }
    }
    if (zrc0) return fail(zrc0, zmsg0);  // (asynchronous execute of a P > 1 plan: queued for the peers' sake, invalid all the same)
    // host-synchronised executes have drained the stream: an asynchronous exchange that timed out on a dead or slow peer
    // must not let the caller print timings / use results (the reference-named wrapper always executes this way)
    if (sync && plan->comm) {
        rc = comm_check(plan->comm);
        if (rc) return rc;
    }
    if ((exec_flags & DFFT_EXEC_PRINT) && plan->direction == DFFT_FORWARD) {
        double t[4];
        rc = dfft_stage_times(plan, t);
        if (rc) return rc;
        // fft_mpi_3d_api.cpp:201
        printf("t0: %lf, t1: %lf, t2: %lf, t3: %lf, total: %lf\n", t[0], t[1], t[2], t[3], t[0] + t[1] + t[2] + t[3]);
    }
    return DFFT_OK;
}

// x_variant= of dfft_plan_describe: the kernel form of the forward X pass.  The 512-point fp64 staged store reports what its last launch
// selected (before the first one: what the plan's shape and switches select); every other kernel reports its switch, as before.
static const char* x_variant_name(const dfft_plan_s* p) {
    if (p->x_form & X_FORM_512_F64) {
        const bool early = (p->x_form & X_FORM_EARLY) != 0;
        if (p->x_form & X_FORM_TICKET) return early ? "ticket-early-wait" : "ticket-late-wait";
        return early ? "static-early-wait" : "static-late-wait";
    }
    return (p->x_hints & FFT_HINT_HALF_PREFETCH) ? "half-prefetch" : ((p->x_hints & FFT_HINT_EARLY_WAIT) ? "early-wait" : "default");
}

int dfft_plan_describe(dfft_plan_t plan, char* buf, int len) {
    if (!plan || !buf || len < 64) return fail(DFFT_EINVAL, "dfft_plan_describe: bad arguments");
    const dfft_plan_s* p = plan;
    if (p->conv) return conv_describe(p, buf, len);
    if (p->r2c) {
        snprintf(buf, (size_t)len, "pipeline=%s n2=%lld bins=%lld chunks=%lldx%lld intermediate_pitch=%lld", p->direction == DFFT_FORWARD ? "r2c" : "c2r",
                 p->n2r, p->N[2], p->chunk_planes > 0 ? (p->xs + p->chunk_planes - 1) / p->chunk_planes : 1ll, p->chunk_planes > 0 ? p->chunk_planes : p->xs,
                 p->cl.pitch);
        if (p->real_any) {  // "real_form=3 complex_form=four-step/125x125" or "... complex_form=bluestein/M194/fused"
            const size_t used = strlen(buf);
            int          a = 0, b = 0;
            char         cf[96] = "";
            if (p->real_form == 3 && p->rtab)
                snprintf(cf, sizeof(cf), " complex_form=bluestein/M%lld/%s", p->rtab->M,
                         (p->n2r == 1 || (p->rfused && p->n2r <= kBluesteinFusedMaxLength)) ? "fused" : "multi-pass");
            else if (p->real_form == 3 && long_split(p->n2r, &a, &b))
                snprintf(cf, sizeof(cf), " complex_form=four-step/%dx%d", a, b);
            if (used + 1 < (size_t)len) snprintf(buf + used, (size_t)len - used, " real_form=%d%s", p->real_form, cf);
        }
        return DFFT_OK;
    }
    const bool         one = p->zy_on && !(p->flags & DFFT_PLAN_UNFUSED);
    const long long    cp = one ? zy_phase_planes(p, p->xs, p->exch && p->direction == DFFT_FORWARD) : (p->chunk_planes > 0 ? p->chunk_planes : p->xs);
    const long long    nch = cp > 0 ? (p->xs + cp - 1) / cp : 1;
    const bool         fused = !(p->flags & DFFT_PLAN_UNFUSED);
    snprintf(buf, (size_t)len,
             "pipeline=%s yz_stage=%s%s chunks=%lldx%lld handover=%s rotated_exchange_rows=%d overlap_parts=%lld ysub=%d parts_in_one_launch=%d tuned=%d x_variant=%s",
             (p->flags & DFFT_PLAN_NATURAL) ? "natural" : (fused ? "fused" : "unfused"),
             (p->zy_on && fused) ? "one-launch" : "two-launches-per-chunk", (p->zy_on && fused && p->zy_lazy) ? "-lazy" : "", nch, cp,
             (fused && p->wbuf && !p->exch) ? "padded-buffer" : "bufferDev1", p->rot_elems, p->part_planes, p->ycuts, (p->zy_on && fused && p->zy_part_done) ? 1 : 0, p->w_kept >= 0 ? 1 : 0,
             x_variant_name(p));
    for (int a = 0; a < 3; ++a) {  // Bluestein axes: "bluestein_axis0=n11/M24/fused"
        if (length_kind(p->N[a]) != 3 || p->bs.tables.empty()) continue;
        const size_t used = strlen(buf);
        if (used + 1 >= (size_t)len) break;
        const bool fused = p->N[a] == 1 || (p->bs.fused && p->N[a] <= kBluesteinFusedMaxLength);
        snprintf(buf + used, (size_t)len - used, " bluestein_axis%d=n%lld/M%lld/%s", a, p->N[a], bluestein_padded_length(p->N[a]),
                 fused ? "fused" : "multi-pass");
    }
    return DFFT_OK;
}

int dfft_plan_sync(dfft_plan_t plan) {
    if (!plan) return fail(DFFT_EINVAL, "dfft_plan_sync: null plan");
    if (plan->conv) return conv_sync(plan);
    if (plan->P > 1) trace("dfft_plan_sync enter", plan->direction, plan->flags);
    DFFT_HIP_TRY(hipStreamSynchronize(plan->stream));
    if (plan->P > 1) trace("dfft_plan_sync stream drained", plan->direction, plan->flags);
    {
        const int rc = zy_check(plan);
        if (rc) return rc;
    }
    if (plan->comm) return comm_check(plan->comm);
    return DFFT_OK;
}

int dfft_stage_times(dfft_plan_t plan, double t[4]) {
    if (!plan || !t) return fail(DFFT_EINVAL, "dfft_stage_times: bad arguments");
    if (plan->conv) return conv_stage_times(plan, t);
    DFFT_HIP_TRY(hipStreamSynchronize(plan->stream));
    {
        const int rc = zy_check(plan);
        if (rc) return rc;
    }
    if (plan->comm) {
        const int rc = comm_check(plan->comm);
        if (rc) return rc;
    }
    if (!plan->timed) return fail(DFFT_EINVAL, "dfft_stage_times: the last execute ran with DFFT_EXEC_NO_TIMING");
    if (plan->host_timed) {
        for (int i = 0; i < 4; ++i) t[i] = plan->host_t[i];
        return DFFT_OK;
    }
    for (int i = 0; i < 4; ++i) {
        float ms = 0;
        DFFT_HIP_TRY(hipEventElapsedTime(&ms, plan->ev[i], plan->ev[i + 1]));
        t[i] = ms * 1e-3;
    }
    return DFFT_OK;
}

int dfft_kernel_times(dfft_plan_t plan, double t[3]) {
    if (!plan || !t) return fail(DFFT_EINVAL, "dfft_kernel_times: bad arguments");
    if (plan->conv) return fail(DFFT_EUNSUPPORTED, "dfft_kernel_times: not available for spectral-filter plans");
    if (plan->host_timed || !plan->timed)
        return fail(DFFT_EINVAL, "dfft_kernel_times: needs an execute without DFFT_EXEC_SYNC_STAGES / DFFT_EXEC_NO_TIMING");
    if (plan->flags & DFFT_PLAN_UNFUSED) return fail(DFFT_EINVAL, "dfft_kernel_times: fused plans only");
    if (plan->r2c) return fail(DFFT_EUNSUPPORTED, "dfft_kernel_times: not available for real-to-complex / complex-to-real plans");
    if (plan->zy_on)
        return fail(DFFT_EINVAL, "dfft_kernel_times: not available -- this plan runs its Z and Y passes inside ONE launch (no event between them); "
                                 "create it with DFFT_T0_ONE_LAUNCH=0 to time the passes separately");
    if (plan->chunk_planes > 0 || plan->part_planes > 0)
        return fail(DFFT_EINVAL, "dfft_kernel_times: Z and Y launches are interleaved per cache chunk (set DFFT_CHUNK_MB=0)");
    DFFT_HIP_TRY(hipStreamSynchronize(plan->stream));
    float z = 0, y = 0, x = 0;
    if (plan->direction == DFFT_FORWARD) {
        DFFT_HIP_TRY(hipEventElapsedTime(&z, plan->ev[0], plan->ev[5]));
        DFFT_HIP_TRY(hipEventElapsedTime(&y, plan->ev[5], plan->ev[1]));
        DFFT_HIP_TRY(hipEventElapsedTime(&x, plan->ev[3], plan->ev[4]));
    } else {
        DFFT_HIP_TRY(hipEventElapsedTime(&x, plan->ev[0], plan->ev[1]));
        DFFT_HIP_TRY(hipEventElapsedTime(&y, plan->ev[3], plan->ev[5]));
        DFFT_HIP_TRY(hipEventElapsedTime(&z, plan->ev[5], plan->ev[4]));
    }
    t[0] = z * 1e-3;
    t[1] = y * 1e-3;
    t[2] = x * 1e-3;
    return DFFT_OK;
}

int dfft_plan_destroy(dfft_plan_t plan) {
    if (!plan) return DFFT_OK;
    if (plan->conv) return conv_destroy(plan);
    if (plan->P > 1) trace("dfft_plan_destroy", plan->direction, plan->flags);
    if (plan->stream) hipStreamSynchronize(plan->stream);
    if (plan->stream2) hipStreamSynchronize(plan->stream2);
    const int zy_rc = zy_check(plan);  // an execute nobody synchronised through the library: its failure is reported here at the latest
    if (plan->comm) {  // same order as the registrations (the IPC communicator makes these collective)
        comm_unregister(plan->comm, plan->me, plan->xd2.slot);
        comm_unregister(plan->comm, plan->me, plan->xd.slot);
    }
    for (auto& e : plan->ev)
        if (e) hipEventDestroy(e);
    for (auto& e : plan->part_ev)
        if (e) hipEventDestroy(e);
    if (plan->join_ev) hipEventDestroy(plan->join_ev);
    for (auto& e : plan->y_ev)
        if (e) hipEventDestroy(e);
    if (plan->stream2) hipStreamDestroy(plan->stream2);
    if (plan->stream && !plan->borrowed) hipStreamDestroy(plan->stream);
    (void)comm_recv_free(plan->comm, plan->buf1);
    (void)comm_recv_free(plan->comm, plan->rbuf);
    if (plan->wbuf && !plan->borrowed) slab_free(plan->wbuf);
    if (plan->lbuf) hipFree(plan->lbuf);
    if (plan->bs.scratch) hipFree(plan->bs.scratch);
    if (plan->rscratch) hipFree(plan->rscratch);
    if (plan->cbuf && (!plan->borrowed || plan->own_cbuf)) hipFree(plan->cbuf);
    if (plan->zy_ctl) hipFree(plan->zy_ctl);
    if (plan->x_ticket_ctr) hipFree(plan->x_ticket_ctr);
    if (plan->zy_part_done) hipFree(plan->zy_part_done);
    if (plan->zy_err) hipHostFree(plan->zy_err);
    delete plan;
    return zy_rc;
}

}  // extern "C"
