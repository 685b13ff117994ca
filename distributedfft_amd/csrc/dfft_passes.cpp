// dfft_passes.cpp -- the passes plans and plan-less entry points share: contiguous rows of any kind of length, Bluestein transforms
// along any axis, and the context of the plan that is executing on this thread (its scratch, grid cap and Bluestein tables).
#include "dfft_plan_impl.h"

namespace dfft {

AxisMap plain_axis(long long n, long long stride, long long cstride) {
    AxisMap m;
    m.blk = (int)n;
    m.nblk = 1;
    m.blk_stride = 0;
    m.stride = stride;
    m.cstride = cstride;
    m.last_delta = 0;
    m.sub = 1;
    m.sub_stride = 0;
    return m;
}

int check_launch(hipError_t e, const char* what) {
    if (e == hipSuccess) return DFFT_OK;
    if (e == hipErrorInvalidValue) return fail(DFFT_EUNSUPPORTED, std::string(what) + ": no gfx950 kernel for this length/precision");
    return fail(DFFT_EHIP, std::string(what) + ": " + hipGetErrorString(e));
}

// the plan that is executing on this thread (ExecutingPlan): its scratch slab (long-axis plans), its cap on the row launches' grids
// (dfft_plan_s::grid_z) and its Bluestein axes
static thread_local void*                t_plan_scratch = nullptr;
static thread_local int                  t_plan_zgrid = 0;
static thread_local const PlanBluestein* t_plan_bs = nullptr;

ExecutingPlan::ExecutingPlan(const dfft_plan_s* p) {
    t_plan_scratch = p->lbuf;
    t_plan_zgrid = p->grid_z;
    t_plan_bs = p->bs.tables.empty() ? nullptr : &p->bs;
}
ExecutingPlan::~ExecutingPlan() {
    t_plan_scratch = nullptr;
    t_plan_zgrid = 0;
    t_plan_bs = nullptr;
}

int bluestein_pass(const void* in, void* out, long long n, long long s, long long batch, int dtype, int dir, double scale, hipStream_t st) {
    if (const PlanBluestein* pb = t_plan_bs) {
        for (const auto& t : pb->tables)
            if (t->n == n && t->dtype == dtype && t->dir == dir) return bluestein_fft(*t, in, out, s, batch, scale, pb->fused, pb->scratch, pb->bytes, st);
        return fail(DFFT_EINVAL, "Bluestein pass: the plan has no tables for length " + std::to_string(n));
    }
    BluesteinTablesPtr t;
    int                rc = bluestein_tables(n, dtype, dir, &t);
    if (rc) return rc;
    const bool   fused = bluestein_fused_env();
    const size_t need = bluestein_scratch_bytes(*t, s, batch, fused, chunk_cap_env());
    ScratchLease lease;
    if (need && !lease.acquire(need, st)) return fail(DFFT_EHIP, "Bluestein pass: cannot allocate the scratch buffer");
    return bluestein_fft(*t, in, out, s, batch, scale, fused, lease.get(), need, st);
}

int fft_rows(const void* in, void* out, int n, long long rows, int dtype, int dir, hipStream_t s, long long first_row, int hints, double scale,
             const SlabLayout* lin, const SlabLayout* lout, long long rows_per_plane, void* long_scratch_buf, int grid_limit) {
    if (length_kind(n) == 3) {  // Bluestein (DFFT_PLAN_ANY_LENGTH plans, which run un-fused): plain contiguous rows only
        if (lin || lout) return fail(DFFT_EINVAL, "fft_rows: Bluestein axes use the natural layout");
        if (rows <= 0) return DFFT_OK;
        const size_t off = (size_t)first_row * n * elem_bytes(dtype);
        return bluestein_pass((const char*)in + off, (char*)out + off, n, 1, rows, dtype, dir, scale, s);
    }
    if (n > 4096) {  // beyond the single-pass range: four-step decomposition (dfft_long.hip), plain contiguous rows only
        if (lin || lout) return fail(DFFT_EINVAL, "fft_rows: long axes use the natural layout");
        if (rows <= 0) return DFFT_OK;
        const size_t off = (size_t)first_row * n * elem_bytes(dtype);
        void*        scr = long_scratch_buf ? long_scratch_buf : t_plan_scratch;
        ScratchLease lease;  // callers without a scratch of their own
        if (!scr && lease.acquire((size_t)rows * n * elem_bytes(dtype), s)) scr = lease.get();
        if (!scr) return fail(DFFT_EHIP, "fft_rows: cannot allocate the scratch buffer of the four-step transform");
        return long_fft((const char*)in + off, (char*)out + off, n, 1, rows, dtype, dir, scale, scr, s);
    }
    const void* tw = nullptr;
    int         rc = get_twiddles(n, dtype, &tw);
    if (rc) return rc;
    FftLaunch L;
    std::memset(&L, 0, sizeof(L));
    L.dtype = dtype;
    L.n = n;
    L.dir = dir;
    L.cols = 0;
    L.in = in;
    L.out = out;
    L.tw = tw;
    L.imap = L.omap = plain_axis(n, 1, 0);
    L.itile = L.otile = TileMap{(long long)n, 0};
    L.ntiles = rows;
    L.a_first = first_row;
    L.hints = hints;
    L.scale = scale;
    L.tiles_per_a = 1;
    L.ncols = 1;
    if (lin && lout && rows_per_plane > 0) {  // tile = (plane a, row b): base = a * plane + b * pitch (CB = 1 for rows)
        if (first_row % rows_per_plane != 0 || rows_per_plane >= (1ll << 31)) return fail(DFFT_EINVAL, "fft_rows: chunk is not whole planes");
        L.itile = TileMap{lin->plane, lin->pitch};
        L.otile = TileMap{lout->plane, lout->pitch};
        L.tiles_per_a = (int)rows_per_plane;
        L.a_first = first_row / rows_per_plane;
    }
    L.grid_limit = grid_limit ? grid_limit : t_plan_zgrid;  // (dfft_plan_s::grid_z: DFFT_Z_GRID when the plan was created)
    return check_launch(launch_fft(L, s), "fft_rows");
}

}  // namespace dfft
