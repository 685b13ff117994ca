// dfft_fused_host.h -- the host scaffold shared by the fused 1-D real kernel families (dfft_rconv.hip, dfft_osconv.hip, dfft_lconv.hip,
// dfft_stft.hip, dfft_xspec.hip, dfft_lxspec.hip, dfft_csd.hip): the grid of an element-wise kernel, the chunking of a composed form
// against its scratch lease, the environment switches, the descriptor of contiguous real rows, the cut of a sum into slices, and the
// dispatch on the tuned lengths of dfft_plans.h.  Plain functions; what a unit decides (its *_fused_ok table, its constants, its
// messages) stays in the unit.  Internal header.
#pragma once
#include "dfft_fft_impl.h"
#include "dfft_internal.h"
#include "dfft_plans.h"
#include "dfft_rconv_impl.h"
#include "dfft_real.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>

namespace dfft {

// grid of an element-wise kernel of 256 threads per workgroup that strides over `total` elements
inline unsigned elementwise_grid(long long total) {
    return (unsigned)std::max(1ll, std::min((total + 255) / 256, (long long)device_info().cus * 16));
}

// units (rows, items) of `unit_bytes` each per chunk: what fits `cap` (chunk_cap_env, read once by the entry point), at least one and at
// least `at_least`, at most all of them
inline long long chunk_units(size_t unit_bytes, long long units, size_t cap, long long at_least = 1) {
    const long long fit = (long long)(std::max(cap, unit_bytes) / unit_bytes);
    return std::max(1ll, std::min(units, std::max(fit, at_least)));
}

// `chunk` units cut down to what the lease holds; 0, behind fail("<who>: scratch buffer too small"), where that is fewer than `at_least`
inline long long fit_chunk_to_lease(const char* who, long long chunk, size_t unit_bytes, const void* scratch, size_t scratch_bytes,
                                    long long at_least = 1) {
    if (scratch_bytes / unit_bytes < (size_t)chunk) chunk = (long long)(scratch_bytes / unit_bytes);
    if (!scratch || chunk < at_least) {
        fail(DFFT_EINVAL, std::string(who) + ": scratch buffer too small");
        return 0;
    }
    return chunk;
}

// a switch that is on unless the environment variable `name` starts with '0' (read per call)
inline bool env_switch_on(const char* name) {
    const char* e = getenv(name);
    return !(e && *e == '0');
}

// `rows` contiguous rows [rows][m] reals <-> [rows][m/2 + 1] bins as one launch of the real-row kernels (dir: +1 R2C, -1 C2R)
inline RealLaunch contiguous_real_rows(int dtype, long long m, long long rows, int dir, double scale, const void* in, void* out) {
    RealLaunch R;
    std::memset(&R, 0, sizeof(R));
    R.dtype = dtype;
    R.n2 = (int)m;
    R.rows = rows;
    R.rows_per_plane = rows;
    R.rpitch = m;
    R.rplane = rows * m;
    R.cpitch = m / 2 + 1;
    R.cplane = rows * (m / 2 + 1);
    R.scale = scale;
    R.dir = dir;
    R.in = in;
    R.out = out;
    return R;
}

// ---- dispatch on the tuned lengths -----------------------------------------------------------------------------------------------
// A family is a tag type:
//     struct Tag {
//         using Launch = ...;                                                       // one fused launch
//         static constexpr bool ok(int N, ...);                                     // the unit's *_fused_ok (tuned_built)
//         template <int N> static hipError_t run(const Launch&, hipStream_t);       // defined in the instantiation groups only
//     };
// FusedInst<Tag, true, N>::run is the entry point of the tuned length N: defined here for the instantiation groups, explicitly
// instantiated by DFFT_FUSED_INSTANTIATE(Tag) in the translation unit of N's group only, and called through run_tuned by the dispatcher.
template <class Tag, bool ON, int N> struct FusedInst {};
template <class Tag, int N> struct FusedInst<Tag, true, N> {
    static hipError_t run(const typename Tag::Launch& F, hipStream_t stream);
};

#if defined(DFFT_INST_GROUP) && DFFT_INST_GROUP < DFFT_NUM_INST_GROUPS
template <class Tag, int N> hipError_t FusedInst<Tag, true, N>::run(const typename Tag::Launch& F, hipStream_t stream) {
    return Tag::template run<N>(F, stream);
}
// every entry point of the translation unit's group (one family per translation unit; behind the definition of Tag::run)
#define DFFT_FUSED_INST(N, GRP, E, ...) template struct FusedInst<FusedUnitTag, (GRP == DFFT_INST_GROUP), N>;
#define DFFT_FUSED_INSTANTIATE(Tag) \
    using FusedUnitTag = Tag;       \
    DFFT_PLAN_TABLE(DFFT_FUSED_INST)
#endif

// the fused launch of the tuned length N; hipErrorInvalidValue for any other N
template <class Tag> hipError_t run_tuned(long long N, const typename Tag::Launch& F, hipStream_t stream) {
    switch (N) {
#define DFFT_FUSED_CASE(N, GRP, E, ...) \
    case N: return FusedInst<Tag, true, N>::run(F, stream);
        DFFT_PLAN_TABLE(DFFT_FUSED_CASE)
#undef DFFT_FUSED_CASE
        default: return hipErrorInvalidValue;
    }
}

// N is a tuned length whose instantiation Tag::ok(N, args...) says is built
template <class Tag, class... A> bool tuned_built(long long N, A... args) {
    switch (N) {
#define DFFT_FUSED_BUILT(N, GRP, E, ...) \
    case N: return Tag::ok(N, args...);
        DFFT_PLAN_TABLE(DFFT_FUSED_BUILT)
#undef DFFT_FUSED_BUILT
        default: return false;
    }
}
// tuned_built<AnyTuned>(N): N has a tuned plan
struct AnyTuned {
    static constexpr bool ok(int) { return true; }
};

// ---- slices of a sum ---------------------------------------------------------------------------------------------------------------
// thread groups per workgroup of a fused kernel of half-length M with the geometry RconvGeom (1 for an untuned M)
inline int groups_per_workgroup(long long M) {
    switch (M) {
#define DFFT_FUSED_G(N, GRP, E, ...) \
    case N: return RconvGeom<double2, PlanFor<N>::type>::G;
        DFFT_PLAN_TABLE(DFFT_FUSED_G)
#undef DFFT_FUSED_G
        default: return 1;
    }
}
// The `inner` terms (rows of a batch, frames of a row) of each of `outer` sums cut into slices, one thread group each: about
// 512 (the resident workgroups of a 256-CU part at two per CU) times min(groups_per_wg, group_cap) items, a slice of at least
// `min_inner` terms.  Fixed constants, never the device.
inline long long slice_count(int groups_per_wg, long long group_cap, long long outer, long long inner, long long min_inner) {
    const long long target = 512 * std::min<long long>(groups_per_wg, group_cap);
    return std::max(1ll, std::min(target / outer, inner / min_inner));
}

}  // namespace dfft
