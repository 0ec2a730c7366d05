// new_points_plan.hpp -- what the entry points of CreateNewMapPoints (csrc/new_map_points.hip) decide before they launch: the
// argument validation, the launch geometry, the per-pair pointer offsets of the chain search -> triangulate, and the layout of the
// host-pointer call's staging block.  Pure host arithmetic, no HIP: tests/new_points_plan_driver.cpp compiles this header with g++
// and tests/test_new_points_cpu.py pins the rules as literals.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <cmath>
#include <cstdio>

#include "../../include/orbfe.h"
#include "host_stage.hpp"   // IoLayout

namespace orbfe {

constexpr int NMP_THREADS = 256;        // both kernels: threads per workgroup
constexpr int NMP_MAX_CAPACITY = 4096;  // features per frame: the bound of the search (its LDS tables) and of k_nmp_prepare's depths in LDS
constexpr int NMP_MAX_LEVELS = 16;      // pyramid levels: the bound of the search's level tables
constexpr int NMP_SEARCH_LAUNCHES = 1;  // kernels orbfe_search_for_triangulation_batch_device launches
constexpr int NMP_INSPECT_FLOATS = 6;   // cosParallaxRays, err1, err2, dist1, dist2, ratioOctave

struct NmpCheck {
    int err = ORBFE_OK;
    char msg[128] = "";
};

inline NmpCheck nmp_fail(int err, const char* name, const char* what)
{
    NmpCheck c;
    c.err = err;
    snprintf(c.msg, sizeof c.msg, "%s: %s", name, what);
    return c;
}

// what every device call shares: the block size, the pair list (both index arrays or none), the intrinsics
inline NmpCheck nmp_check_common(const char* name, int capacity, int npairs, const void* d_pair1, const void* d_pair2, const float* K4)
{
    if (capacity <= 0 || npairs < 0) return nmp_fail(ORBFE_ERR_INVALID, name, "invalid argument");
    if ((d_pair1 == nullptr) != (d_pair2 == nullptr)) return nmp_fail(ORBFE_ERR_INVALID, name, "d_pair1 and d_pair2 are both given or both NULL");
    if (!K4) return nmp_fail(ORBFE_ERR_INVALID, name, "invalid argument");
    for (int i = 0; i < 4; i++)
        if (!std::isfinite(K4[i])) return nmp_fail(ORBFE_ERR_INVALID, name, "K4 is not finite");
    if (K4[0] == 0 || K4[1] == 0) return nmp_fail(ORBFE_ERR_INVALID, name, "a zero focal length");
    if (capacity > NMP_MAX_CAPACITY) return nmp_fail(ORBFE_ERR_CAPACITY, name, "at most 4096 features per frame");
    return NmpCheck{};
}

// the level tables and the ratio of the scale-consistency gate
inline NmpCheck nmp_check_levels(const char* name, const float* scale_factors, const float* level_sigma2, int nlevels, float ratio_factor)
{
    if (!scale_factors || !level_sigma2 || nlevels < 1 || nlevels > NMP_MAX_LEVELS) return nmp_fail(ORBFE_ERR_INVALID, name, "1 to 16 pyramid levels");
    for (int l = 0; l < nlevels; l++)
        if (!std::isfinite(scale_factors[l]) || !std::isfinite(level_sigma2[l]) || scale_factors[l] <= 0 || level_sigma2[l] <= 0)
            return nmp_fail(ORBFE_ERR_INVALID, name, "a level table entry that is not positive and finite");
    if (!(ratio_factor > 0) || !std::isfinite(ratio_factor)) return nmp_fail(ORBFE_ERR_INVALID, name, "ratio_factor must be positive and finite");
    return NmpCheck{};
}

struct NmpGrid { int x = 0, y = 0, block = NMP_THREADS; };
// k_nmp_prepare: one workgroup per pair
inline NmpGrid nmp_prepare_grid(int npairs) { NmpGrid g; g.x = npairs; g.y = 1; return g; }
// k_nmp_triangulate: one thread per side-1 feature, pairs along y
inline NmpGrid nmp_triangulate_grid(int capacity, int npairs) { NmpGrid g; g.x = (capacity + NMP_THREADS - 1) / NMP_THREADS; g.y = npairs; return g; }
// kernels one chain call enqueues: prepare, then search and triangulation per pair
inline int nmp_chain_launches(int npairs) { return 1 + npairs * (NMP_SEARCH_LAUNCHES + 1); }

// Pair p of the chain as a batch of ONE pair.  With index arrays the per-frame blocks stay where they are and the arrays advance by
// p; without them pair p is frames (p, p + 1), which a one-pair batch reads as frames (0, 1) of blocks advanced by p frames.
// Everything indexed by pair advances by p either way.
struct NmpChainStep {
    size_t pair = 0;          // elements of a per-pair array of 1 entry; x capacity, x 9, x 2 ... at the call site
    size_t frame = 0;         // frames to advance the per-frame blocks by
    size_t index = 0;         // entries to advance d_pair1 / d_pair2 by (when they are given)
};
inline NmpChainStep nmp_chain_step(int p, bool have_index)
{
    NmpChainStep s;
    s.pair = (size_t)p;
    s.frame = have_index ? 0 : (size_t)p;
    s.index = have_index ? (size_t)p : 0;
    return s;
}
// element offsets of the per-frame arrays for a step
struct NmpFrameOffsets { size_t per_feature, fv_offset, per_frame, tcw; };
inline NmpFrameOffsets nmp_frame_offsets(const NmpChainStep& s, int capacity)
{
    NmpFrameOffsets o;
    o.per_feature = s.frame * (size_t)capacity;        // x 1 (flags, kps records, fv nodes / features), x 3 (points), x 32 (descriptors)
    o.fv_offset = s.frame * ((size_t)capacity + 1);
    o.per_frame = s.frame;                             // d_n, d_nfv
    o.tcw = s.frame * 12;
    return o;
}

// The staging block of orbfe_create_new_map_points: two frames as a batch of one pair (frame 1 in block 0, frame 2 in block 1 of `cap`
// features).  Inputs, then what goes up and comes back (the map state), then the outputs.
struct NmpHostLayout {
    IoLayout io;
    size_t kps, desc, n, fn, fo, ff, nf, tcw;                     // inputs
    size_t x3Dw, valid, free_;                                    // in-out
    size_t F12, epipole, prep, m12, m21, nm, status, x3D, normal, dist, res, inspect;   // outputs
};
inline NmpHostLayout nmp_host_layout(int cap, bool with_search, bool with_inspect)
{
    NmpHostLayout l;
    const size_t C = (size_t)cap, S = with_search ? C : 0;
    l.kps = l.io.take(2 * C * sizeof(orbfe_keypoint));
    l.desc = l.io.take(2 * S * 32);
    l.n = l.io.take(8);
    l.fn = l.io.take(2 * S * 4);
    l.fo = l.io.take(with_search ? 2 * (C + 1) * 4 : 0);
    l.ff = l.io.take(2 * S * 4);
    l.nf = l.io.take(8);
    l.tcw = l.io.take(24 * 4);
    l.io.inout();
    l.x3Dw = l.io.take(2 * C * 12);
    l.valid = l.io.take(2 * C);
    l.free_ = l.io.take(2 * C);
    l.io.outputs();
    l.F12 = l.io.take(9 * 4);
    l.epipole = l.io.take(2 * 4);
    l.prep = l.io.take(sizeof(orbfe_new_points_pair));
    l.m12 = l.io.take(C * 4);
    l.m21 = l.io.take(S * 4);
    l.nm = l.io.take(4);
    l.status = l.io.take(C);
    l.x3D = l.io.take(C * 12);
    l.normal = l.io.take(C * 12);
    l.dist = l.io.take(C * 8);
    l.res = l.io.take(sizeof(orbfe_new_points_result));
    l.inspect = l.io.take(with_inspect ? C * NMP_INSPECT_FLOATS * 4 : 0);
    return l;
}

} // namespace orbfe
