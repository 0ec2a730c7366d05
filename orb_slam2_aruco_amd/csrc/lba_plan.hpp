// lba_plan.hpp -- what the entry points of LocalBundleAdjustment (csrc/local_ba.hip) decide before they launch: the argument
// validation, the layout of the scratch (one list, walked for the offsets and for the kernels' pointers alike), the layout of the
// host-pointer call's staging block, and the launch schedule.  Pure host arithmetic, no HIP: tests/lba_plan_driver.cpp compiles this
// header with g++ and tests/test_lba_plan_cpu.py pins the rules as literals.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "../../include/orbfe.h"
#include "ba_camera.hpp"    // BaCheck, ba_fail
#include "host_stage.hpp"   // IoLayout
#include "lm_rules.hpp"     // LmState

namespace orbfe {

constexpr int LBA_MAXV = ORBFE_LBA_MAX_FREE_POSES;
constexpr int LBA_N = 6 * LBA_MAXV;     // rows of S, and its row stride
constexpr int LBA_PT = 64;              // threads of the per-point kernels: one wave, so that a few thousand points are many workgroups
constexpr int LBA_MAX_LEVELS = BA_MAX_LEVELS;
constexpr int LBA_EBLK = 45;            // doubles of a monocular edge's blocks: A = Jp^T w Jp (21), b (6), W = Jp^T w Jx (6 x 3)
constexpr int LBA_MBLK = 90;            // of a marker edge: Acc (21), bc (6), Amm (21), bm (6), Acm (36)
constexpr size_t LBA_SE3_BYTES = 64;    // sizeof(SE3) of se3_quat.hpp, a device header; local_ba.hip asserts it
constexpr size_t LBA_SOLVE_LDS = 4096;  // what k_lba_solve holds in LDS beside the reduced system, rounded up

struct LbaCtl {
    LmState lm;            // g2o's Levenberg scalars and their rules (lm_rules.hpp), as the dense optimizers run them
    double lambda0;        // the round's initial lambda, for orbfe_lba_inspect
    int it, ok2;
    int iter_go, trial_go, cur, round;
    int stopped, stale, abort_status, bad;
    int nfree_kf, nv, aborted, pad0;
    int iters[2], n_level1[2];
    int n_erase, stale_mask, pad1, pad2;
};
static_assert(sizeof(LbaCtl) == 144, "the scratch layout and tests/test_lba_plan_cpu.py pin this size");

struct LbaSizes {
    int nkf, np, nobs, nma, nmobs;
};

// The problem as the caller gives it, host pointers or device pointers.  The observations are values (obs_xy, obs_octave) or, in
// the device call only, features of resident keypoint blocks (obs_feature, kps, capacity).
struct LbaProblem {
    LbaSizes n;
    float* Tcw; const uint8_t* kf_fixed; float* x3Dw; const int32_t* obs_offset; const int32_t* obs_kf; const float* obs_xy;
    const int32_t* obs_octave; const int32_t* obs_feature; const orbfe_keypoint* kps; int capacity;
    float* Twm; const float* marker_local; const int32_t* mobs_offset; const int32_t* mobs_kf; const float* mobs_corners;
};

// ---------------------------------------------------------------------------------------- validation --
inline bool lba_sizes_ok(const LbaSizes& n)
{
    return n.nkf >= 0 && n.np >= 0 && n.nobs >= 0 && n.nma >= 0 && n.nmobs >= 0 &&
           (size_t)std::max(n.nkf, 1) * (size_t)std::max(n.np, 1) < ((size_t)1 << 30) && n.nmobs < (1 << 24);
}

// the checks of the host calls (the device call leaves them to k_lba_setup / k_lba_begin)
inline BaCheck lba_check_host(const LbaProblem& pb, int nlevels, int use_markers, const char* name)
{
    const int nkf = pb.n.nkf, np = pb.n.np, nobs = pb.n.nobs, nma = pb.n.nma, nmobs = pb.n.nmobs;
    if (!lba_sizes_ok(pb.n) || (nkf && (!pb.Tcw || !pb.kf_fixed)) || (np && (!pb.x3Dw || !pb.obs_offset)) ||
        (nobs && (!pb.obs_kf || !pb.obs_xy || !pb.obs_octave || !np)) || (nma && (!pb.Twm || !pb.marker_local || !pb.mobs_offset)) ||
        (nmobs && (!pb.mobs_kf || !pb.mobs_corners || !nma)))
        return ba_fail(ORBFE_ERR_INVALID, "%s: invalid argument", name);
    auto fin = [](const float* v, size_t n) {
        for (size_t i = 0; i < n; i++)
            if (!std::isfinite(v[i])) return false;
        return true;
    };
    if (!fin(pb.Tcw, (size_t)nkf * 12) || !fin(pb.x3Dw, (size_t)np * 3) || !fin(pb.obs_xy, (size_t)nobs * 2) || !fin(pb.Twm, (size_t)nma * 12) ||
        !fin(pb.marker_local, (size_t)nma * 12) || !fin(pb.mobs_corners, (size_t)nmobs * 8))
        return ba_fail(ORBFE_ERR_INVALID, "%s: an input is not finite", name);
    const int32_t *off = pb.obs_offset, *moff = pb.mobs_offset;
    if (np && (off[0] != 0 || off[np] != nobs)) return ba_fail(ORBFE_ERR_INVALID, "%s: obs_offset does not span [0, nobs]", name);
    if (!np && nobs) return ba_fail(ORBFE_ERR_INVALID, "%s: observations without points", name);
    for (int i = 0; i < np; i++)
        if (off[i + 1] < off[i]) return ba_fail(ORBFE_ERR_INVALID, "%s: obs_offset decreases at point %d", name, i);
    if (nma && (moff[0] != 0 || moff[nma] != nmobs)) return ba_fail(ORBFE_ERR_INVALID, "%s: mobs_offset does not span [0, nmobs]", name);
    for (int i = 0; i < nma; i++)
        if (moff[i + 1] < moff[i]) return ba_fail(ORBFE_ERR_INVALID, "%s: mobs_offset decreases at marker %d", name, i);
    for (int e = 0; e < nobs; e++) {
        if (pb.obs_kf[e] < 0 || pb.obs_kf[e] >= nkf)
            return ba_fail(ORBFE_ERR_INVALID, "%s: observation %d names keyframe %d of %d", name, e, pb.obs_kf[e], nkf);
        if (pb.obs_octave[e] < 0 || pb.obs_octave[e] >= nlevels)
            return ba_fail(ORBFE_ERR_INVALID, "%s: observation %d has octave %d, outside [0, %d)", name, e, pb.obs_octave[e], nlevels);
    }
    for (int e = 0; e < nmobs; e++)
        if (pb.mobs_kf[e] < 0 || pb.mobs_kf[e] >= nkf)
            return ba_fail(ORBFE_ERR_INVALID, "%s: marker observation %d names keyframe %d of %d", name, e, pb.mobs_kf[e], nkf);
    std::vector<int> seen((size_t)std::max(nkf, 1), -1);
    for (int i = 0; i < np; i++)
        for (int e = off[i]; e < off[i + 1]; e++) {
            if (seen[(size_t)pb.obs_kf[e]] == i) return ba_fail(ORBFE_ERR_INVALID, "%s: keyframe %d observes point %d twice", name, pb.obs_kf[e], i);
            seen[(size_t)pb.obs_kf[e]] = i;
        }
    int nv = use_markers ? nma : 0;
    for (int k = 0; k < nkf; k++) nv += pb.kf_fixed[k] == 0;
    if (nv > LBA_MAXV)
        return ba_fail(ORBFE_ERR_CAPACITY, "%s: %d free pose vertices (keyframes and markers), at most ORBFE_LBA_MAX_FREE_POSES = %d", name, nv, LBA_MAXV);
    for (int i = 0; i < np; i++)
        if (off[i + 1] - off[i] > ORBFE_LBA_MAX_OBSERVATIONS)
            return ba_fail(ORBFE_ERR_CAPACITY, "%s: point %d has %d observations, at most ORBFE_LBA_MAX_OBSERVATIONS = %d", name, i, off[i + 1] - off[i],
                           ORBFE_LBA_MAX_OBSERVATIONS);
    return BaCheck{};
}

// the arguments of the device call: which pointers each observation form needs, the alignment of the scratch.  Nothing is read.
inline BaCheck lba_check_device(const LbaProblem& d, const void* d_erase, const void* d_res, const void* d_scratch, const char* name)
{
    const LbaSizes& n = d.n;
    const bool form_xy = d.obs_xy != nullptr;
    if (!lba_sizes_ok(n) || !d_res || !d_scratch || ((uintptr_t)d_scratch & 255) || (n.nkf && (!d.Tcw || !d.kf_fixed)) ||
        (n.np && (!d.x3Dw || !d.obs_offset)) || (n.nobs && (!d.obs_kf || !d_erase || !n.np)) || (n.nobs && form_xy && !d.obs_octave) ||
        (n.nobs && !form_xy && (!d.obs_feature || !d.kps || d.capacity <= 0)) || (n.nma && (!d.Twm || !d.marker_local || !d.mobs_offset)) ||
        (n.nmobs && (!d.mobs_kf || !d.mobs_corners || !n.nma)))
        return ba_fail(ORBFE_ERR_INVALID, "%s: invalid argument", name);
    return BaCheck{};
}

// ---------------------------------------------------------------------------------------- scratch layout --
inline int lba_point_blocks(int np) { return (np + LBA_PT - 1) / LBA_PT; }              // workgroups of a pass over the points
inline int lba_marker_blocks(int nmobs) { return (4 * nmobs + LBA_PT - 1) / LBA_PT; }    // over the marker corner edges, 4 an observation

// the offsets of the scratch arrays, named as the kernels' argument (LbaP of local_ba.hip) names its pointers
struct LbaLayout {
    size_t ctl, xv, xl, e_chi2, m_chi2, e_level, m_level, pose[2], pt[2], e_kf, e_pt, e_ox, e_oy, e_info, e_use, e_blk, mo_marker, m_use, m_blk, Hll,
        bl, Dinv, p_active, Hpp, bp, vmax, v_active, v_kf, kf_free, tbl, S, bs, chi_part, scale_part, max_part;
};
struct LbaExtent {
    size_t zero_end, tbl_bytes, end;   // [0, zero_end) is zeroed and the table set to -1 at every call
};

// gives a field its array: an offset (LbaLayout), or the pointer at that offset of `base` (LbaP)
struct LbaTake {
    IoLayout o;
    unsigned char* base = nullptr;
    void operator()(size_t& f, size_t bytes) { f = o.take(bytes); }
    template <class T> void operator()(T*& f, size_t bytes) { f = (T*)(base + o.take(bytes)); }
};

// THE list of the scratch arrays, in their order.  An array of no elements still has one: a size of 0 is a valid problem.
template <class A> LbaExtent lba_scratch(A& a, const LbaSizes& n, void* base = nullptr)
{
    LbaTake take;
    take.base = (unsigned char*)base;
    LbaExtent x;
    const size_t K = (size_t)std::max(n.nkf, 1), P = (size_t)std::max(n.np, 1), E = (size_t)std::max(n.nobs, 1), M = (size_t)std::max(n.nma, 1),
                 MO = (size_t)std::max(n.nmobs, 1), ME = 4 * MO, NB = (size_t)std::max(lba_point_blocks(n.np) + lba_marker_blocks(n.nmobs), 1);
    // zeroed at every call: the state, the updates, the chi2 caches (an edge no pass evaluated has g2o's initial error 0), the levels
    take(a.ctl, sizeof(LbaCtl));
    take(a.xv, LBA_N * 8);
    take(a.xl, P * 24);
    take(a.e_chi2, E * 8);
    take(a.m_chi2, ME * 8);
    take(a.e_level, E);
    take(a.m_level, ME);
    x.zero_end = take.o.end();
    for (int k = 0; k < 2; k++) take(a.pose[k], (K + M) * LBA_SE3_BYTES);   // nkf keyframes, then nma markers
    for (int k = 0; k < 2; k++) take(a.pt[k], P * 24);
    take(a.e_kf, E * 4); take(a.e_pt, E * 4); take(a.e_ox, E * 4); take(a.e_oy, E * 4); take(a.e_info, E * 4);
    take(a.e_use, E);
    take(a.e_blk, E * LBA_EBLK * 8);
    take(a.mo_marker, MO * 4);
    take(a.m_use, ME);
    take(a.m_blk, ME * LBA_MBLK * 8);
    take(a.Hll, P * 48); take(a.bl, P * 24); take(a.Dinv, P * 72); take(a.p_active, P);
    take(a.Hpp, LBA_MAXV * 36 * 8); take(a.bp, LBA_N * 8); take(a.vmax, LBA_MAXV * 8);
    take(a.v_active, LBA_MAXV * 4); take(a.v_kf, LBA_MAXV * 4); take(a.kf_free, K * 4);
    x.tbl_bytes = K * P * 4;
    take(a.tbl, x.tbl_bytes);   // nkf x np: the edge of (keyframe, point), -1 none
    take(a.S, (size_t)LBA_N * LBA_N * 8); take(a.bs, LBA_N * 8);
    take(a.chi_part, NB * 8); take(a.scale_part, NB * 8); take(a.max_part, NB * 8);
    x.end = take.o.end();
    return x;
}

inline size_t lba_scratch_bytes(const LbaSizes& n)
{
    LbaLayout l;
    return lba_scratch(l, n).end;
}

inline BaCheck lba_check_scratch(const LbaSizes& n, size_t scratch_bytes, const char* name)
{
    const size_t need = lba_scratch_bytes(n);
    if (scratch_bytes < need) return ba_fail(ORBFE_ERR_CAPACITY, "%s: %zu bytes of scratch, orbfe_lba_scratch_bytes asks for %zu", name, scratch_bytes, need);
    return BaCheck{};
}

// ---------------------------------------------------------------------------------------- the host call's staging block --
// everything up, the estimates up and back, the erase bytes and the record down
struct LbaHostIo {
    IoLayout io;
    size_t fixed, off, kf, xy, oct, mloc, moff, mkf, mcor;   // inputs
    size_t T, X, M;                                          // in-out
    size_t erase, res;                                       // outputs
};
inline LbaHostIo lba_host_io(const LbaSizes& n)
{
    const size_t K = (size_t)std::max(n.nkf, 1), P = (size_t)std::max(n.np, 1), E = (size_t)std::max(n.nobs, 1), M = (size_t)std::max(n.nma, 1),
                 MO = (size_t)std::max(n.nmobs, 1);
    LbaHostIo l;
    IoLayout& o = l.io;
    l.fixed = o.take(K); l.off = o.take((P + 1) * 4); l.kf = o.take(E * 4); l.xy = o.take(E * 8); l.oct = o.take(E * 4);
    l.mloc = o.take(M * 48); l.moff = o.take((M + 1) * 4); l.mkf = o.take(MO * 4); l.mcor = o.take(MO * 32);
    o.inout();
    l.T = o.take(K * 48); l.X = o.take(P * 12); l.M = o.take(M * 48);
    o.outputs();
    l.erase = o.take(E); l.res = o.take(sizeof(orbfe_lba_result));
    return l;
}

// ---------------------------------------------------------------------------------------- the launch schedule --
// The host enqueues the same kernels whatever the problem does: a round is a begin (and, before round 2, the first check), `maxit`
// iterations of linearize / pose_blocks / ctl_lin and `trials` trials each of schur_points / assemble / solve / backsub / ctl_trial;
// setup before, the second check and finish after.  An inspect call is setup, one begin, one iteration with one trial and no ctl_trial.
struct LbaSchedule {
    int npb, nb;             // workgroups of LBA_PT threads over the points; those and the ones over the marker corner edges (when in use)
    int g_setup;             // grids, each at least 1.  k_lba_setup, k_lba_finish: 256 threads over the longest of the caller's arrays
    int g_pass;              // k_lba_linearize, k_lba_backsub: nb
    int g_points;            // k_lba_schur_points: npb
    int g_edges;             // k_lba_check: 256 threads over the edges
    int vmax;                // k_lba_pose_blocks (vmax), k_lba_assemble (vmax x vmax): the device counts the free vertices, this bounds them
    int lds_rows;            // rows of the reduced system k_lba_solve may factor in LDS: the most that fit, 6 a vertex
    size_t tri_bytes;        // the dynamic LDS of that, a packed lower triangle of doubles
    int rounds, maxit[2], trials;
    int launches;            // kernels one call enqueues
};
inline LbaSchedule lba_schedule(const LbaSizes& n, bool use_markers, bool inspect, size_t lds_limit)
{
    LbaSchedule s;
    const int nme = use_markers ? 4 * n.nmobs : 0;
    s.npb = lba_point_blocks(n.np);
    s.nb = s.npb + (use_markers ? lba_marker_blocks(n.nmobs) : 0);
    s.g_setup = std::max((std::max(std::max(n.nobs, n.np), std::max(n.nkf + n.nma, n.nmobs)) + 255) / 256, 1);
    s.g_pass = std::max(s.nb, 1);
    s.g_points = std::max(s.npb, 1);
    s.g_edges = std::max((n.nobs + nme + 255) / 256, 1);
    s.vmax = std::max(1, std::min(LBA_MAXV, n.nkf + (use_markers ? n.nma : 0)));
    s.lds_rows = 6 * s.vmax;
    while (s.lds_rows > 0 && (size_t)s.lds_rows * (s.lds_rows + 1) / 2 * 8 + LBA_SOLVE_LDS > lds_limit) s.lds_rows -= 6;
    s.tri_bytes = (size_t)s.lds_rows * (s.lds_rows + 1) / 2 * 8;
    s.rounds = inspect ? 1 : 2;
    s.maxit[0] = inspect ? 1 : 5;
    s.maxit[1] = inspect ? 0 : 10;
    s.trials = inspect ? 1 : 10;
    s.launches = 1 + (inspect ? 0 : 2);
    for (int r = 0; r < s.rounds; r++) s.launches += 1 + (r == 1) + s.maxit[r] * (3 + s.trials * (inspect ? 4 : 5));
    return s;
}

} // namespace orbfe
