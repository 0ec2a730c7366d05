// ba_camera.hpp -- the step the optimizers of pose_optimizer.hip and local_ba.hip share before anything else: the intrinsics and
// marker_info checked, the table of inverse level sigma^2 padded with zeros to BA_MAX_LEVELS, the Huber delta.  Also the check
// record (error code and message) their host-only rules return.  Pure host arithmetic, no HIP: tests/lba_plan_driver.cpp compiles
// this header with g++ and tests/test_lba_plan_cpu.py pins the rules as literals.
#pragma once
#include <cmath>
#include <cstdarg>
#include <cstdio>

#include "../../include/orbfe.h"

namespace orbfe {

constexpr int BA_MAX_LEVELS = 32;

struct BaCheck {
    int err = ORBFE_OK;
    char msg[256] = "";
};

__attribute__((format(printf, 2, 3))) inline BaCheck ba_fail(int err, const char* fmt, ...)
{
    BaCheck c;
    c.err = err;
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(c.msg, sizeof c.msg, fmt, ap);
    va_end(ap);
    return c;
}

struct BaCamera {
    float fx, fy, cx, cy, marker_info;
    int nlevels;
    double delta;                       // (double)(float)sqrt(chi2_delta), as deltaMono reaches RobustKernelHuber::setDelta
    float inv_sigma2[BA_MAX_LEVELS];    // zeros from nlevels on
};

// the sigma table's entries are not looked at: local_ba.hip refuses a non-finite one, pose_optimizer.hip takes them as they are.
// chi2_delta: the square of the Huber delta as the reference writes it (5.991 in PoseOptimization and LocalBundleAdjustment, 5.99 in
// BundleAdjustment)
inline BaCheck ba_camera(BaCamera& c, const float* K4, const float* inv_sigma2, int nlevels, float marker_info, const char* name,
                         double chi2_delta = 5.991)
{
    if (!K4 || !inv_sigma2 || nlevels <= 0 || nlevels > BA_MAX_LEVELS) return ba_fail(ORBFE_ERR_INVALID, "%s: invalid K4 / sigma table", name);
    for (int i = 0; i < 4; i++)
        if (!std::isfinite(K4[i])) return ba_fail(ORBFE_ERR_INVALID, "%s: K is not finite", name);
    if (K4[0] == 0 || K4[1] == 0) return ba_fail(ORBFE_ERR_INVALID, "%s: fx or fy is 0", name);
    if (!std::isfinite(marker_info)) return ba_fail(ORBFE_ERR_INVALID, "%s: marker_info is not finite", name);
    c.fx = K4[0]; c.fy = K4[1]; c.cx = K4[2]; c.cy = K4[3];
    c.marker_info = marker_info;
    c.nlevels = nlevels;
    c.delta = (double)(float)std::sqrt(chi2_delta);
    for (int l = 0; l < BA_MAX_LEVELS; l++) c.inv_sigma2[l] = l < nlevels ? inv_sigma2[l] : 0.f;
    return BaCheck{};
}

} // namespace orbfe

#ifdef __HIPCC__
// for the entry points (hipcc only; the rules above stay free of HIP)
#include "orbfe_common.hpp"

namespace orbfe {

// what a host-only rule found, as the entry points return it
inline int report(const BaCheck& c) { return c.err ? fail(c.err, "%s", c.msg) : ORBFE_OK; }

// what a call is given beside its arrays, into the kernels' argument: the camera and the level table (every entry finite here), the
// marker weight and switch, the Huber delta of chi2_delta (ba_camera.hpp)
template <class P>
int ba_fill(P& p, const float* K4, const float* inv_sigma2, int nlevels, float marker_info, int use_markers, double chi2_delta, const char* name)
{
    BaCamera c;
    const int rc = report(ba_camera(c, K4, inv_sigma2, nlevels, marker_info, name, chi2_delta));
    if (rc) return rc;
    for (int l = 0; l < nlevels; l++)
        if (!std::isfinite(inv_sigma2[l])) return fail(ORBFE_ERR_INVALID, "%s: inv_level_sigma2 is not finite", name);
    p.nlevels = nlevels;
    for (int l = 0; l < BA_MAX_LEVELS; l++) p.inv_sigma2[l] = c.inv_sigma2[l];
    p.K = {c.fx, c.fy, c.cx, c.cy};
    p.marker_info = marker_info;
    p.delta = c.delta;
    p.use_markers = use_markers != 0;
    return ORBFE_OK;
}

} // namespace orbfe
#endif
