/*
 * Optimizer_sim3_orbfe.cc (shim) -- Optimizer::OptimizeSim3 (src/Optimizer.cc:1544-1739) implemented on liborbfe.so.  Link it together
 * with src/Optimizer.cc from which this definition has been removed.  include/Optimizer.h, KeyFrame, MapPoint and
 * g2o::Sim3 stay the reference's own.
 *
 * The shim walks the two keyframes on the host and makes one orbfe_optimize_sim3 call.  Side 1 is keyframe 1 by feature index
 * (GetMapPointMatches); side 2 holds, at index i2 = vpMatches1[i]->GetIndexInKeyFrame(pKF2), the matched point itself, as the
 * reference reads it.  A match whose point is not observed in keyframe 2 (i2 < 0) is passed as "no match" and stays in vpMatches1,
 * as the reference skips it.  The initial similarity goes through the floats of the C ABI: rotation().toRotationMatrix(),
 * translation() and scale() rounded to float -- what both call sites of LoopClosing.cc built g2oS12 from.  Afterwards vpMatches1
 * gets NULL where the library removed the pair, and g2oS12 the optimized similarity unless the call returned early (fewer than 10
 * pairs left after the first check: the reference returns 0 without writing g2oS12).  Library errors are thrown as
 * std::runtime_error.
 */
#include "Optimizer.h"

#include <cstdint>
#include <stdexcept>
#include <vector>

#include "KeyFrame.h"
#include "MapPoint.h"
#include "orbfe_shim.h"

using namespace std;

namespace ORB_SLAM2
{

using namespace orbfe_shim;

namespace
{

void put_point(MapPoint* pMP, size_t i, vector<float>& x3Dw, vector<uint8_t>& valid)
{
    point3(pMP->GetWorldPos(), &x3Dw[3 * i]);
    valid[i] = pMP->isBad() ? 0 : 1;
}

} // namespace

int Optimizer::OptimizeSim3(KeyFrame* pKF1, KeyFrame* pKF2, vector<MapPoint*>& vpMatches1, g2o::Sim3& g2oS12, const float th2,
                            const bool bFixScale)
{
    const size_t N = vpMatches1.size(), n2 = pKF2->mvKeysUn.size();
    const vector<MapPoint*> vpMapPoints1 = pKF1->GetMapPointMatches();
    if (N > pKF1->mvKeysUn.size() || N > vpMapPoints1.size()) throw std::runtime_error("Optimizer::OptimizeSim3: more matches than features");
    vector<float> x1(3 * N, 0.f), x2(3 * n2, 0.f);
    vector<uint8_t> v1(N, 0), v2(n2, 0);
    vector<int32_t> m12(N, -1), out(N, -1);
    for (size_t i = 0; i < N; i++) {
        if (vpMapPoints1[i]) put_point(vpMapPoints1[i], i, x1, v1);
        MapPoint* pMP2 = vpMatches1[i];
        if (!pMP2) continue;
        const int i2 = pMP2->GetIndexInKeyFrame(pKF2);
        if (i2 < 0 || (size_t)i2 >= n2) continue;
        put_point(pMP2, (size_t)i2, x2, v2);
        m12[i] = i2;
    }
    float T1[12], T2[12], K1[4], K2[4], R12[9], t12[3];
    pose34(pKF1->GetRotation(), pKF1->GetTranslation(), T1);
    intrinsics(pKF1->mK, K1);
    pose34(pKF2->GetRotation(), pKF2->GetTranslation(), T2);
    intrinsics(pKF2->mK, K2);
    const Eigen::Matrix3d R = g2oS12.rotation().toRotationMatrix();
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) R12[3 * r + c] = (float)R(r, c);
        t12[r] = (float)g2oS12.translation()[r];
    }
    orbfe_sim3_opt_result res;
    check(orbfe_optimize_sim3(keys(pKF1->mvKeysUn), (int)N, x1.data(), v1.data(), T1, K1, keys(pKF2->mvKeysUn), (int)n2, x2.data(), v2.data(),
                              T2, K2, m12.data(), pKF1->mvInvLevelSigma2.data(), (int)pKF1->mvInvLevelSigma2.size(), (float)g2oS12.scale(),
                              R12, t12, th2, bFixScale ? 1 : 0, out.data(), &res, 0));
    for (size_t i = 0; i < N; i++)
        if (m12[i] >= 0 && out[i] < 0) vpMatches1[i] = static_cast<MapPoint*>(NULL);
    if (res.more_iterations == 0) return 0;   // the early return: g2oS12 stays
    g2oS12 = g2o::Sim3(Eigen::Quaterniond(res.q12[3], res.q12[0], res.q12[1], res.q12[2]), Eigen::Vector3d(res.t12[0], res.t12[1], res.t12[2]),
                       res.s12);
    return res.n_inliers;
}

} // namespace ORB_SLAM2
