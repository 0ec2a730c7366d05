/*
 * Optimizer_pose_orbfe.cc (shim) -- Optimizer::PoseOptimization(Frame*) and Optimizer::PoseOptimizationByAruco(Frame*)
 * (src/Optimizer.cc:308-770) implemented on liborbfe.so.  Link it together with src/Optimizer.cc from which these two definitions
 * have been removed (LocalBundleAdjustment has a shim of its own, Optimizer_localba_orbfe.cc; the global bundle adjustment and the
 * essential graph stay the reference's own).  include/Optimizer.h, Frame, MapPoint and MapAruco stay the reference's own.
 *
 * The shim walks the frame on the host -- mvpMapPoints (world positions), and for PoseOptimizationByAruco when Frame::mbUArucoIni
 * the markers with !mvbOldAruco, mvbArucoGood and a MapAruco (Twm, get3DPointsLocalRefSystem, mvArucoUn) -- and makes one
 * orbfe_pose_optimization call.  mvbOutlier is written for every keypoint with a map point, and SetPose receives the optimized pose
 * unless fewer than 3 observations were found (the reference returns 0 without touching the pose).  Like the reference's,
 * PoseOptimizationByAruco leaves stereo observations (mvuRight >= 0) out; PoseOptimization, whose stereo branch is not ported (stereo
 * is dead code in this fork), throws std::runtime_error when it meets one.  Library errors are thrown as std::runtime_error.
 */
#include "Optimizer.h"

#include <cstdint>
#include <stdexcept>
#include <vector>

#include "Frame.h"
#include "MapAruco.h"
#include "MapPoint.h"
#include "orbfe_shim.h"

using namespace std;

namespace ORB_SLAM2
{

using namespace orbfe_shim;

namespace
{

const float kMarkerInformation = 25.f;   // PoseOptimizationByAruco's wei

int pose_optimization(Frame* pFrame, bool markers, const char* name)
{
    const int N = pFrame->N;
    vector<uint8_t> has(N, 0), outlier(N, 0);
    vector<float> x3Dw(3 * (size_t)N, 0.f);
    for (int i = 0; i < N; i++) {
        MapPoint* pMP = pFrame->mvpMapPoints[i];
        if (!pMP) continue;
        if (pFrame->mvuRight[i] >= 0) {
            if (!markers) throw std::runtime_error(string(name) + ": stereo observations are not supported");
            continue;
        }
        point3(pMP->GetWorldPos(), &x3Dw[3 * (size_t)i]);
        has[i] = 1;
        outlier[i] = pFrame->mvbOutlier[i] ? 1 : 0;
    }
    vector<orbfe_pose_marker> mk;
    if (markers && Frame::mbUArucoIni) {
        for (size_t i = 0; i < (size_t)pFrame->NA; i++) {
            if (pFrame->mvbOldAruco[i] || !pFrame->mvbArucoGood[i]) continue;
            MapAruco* pMA = pFrame->mvpMapArucos[i];
            if (!pMA) continue;
            orbfe_pose_marker m;
            const cv::Mat Twm = pMA->GetTwm();
            for (int r = 0; r < 3; r++)
                for (int c = 0; c < 4; c++) m.Twm[r * 4 + c] = Twm.at<float>(r, c);
            for (size_t k = 0; k < 4; k++) {
                m.corners[2 * k] = pFrame->mvArucoUn[4 * i + k].x;
                m.corners[2 * k + 1] = pFrame->mvArucoUn[4 * i + k].y;
                const cv::Point3f p = pMA->get3DPointsLocalRefSystem(k);
                m.local[3 * k] = p.x;
                m.local[3 * k + 1] = p.y;
                m.local[3 * k + 2] = p.z;
            }
            mk.push_back(m);
        }
    }
    float Tin[12], Tout[12];
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 4; c++) Tin[r * 4 + c] = pFrame->mTcw.at<float>(r, c);
    const float K4[4] = {pFrame->fx, pFrame->fy, pFrame->cx, pFrame->cy};
    orbfe_pose_result res;
    check(orbfe_pose_optimization(keys(pFrame->mvKeysUn), N, has.data(), x3Dw.data(), pFrame->mvInvLevelSigma2.data(),
                                  (int)pFrame->mvInvLevelSigma2.size(), K4, mk.data(), (int)mk.size(), kMarkerInformation, Tin, Tout,
                                  outlier.data(), nullptr, &res, 0));
    for (int i = 0; i < N; i++)
        if (has[i]) pFrame->mvbOutlier[i] = outlier[i] != 0;
    if (res.n_initial < 3) return 0;
    cv::Mat pose(4, 4, CV_32F);
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 4; c++) pose.at<float>(r, c) = Tout[r * 4 + c];
    pose.at<float>(3, 0) = pose.at<float>(3, 1) = pose.at<float>(3, 2) = 0.f;
    pose.at<float>(3, 3) = 1.f;
    pFrame->SetPose(pose);
    return res.n_good;
}

} // namespace

int Optimizer::PoseOptimization(Frame* pFrame) { return pose_optimization(pFrame, false, "Optimizer::PoseOptimization"); }

int Optimizer::PoseOptimizationByAruco(Frame* pFrame) { return pose_optimization(pFrame, true, "Optimizer::PoseOptimizationByAruco"); }

} // namespace ORB_SLAM2
