/*
 * Optimizer_globalba_orbfe.cc (shim) -- Optimizer::BundleAdjustment(vpKFs, vpMP, vpMA, nIterations, pbStopFlag, nLoopKF, bRobust)
 * (src/Optimizer.cc:50-307) implemented on liborbfe.so.  Link it together with src/Optimizer.cc from which that definition has been
 * removed; Optimizer::GlobalBundleAdjustemnt, which gathers the whole map and calls it, stays the reference's.
 * include/Optimizer.h, KeyFrame, MapPoint and MapAruco stay the reference's own.
 *
 * Collect (host), in the reference's order: the keyframes that are not bad (fixed: mnId == 0); the map points that are not bad,
 * each with its observations in the order of its observation map -- an observation in a bad keyframe, or in a keyframe that is not
 * among the collected ones, gives no edge (the reference passes over an observer with mnId > maxKFid; one it was not given at all it
 * would hand to g2o without a vertex); with Frame::mbUArucoIni the map markers that are not bad, their observers being those among
 * the collected keyframes.  ONE orbfe_global_bundle_adjustment call.
 * Apply (:243-304): with nLoopKF == 0 SetPose of the keyframes, SetWorldPos + UpdateNormalAndDepth of the points; otherwise mTcwGBA /
 * mPosGBA and mnBAGlobalForKF = nLoopKF, for LoopClosing::RunGlobalBundleAdjustment to propagate.  A point without an edge is left out
 * (vbNotIncludedMP); a keyframe or point that went bad meanwhile is passed over.  With Frame::mbUArucoIni SetRtwm of the markers, in
 * the nLoopKF != 0 case as well, as the reference does.  A keyframe the library does not move -- the fixed one, one without an edge --
 * receives its own pose again, to the bit (the reference hands it the same pose through a quaternion).
 * *pbStopFlag is read at the call: when it is set nothing is optimized and the map stays as it is (the reference's optimize()
 * returns at once and writes the unchanged estimates back; its caller drops a stopped result).  A stereo observation
 * (mvuRight >= 0) throws std::runtime_error: stereo is dead code in this fork.  Every library error throws std::runtime_error with
 * the library's message, which names the bound.
 */
#include "Optimizer.h"

#include <cstdint>
#include <map>
#include <stdexcept>
#include <vector>

#include "Frame.h"
#include "KeyFrame.h"
#include "MapAruco.h"
#include "MapPoint.h"
#include "Optimizer_globalba_orbfe.h"
#include "orbfe_shim.h"

namespace ORB_SLAM2
{

using namespace orbfe_shim;

namespace orbfe_globalba
{

void Collect(const std::vector<KeyFrame*>& vpKFs, const std::vector<MapPoint*>& vpMP, const std::vector<MapAruco*>& vpMA, Problem& pb)
{
    pb = Problem();
    std::map<KeyFrame*, int32_t> slot;
    for (KeyFrame* kf : vpKFs) {
        if (kf->isBad()) continue;
        slot[kf] = (int32_t)pb.vpKeyFrames.size();
        pb.vpKeyFrames.push_back(kf);
        pb.kf_fixed.push_back(kf->mnId == 0 ? 1 : 0);
        append_pose(kf->GetPose(), pb.Tcw);
    }
    if (!pb.vpKeyFrames.empty()) {
        KeyFrame* kf = pb.vpKeyFrames[0];   // one camera: every edge of the reference carries its own keyframe's, which are the same
        pb.K4[0] = kf->fx; pb.K4[1] = kf->fy; pb.K4[2] = kf->cx; pb.K4[3] = kf->cy;
        pb.inv_level_sigma2 = kf->mvInvLevelSigma2;
    }

    // an observer that is bad, or not among the collected keyframes, gives no edge
    const auto collected = [&slot](KeyFrame* kf) { return !kf->isBad() && slot.count(kf) != 0; };
    pb.obs_offset.push_back(0);
    for (MapPoint* mp : vpMP) {
        if (mp->isBad()) continue;
        pb.vpMapPoints.push_back(mp);
        orbfe_ba::AppendPoint(mp, slot, collected, "Optimizer::BundleAdjustment", pb);
    }

    pb.mobs_offset.push_back(0);
    if (!Frame::mbUArucoIni) return;
    for (MapAruco* ma : vpMA) {
        if (ma->isBad()) continue;
        pb.vpMapArucos.push_back(ma);
        orbfe_ba::AppendMarker(ma, slot, collected, pb);
    }
}

} // namespace orbfe_globalba

void Optimizer::BundleAdjustment(const std::vector<KeyFrame*>& vpKFs, const std::vector<MapPoint*>& vpMP, const std::vector<MapAruco*>& vpMA,
                                 int nIterations, bool* pbStopFlag, const unsigned long nLoopKF, const bool bRobust)
{
    orbfe_globalba::Problem pb;
    orbfe_globalba::Collect(vpKFs, vpMP, vpMA, pb);
    const int nkf = (int)pb.vpKeyFrames.size(), np = (int)pb.vpMapPoints.size(), nobs = (int)pb.obs_kf.size();
    const int nma = (int)pb.vpMapArucos.size(), nmobs = (int)pb.mobs_kf.size();
    if (nkf == 0) return;
    const uint8_t stop = pbStopFlag && *pbStopFlag ? 1 : 0;
    orbfe_gba_result res;
    check(orbfe_global_bundle_adjustment(pb.Tcw.data(), pb.kf_fixed.data(), nkf, pb.x3Dw.data(), np, pb.obs_offset.data(), pb.obs_kf.data(),
                                         pb.obs_xy.data(), pb.obs_octave.data(), nobs, pb.K4, pb.inv_level_sigma2.data(),
                                         (int)pb.inv_level_sigma2.size(), pb.Twm.data(), pb.marker_local.data(), nma, pb.mobs_offset.data(),
                                         pb.mobs_kf.data(), pb.mobs_corners.data(), nmobs, kMarkerInformation,
                                         Frame::mbUArucoIni ? 1 : 0, nIterations, bRobust ? 1 : 0, &stop, 0, &res, 0));
    if (res.status == ORBFE_GBA_STOPPED) return;   // nothing was optimized: the map stays as it is

    for (int k = 0; k < nkf; k++) {
        KeyFrame* kf = pb.vpKeyFrames[(size_t)k];
        if (kf->isBad()) continue;
        const cv::Mat pose = pose4x4(&pb.Tcw[12 * (size_t)k]);
        if (nLoopKF == 0) {
            kf->SetPose(pose);
        } else {
            kf->mTcwGBA.create(4, 4, CV_32F);
            pose.copyTo(kf->mTcwGBA);
            kf->mnBAGlobalForKF = nLoopKF;
        }
    }
    for (int i = 0; i < np; i++) {
        MapPoint* mp = pb.vpMapPoints[(size_t)i];
        if (pb.obs_offset[(size_t)i + 1] == pb.obs_offset[(size_t)i] || mp->isBad()) continue;   // no edge: no vertex
        const cv::Mat X = mat32(3, 1, &pb.x3Dw[3 * (size_t)i]);
        if (nLoopKF == 0) {
            mp->SetWorldPos(X);
            mp->UpdateNormalAndDepth();
        } else {
            mp->mPosGBA.create(3, 1, CV_32F);
            X.copyTo(mp->mPosGBA);
            mp->mnBAGlobalForKF = nLoopKF;
        }
    }
    if (Frame::mbUArucoIni)
        for (int m = 0; m < nma; m++) {
            MapAruco* ma = pb.vpMapArucos[(size_t)m];
            if (ma->isBad()) continue;
            const cv::Mat T = mat32(3, 4, &pb.Twm[12 * (size_t)m]);
            ma->SetRtwm(T.rowRange(0, 3).colRange(0, 3), T.rowRange(0, 3).colRange(3, 4));
        }
}

} // namespace ORB_SLAM2
