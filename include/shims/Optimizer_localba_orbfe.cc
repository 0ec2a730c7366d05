/*
 * Optimizer_localba_orbfe.cc (shim) -- Optimizer::LocalBundleAdjustment(KeyFrame*, bool*, Map*) (src/Optimizer.cc:772-1242)
 * implemented on liborbfe.so.  Link it together with src/Optimizer.cc from which that definition has been removed.
 * include/Optimizer.h, KeyFrame, MapPoint, MapAruco and Map stay the reference's own.
 *
 * Collect (host) builds what the reference's lines 777-888 build, with the same side effects on the map: the vertex keyframes
 * (the current keyframe and its covisible ones, marked mnBALocalForKF; then every other observer of their map points, marked
 * mnBAFixedForKF), the map points those local keyframes hold, and the map markers the vertex keyframes see (entries that are not
 * old, markers that are not bad, one vertex an id).  The flat arrays follow in the order g2o would have received the vertices and
 * edges, and ONE orbfe_local_bundle_adjustment call.
 * Apply (under Map::mMutexMapUpdate): the erased observations in edge order (EraseMapPointMatch, EraseObservation; a point that
 * went bad meanwhile is passed over, as the reference's second check does -- its first check's skip cannot be reproduced, the
 * library sees no bad flags), SetPose of the local keyframes, SetWorldPos + UpdateNormalAndDepth of the points, SetRtwm of the
 * markers when Frame::mbUArucoIni.  The keyframe with mnId 0 is fixed: it receives its own pose again, to the bit (the reference
 * hands it the same pose through a quaternion).  *pbStopFlag is read at the call; a flag set while the call runs is seen by the
 * next one.  A stereo observation (mvuRight >= 0) throws std::runtime_error: stereo is dead code in this fork.  More free pose
 * vertices than ORBFE_LBA_MAX_FREE_POSES, like every library error, throws std::runtime_error with the library's message, which
 * names the bound.
 */
#include "Optimizer.h"

#include <algorithm>
#include <cstdint>
#include <map>
#include <mutex>
#include <stdexcept>
#include <vector>

#include "Frame.h"
#include "KeyFrame.h"
#include "Map.h"
#include "MapAruco.h"
#include "MapPoint.h"
#include "Optimizer_localba_orbfe.h"
#include "orbfe_shim.h"

namespace ORB_SLAM2
{

using namespace orbfe_shim;

namespace orbfe_localba
{

namespace
{

// The vertex keyframes while they are being gathered.  A keyframe is marked the first time it is met -- as a local one or as a
// fixed one, with the current keyframe's id in the member the reference uses -- and becomes a vertex unless it is bad; a bad one
// keeps its mark, so that it is not looked at again.
struct Vertices {
    const long unsigned int tag;
    Problem& pb;
    std::map<KeyFrame*, int32_t> slot;
    std::vector<long unsigned int> ids;   // mnId of every vertex: a marker observation from any other keyframe is dropped

    Vertices(long unsigned int t, Problem& p) : tag(t), pb(p) {}
    static bool marked(KeyFrame* kf, long unsigned int t) { return kf->mnBALocalForKF == t || kf->mnBAFixedForKF == t; }
    void meet(KeyFrame* kf, bool local)
    {
        (local ? kf->mnBALocalForKF : kf->mnBAFixedForKF) = tag;
        if (kf->isBad()) return;
        slot[kf] = (int32_t)pb.vpKeyFrames.size();
        pb.vpKeyFrames.push_back(kf);
        pb.kf_fixed.push_back(!local || kf->mnId == 0 ? 1 : 0);
        ids.push_back(kf->mnId);
    }
    bool has_id(long unsigned int id) const { return std::find(ids.begin(), ids.end(), id) != ids.end(); }
};

} // namespace

void Collect(KeyFrame* pKF, Map* /*pMap*/, Problem& pb)
{
    pb = Problem();
    const long unsigned int tag = pKF->mnId;
    Vertices V(tag, pb);

    // local keyframes: the current one, then its covisible ones, best first
    V.meet(pKF, true);
    for (KeyFrame* kf : pKF->GetVectorCovisibleKeyFrames()) V.meet(kf, true);
    pb.nLocal = pb.vpKeyFrames.size();

    // their map points, each once, in the order the keyframes hold them
    for (size_t k = 0; k < pb.nLocal; k++)
        for (MapPoint* mp : pb.vpKeyFrames[k]->GetMapPointMatches()) {
            if (!mp || mp->isBad() || mp->mnBALocalForKF == tag) continue;
            mp->mnBALocalForKF = tag;
            pb.vpMapPoints.push_back(mp);
        }

    // fixed cameras: whoever else observes one of those points, in the order the points' observation maps give
    for (MapPoint* mp : pb.vpMapPoints) {
        const std::map<KeyFrame*, size_t> seen = mp->GetObservations();
        for (const auto& o : seen)
            if (!Vertices::marked(o.first, tag)) V.meet(o.first, false);
    }

    // the markers of the vertex keyframes, local ones first: one vertex an id
    std::vector<int> marker_ids;
    for (KeyFrame* kf : pb.vpKeyFrames)
        for (size_t i = 0; i < (size_t)kf->NA; i++) {
            if (kf->isIdxArucoOld(i)) continue;
            MapAruco* ma = kf->GetMapAruco(i);
            if (!ma || ma->isBad()) continue;
            const int id = ma->GetMapArucoID();
            if (std::find(marker_ids.begin(), marker_ids.end(), id) != marker_ids.end()) continue;
            marker_ids.push_back(id);
            pb.vpMapArucos.push_back(ma);
        }

    // ---- the flat arrays
    for (KeyFrame* kf : pb.vpKeyFrames) append_pose(kf->GetPose(), pb.Tcw);
    pb.K4[0] = pKF->fx; pb.K4[1] = pKF->fy; pb.K4[2] = pKF->cx; pb.K4[3] = pKF->cy;
    pb.inv_level_sigma2 = pKF->mvInvLevelSigma2;

    pb.obs_offset.push_back(0);
    for (MapPoint* mp : pb.vpMapPoints) {
        // a bad observer is marked, but no vertex
        orbfe_ba::AppendPoint(mp, V.slot, [](KeyFrame* kf) { return !kf->isBad(); }, "Optimizer::LocalBundleAdjustment", pb);
        for (size_t e = pb.vpEdgeKF.size(); e < pb.obs_kf.size(); e++) {
            pb.vpEdgeKF.push_back(pb.vpKeyFrames[(size_t)pb.obs_kf[e]]);
            pb.vpEdgeMP.push_back(mp);
        }
    }

    pb.mobs_offset.push_back(0);
    for (MapAruco* ma : pb.vpMapArucos)
        orbfe_ba::AppendMarker(ma, V.slot, [&V](KeyFrame* kf) { return !kf->isBad() && V.has_id(kf->mnId); }, pb);
}

} // namespace orbfe_localba

void Optimizer::LocalBundleAdjustment(KeyFrame* pKF, bool* pbStopFlag, Map* pMap)
{
    orbfe_localba::Problem pb;
    orbfe_localba::Collect(pKF, pMap, pb);
    const int nkf = (int)pb.vpKeyFrames.size(), np = (int)pb.vpMapPoints.size(), nobs = (int)pb.obs_kf.size();
    const int nma = (int)pb.vpMapArucos.size(), nmobs = (int)pb.mobs_kf.size();
    std::vector<uint8_t> erase((size_t)nobs, 0);
    const uint8_t stop = pbStopFlag && *pbStopFlag ? 1 : 0;
    orbfe_lba_result res;
    check(orbfe_local_bundle_adjustment(pb.Tcw.data(), pb.kf_fixed.data(), nkf, pb.x3Dw.data(), np, pb.obs_offset.data(), pb.obs_kf.data(),
                                        pb.obs_xy.data(), pb.obs_octave.data(), nobs, pb.K4, pb.inv_level_sigma2.data(),
                                        (int)pb.inv_level_sigma2.size(), pb.Twm.data(), pb.marker_local.data(), nma, pb.mobs_offset.data(),
                                        pb.mobs_kf.data(), pb.mobs_corners.data(), nmobs, kMarkerInformation,
                                        Frame::mbUArucoIni ? 1 : 0, &stop, erase.data(), &res, 0));
    if (res.status == ORBFE_LBA_STOPPED) return;   // nothing was optimized: the map stays as it is

    std::unique_lock<std::mutex> lock(pMap->mMutexMapUpdate);
    for (int e = 0; e < nobs; e++) {
        MapPoint* mp = pb.vpEdgeMP[(size_t)e];
        if (!erase[(size_t)e] || mp->isBad()) continue;
        pb.vpEdgeKF[(size_t)e]->EraseMapPointMatch(mp);
        mp->EraseObservation(pb.vpEdgeKF[(size_t)e]);
    }
    for (size_t k = 0; k < pb.nLocal; k++) pb.vpKeyFrames[k]->SetPose(pose4x4(&pb.Tcw[12 * k]));
    for (int i = 0; i < np; i++) {
        pb.vpMapPoints[(size_t)i]->SetWorldPos(mat32(3, 1, &pb.x3Dw[3 * (size_t)i]));
        pb.vpMapPoints[(size_t)i]->UpdateNormalAndDepth();
    }
    if (Frame::mbUArucoIni)
        for (int m = 0; m < nma; m++) {
            const cv::Mat T = mat32(3, 4, &pb.Twm[12 * (size_t)m]);
            pb.vpMapArucos[(size_t)m]->SetRtwm(T.rowRange(0, 3).colRange(0, 3), T.rowRange(0, 3).colRange(3, 4));
        }
}

} // namespace ORB_SLAM2
