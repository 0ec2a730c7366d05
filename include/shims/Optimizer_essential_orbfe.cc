/*
 * Optimizer_essential_orbfe.cc (shim) -- Optimizer::OptimizeEssentialGraph(Map*, KeyFrame*, KeyFrame*, const KeyFrameAndPose&,
 * const KeyFrameAndPose&, const map<KeyFrame*, set<KeyFrame*> >&, const bool&) (src/Optimizer.cc:1245-1542) implemented on
 * liborbfe.so.  Link it together with src/Optimizer.cc from which that definition has been removed.
 * include/Optimizer.h, LoopClosing.h, KeyFrame, MapPoint, MapAruco and Map stay the reference's own.
 *
 * Collect (host): the vertices are GetAllKeyFrames() without the bad ones, in its order.  The edge rules are the reference's code
 * paths, producing the flat list in insertion order: the LoopConnections (minFeat = 100 unless the pair is pCurKF / pLoopKF; the pair
 * goes into sInsertedEdges), then per keyframe its parent, its loop edges with the smaller id, and its GetCovisiblesByWeight(100)
 * minus parent, children, loop edges, bad ones, larger ids and pairs of sInsertedEdges.  The first group measures with vScw (kind 0),
 * the rest with NonCorrectedSim3 where a keyframe has an entry (kind 1).  A map point's reference is mnCorrectedReference when
 * mnCorrectedByKF is pCurKF's id, else its reference keyframe's id.
 * Apply (under Map::mMutexMapUpdate): SetPose of every vertex; then per map point that is not bad the fork's marker block
 * (lines 1507-1535: UpdateTcmByKF, SetRtwmByKeyFrame, sModified) WITH its early `continue`, which skips the SetWorldPos of a marker
 * point whose keyframe does not hold the marker's id -- the reference's behaviour, kept; SetWorldPos; UpdateNormalAndDepth.
 *
 * What differs.  Bad keyframes are not vertices, and an edge or a point that names one is dropped (the point keeps its position but is
 * still set and updated): the reference adds no vertex for a bad keyframe either and then dereferences a null vertex for the edge.
 * pbStopFlag does not exist for this function.  Library errors throw std::runtime_error with the library's message.
 */
#include "Optimizer.h"

#include <algorithm>
#include <cstdint>
#include <map>
#include <mutex>
#include <set>
#include <stdexcept>
#include <utility>
#include <vector>

#include "KeyFrame.h"
#include "LoopClosing.h"
#include "Map.h"
#include "MapAruco.h"
#include "MapPoint.h"
#include "Optimizer_essential_orbfe.h"
#include "orbfe_shim.h"

namespace ORB_SLAM2
{

using namespace orbfe_shim;

namespace orbfe_essential
{

namespace
{

void append_sim(const g2o::Sim3& S, std::vector<double>& out)
{
    out.push_back(S.rotation().x()); out.push_back(S.rotation().y()); out.push_back(S.rotation().z()); out.push_back(S.rotation().w());
    for (int i = 0; i < 3; i++) out.push_back(S.translation()[i]);
    out.push_back(S.scale());
}

} // namespace

void Collect(Map* pMap, KeyFrame* pLoopKF, KeyFrame* pCurKF, const LoopClosing::KeyFrameAndPose& NonCorrectedSim3,
             const LoopClosing::KeyFrameAndPose& CorrectedSim3, const std::map<KeyFrame*, std::set<KeyFrame*> >& LoopConnections, Problem& pb)
{
    pb = Problem();
    const std::vector<KeyFrame*> vpKFs = pMap->GetAllKeyFrames();
    std::map<KeyFrame*, int32_t> slot;
    std::map<long unsigned int, int32_t> slot_of_id;
    for (KeyFrame* pKF : vpKFs) {
        if (pKF->isBad()) continue;
        const int32_t at = (int32_t)pb.vpKeyFrames.size();
        slot[pKF] = at;
        slot_of_id[pKF->mnId] = at;
        pb.vpKeyFrames.push_back(pKF);
        pb.kf_id.push_back((int32_t)pKF->mnId);
        float T[12];
        pose34(pKF->GetRotation(), pKF->GetTranslation(), T);
        pb.Tcw.insert(pb.Tcw.end(), T, T + 12);
        LoopClosing::KeyFrameAndPose::const_iterator it = CorrectedSim3.find(pKF);
        if (it != CorrectedSim3.end()) {
            pb.corrected_pos.push_back(at);
            append_sim(it->second, pb.corrected);
        }
        it = NonCorrectedSim3.find(pKF);
        if (it != NonCorrectedSim3.end()) {
            pb.noncorrected_pos.push_back(at);
            append_sim(it->second, pb.noncorrected);
        }
    }
    if (!slot.count(pLoopKF)) throw std::runtime_error("Optimizer::OptimizeEssentialGraph: the loop keyframe is bad or not in the map");
    pb.fixed = slot[pLoopKF];
    auto add = [&](KeyFrame* a, KeyFrame* b, int kind) {
        if (!slot.count(a) || !slot.count(b)) return;   // a bad keyframe is no vertex
        pb.edge_i.push_back(slot[a]);
        pb.edge_j.push_back(slot[b]);
        pb.edge_kind.push_back(kind);
    };

    const int minFeat = 100;
    std::set<std::pair<long unsigned int, long unsigned int> > sInsertedEdges;

    // Set Loop edges
    for (std::map<KeyFrame*, std::set<KeyFrame*> >::const_iterator mit = LoopConnections.begin(), mend = LoopConnections.end(); mit != mend; mit++) {
        KeyFrame* pKF = mit->first;
        const long unsigned int nIDi = pKF->mnId;
        const std::set<KeyFrame*>& spConnections = mit->second;
        for (std::set<KeyFrame*>::const_iterator sit = spConnections.begin(), send = spConnections.end(); sit != send; sit++) {
            const long unsigned int nIDj = (*sit)->mnId;
            if ((nIDi != pCurKF->mnId || nIDj != pLoopKF->mnId) && pKF->GetWeight(*sit) < minFeat) continue;
            add(pKF, *sit, 0);
            sInsertedEdges.insert(std::make_pair(std::min(nIDi, nIDj), std::max(nIDi, nIDj)));
        }
    }

    // Set normal edges
    for (size_t i = 0, iend = vpKFs.size(); i < iend; i++) {
        KeyFrame* pKF = vpKFs[i];
        if (pKF->isBad()) continue;
        KeyFrame* pParentKF = pKF->GetParent();
        // Spanning tree edge
        if (pParentKF) add(pKF, pParentKF, 1);
        // Loop edges
        const std::set<KeyFrame*> sLoopEdges = pKF->GetLoopEdges();
        for (std::set<KeyFrame*>::const_iterator sit = sLoopEdges.begin(), send = sLoopEdges.end(); sit != send; sit++) {
            KeyFrame* pLKF = *sit;
            if (pLKF->mnId < pKF->mnId) add(pKF, pLKF, 1);
        }
        // Covisibility graph edges
        const std::vector<KeyFrame*> vpConnectedKFs = pKF->GetCovisiblesByWeight(minFeat);
        for (std::vector<KeyFrame*>::const_iterator vit = vpConnectedKFs.begin(); vit != vpConnectedKFs.end(); vit++) {
            KeyFrame* pKFn = *vit;
            if (pKFn && pKFn != pParentKF && !pKF->hasChild(pKFn) && !sLoopEdges.count(pKFn)) {
                if (!pKFn->isBad() && pKFn->mnId < pKF->mnId) {
                    if (sInsertedEdges.count(std::make_pair(std::min(pKF->mnId, pKFn->mnId), std::max(pKF->mnId, pKFn->mnId)))) continue;
                    add(pKF, pKFn, 1);
                }
            }
        }
    }

    // the points and the keyframe each one is corrected through
    pb.vpMapPoints = pMap->GetAllMapPoints();
    for (MapPoint* pMP : pb.vpMapPoints) {
        float X[3];
        point3(pMP->GetWorldPos(), X);
        pb.x3Dw.insert(pb.x3Dw.end(), X, X + 3);
        int32_t ref = -1;
        if (!pMP->isBad()) {
            long unsigned int nIDr;
            if (pMP->mnCorrectedByKF == pCurKF->mnId) nIDr = pMP->mnCorrectedReference;
            else nIDr = pMP->GetReferenceKeyFrame()->mnId;
            std::map<long unsigned int, int32_t>::const_iterator it = slot_of_id.find(nIDr);
            if (it != slot_of_id.end()) ref = it->second;
        }
        pb.point_ref.push_back(ref);
    }
}

} // namespace orbfe_essential

void Optimizer::OptimizeEssentialGraph(Map* pMap, KeyFrame* pLoopKF, KeyFrame* pCurKF, const LoopClosing::KeyFrameAndPose& NonCorrectedSim3,
                                       const LoopClosing::KeyFrameAndPose& CorrectedSim3,
                                       const std::map<KeyFrame*, std::set<KeyFrame*> >& LoopConnections, const bool& bFixScale)
{
    orbfe_essential::Problem pb;
    orbfe_essential::Collect(pMap, pLoopKF, pCurKF, NonCorrectedSim3, CorrectedSim3, LoopConnections, pb);
    const int nkf = (int)pb.vpKeyFrames.size(), np = (int)pb.vpMapPoints.size();
    std::vector<float> Tout((size_t)nkf * 12), Xout((size_t)np * 3 + 3);
    orbfe_eg_result res;
    check(orbfe_optimize_essential_graph(pb.kf_id.data(), pb.Tcw.data(), nkf, pb.fixed, pb.corrected_pos.data(), pb.corrected.data(),
                                         (int)pb.corrected_pos.size(), pb.noncorrected_pos.data(), pb.noncorrected.data(),
                                         (int)pb.noncorrected_pos.size(), pb.edge_i.data(), pb.edge_j.data(), pb.edge_kind.data(), (int)pb.edge_i.size(),
                                         pb.x3Dw.data(), pb.point_ref.data(), np, 20, bFixScale ? 1 : 0, 0, Tout.data(), Xout.data(), nullptr, &res, 0));

    std::unique_lock<std::mutex> lock(pMap->mMutexMapUpdate);

    // SE3 Pose Recovering. Sim3:[sR t;0 1] -> SE3:[R t/s;0 1]
    for (int k = 0; k < nkf; k++) {
        cv::Mat Tiw(4, 4, CV_32F);
        for (int i = 0; i < 16; i++) Tiw.at<float>(i / 4, i % 4) = i < 12 ? Tout[12 * (size_t)k + (size_t)i] : (i == 15 ? 1.f : 0.f);
        pb.vpKeyFrames[(size_t)k]->SetPose(Tiw);
    }

    // Correct points
    std::set<int> sModified;
    for (int i = 0; i < np; i++) {
        MapPoint* pMP = pb.vpMapPoints[(size_t)i];
        if (pMP->isBad()) continue;
        if (pMP->forflag) {
            const int ArucoId = pMP->mArucoID;
            if (sModified.find(ArucoId) == sModified.end()) {
                KeyFrame* pTmp = pMP->mnCorrectedByKF == pCurKF->mnId ? pCurKF : pMP->GetReferenceKeyFrame();
                if (!pTmp->isBad()) {
                    if (!pTmp->mmArucoIdandIdx.count(ArucoId)) continue;
                    const int idx = pTmp->mmArucoIdandIdx[ArucoId];
                    MapAruco* pMA = pTmp->GetMapAruco((size_t)idx);
                    if (pMA && !pMA->isBad()) {
                        pMA->UpdateTcmByKF(pTmp, (size_t)idx);
                        pMA->SetRtwmByKeyFrame(pTmp->GetRotation().t(), pTmp->GetCameraCenter());
                    }
                    sModified.insert(ArucoId);
                }
            }
        }
        pMP->SetWorldPos(mat32(3, 1, &Xout[3 * (size_t)i]));
        pMP->UpdateNormalAndDepth();
    }
}

} // namespace ORB_SLAM2
