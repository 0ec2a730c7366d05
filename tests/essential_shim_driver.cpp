// TEST INFRASTRUCTURE ONLY -- drives include/shims/Optimizer_essential_orbfe.cc the way LoopClosing::CorrectLoopByAruco does, on a
// hand-built mock map (the mock headers of tests/mock_orbslam/), and dumps raw arrays for
// tests/test_essential_shim_cpu.py and tests/test_essential_shim_gpu.py.
//   essential_shim_driver collect <out prefix>   the collect step alone (no library call): the flat arrays
//   essential_shim_driver run <out prefix>       the flat arrays, then Optimizer::OptimizeEssentialGraph (bFixScale = true) and the map
// The map: keyframes k = 0 .. 7 with mnId 10 + 2 k, keyframe 5 bad; the loop keyframe is 1, the current one 7.  Parents: k - 1, but 4
// for 5 and 6.  Weights: 300 along the spanning tree, 120 two apart, (7, 1) = 30, (7, 2) = 50, (6, 2) = 150, (7, 5) = 200.  Keyframes 4
// and 0 share an old loop edge.  LoopConnections: 7 -> {1, 2}, 6 -> {2}.  CorrectedSim3 and NonCorrectedSim3 hold 6 and 7.
//   - (7, 1) has weight 30 and survives as the cur / loop pair alone; (7, 2) with 50 does not
//   - (6, 2) is a loop connection and covisible: kept once, as the loop connection
//   - (4, 0) is the old loop edge, from the larger id
//   - 6 is in CorrectedSim3 and is not the fixed one
//   - keyframe 5 is no vertex; 7 sees it with weight 200 and gets no edge to it; point 11, whose reference it is, stays where it is
//   - point 7 has mnCorrectedByKF == pCurKF->mnId and goes through keyframe 6, not through its reference keyframe 3
//   - point 8 is a marker point (id 9) whose keyframe 2 lacks the id: its SetWorldPos is skipped; points 9 and 10 are marker points
//     (id 4) of keyframe 3, which holds it: the marker is updated once
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "Optimizer.h"
#include "Optimizer_essential_orbfe.h"
#include "shim_driver_io.hpp"

using namespace ORB_SLAM2;

static void link(KeyFrame& a, KeyFrame& b, int w)
{
    a.mConnectedKeyFrameWeights[&b] = w;
    b.mConnectedKeyFrameWeights[&a] = w;
}

int main(int argc, char** argv)
{
    if (argc != 3) return 2;
    const std::string mode = argv[1], out = argv[2];
    const int NK = 8, NP = 12;
    std::vector<KeyFrame> kfs((size_t)NK);
    std::vector<MapPoint> mps((size_t)NP);
    MapAruco marker;
    Map map;
    for (int k = 0; k < NK; k++) {
        KeyFrame& F = kfs[(size_t)k];
        F.mnId = (long unsigned)(10 + 2 * k);
        F.mbBad = k == 5;
        const float a = 0.05f * (float)k, c = std::cos(a), s = std::sin(a);
        cv::Mat T(4, 4, CV_32F);
        const float v[16] = {c, 0, s, -0.5f * (float)k, 0, 1, 0, 0.01f * (float)k, -s, 0, c, 0.02f * (float)(k * k), 0, 0, 0, 1};
        for (int i = 0; i < 16; i++) T.at<float>(i / 4, i % 4) = v[i];
        F.SetPose(T);
        F.nSetPose = 0;
        map.mvpKeyFrames.push_back(&F);
    }
    const int parent[8] = {-1, 0, 1, 2, 3, 4, 4, 6};
    for (int k = 2; k < NK; k++) link(kfs[(size_t)k], kfs[(size_t)k - 2], 120);
    for (int k = 1; k < NK; k++) {
        kfs[(size_t)k].mpParent = &kfs[(size_t)parent[k]];
        kfs[(size_t)parent[k]].mspChildrens.insert(&kfs[(size_t)k]);
        link(kfs[(size_t)k], kfs[(size_t)parent[k]], 300);
    }
    link(kfs[7], kfs[1], 30); link(kfs[7], kfs[2], 50); link(kfs[6], kfs[2], 150); link(kfs[7], kfs[5], 200);
    for (KeyFrame& F : kfs) {   // by weight, best first; ties by mnId
        for (int w : {300, 200, 150, 120, 50, 30})
            for (KeyFrame& G : kfs)
                if (F.mConnectedKeyFrameWeights.count(&G) && F.mConnectedKeyFrameWeights[&G] == w) F.mvpOrderedConnectedKeyFrames.push_back(&G);
    }
    kfs[4].mspLoopEdges.insert(&kfs[0]);
    kfs[0].mspLoopEdges.insert(&kfs[4]);
    KeyFrame *pLoopKF = &kfs[1], *pCurKF = &kfs[7];
    std::map<KeyFrame*, std::set<KeyFrame*> > LoopConnections;
    LoopConnections[pCurKF].insert(pLoopKF);
    LoopConnections[pCurKF].insert(&kfs[2]);
    LoopConnections[&kfs[6]].insert(&kfs[2]);
    LoopClosing::KeyFrameAndPose Corrected, NonCorrected;
    for (int k = 6; k < NK; k++) {
        KeyFrame& F = kfs[(size_t)k];
        Eigen::Matrix3d R;
        Eigen::Vector3d t, tc;
        for (int r = 0; r < 3; r++) {
            for (int c = 0; c < 3; c++) R(r, c) = F.Rcw.at<float>(r, c);
            t[r] = F.tcw.at<float>(r);
        }
        tc = t;
        tc[0] += 0.05 * (k - 5); tc[1] += 0.02; tc[2] -= 0.03 * (k - 5);
        NonCorrected[&F] = g2o::Sim3(R, t, 1.0);
        Corrected[&F] = g2o::Sim3(R, tc, 1.0);
    }
    marker.mTwm = cv::Mat(4, 4, CV_32F);
    kfs[3].mmArucoIdandIdx[4] = 0;
    kfs[3].mvpMapArucos.push_back(&marker);
    const int ref[12] = {0, 2, 3, 4, 6, 7, 1, 3, 2, 3, 3, 5};
    for (int i = 0; i < NP; i++) {
        MapPoint& P = mps[(size_t)i];
        P.mWorldPos = cv::Mat(3, 1, CV_32F);
        P.mWorldPos.at<float>(0) = 0.3f * (float)i - 1.f; P.mWorldPos.at<float>(1) = 0.1f * (float)(i % 3); P.mWorldPos.at<float>(2) = 2.f + 0.2f * (float)i;
        P.mpRefKF = &kfs[(size_t)ref[i]];
        map.mvpMapPoints.push_back(&P);
    }
    mps[6].mbBad = true;
    mps[7].mnCorrectedByKF = pCurKF->mnId;
    mps[7].mnCorrectedReference = kfs[6].mnId;
    mps[8].forflag = true; mps[8].mArucoID = 9;
    mps[9].forflag = true; mps[9].mArucoID = 4;
    mps[10].forflag = true; mps[10].mArucoID = 4;

    orbfe_essential::Problem pb;
    orbfe_essential::Collect(&map, pLoopKF, pCurKF, NonCorrected, Corrected, LoopConnections, pb);
    std::vector<int32_t> vk, fixed(1, pb.fixed);
    for (KeyFrame* p : pb.vpKeyFrames) vk.push_back((int32_t)(p - kfs.data()));
    dump(out + "_vk.bin", vk); dump(out + "_id.bin", pb.kf_id); dump(out + "_fixed.bin", fixed); dump(out + "_cpos.bin", pb.corrected_pos);
    dump(out + "_npos.bin", pb.noncorrected_pos); dump(out + "_ei.bin", pb.edge_i); dump(out + "_ej.bin", pb.edge_j); dump(out + "_ek.bin", pb.edge_kind);
    dump(out + "_pref.bin", pb.point_ref); dump(out + "_Tcw.bin", pb.Tcw); dump(out + "_x.bin", pb.x3Dw); dump(out + "_csim.bin", pb.corrected);
    dump(out + "_nsim.bin", pb.noncorrected);
    int32_t threw = 0;
    kfs[1].mbBad = true;   // a bad loop keyframe throws
    try {
        orbfe_essential::Problem other;
        orbfe_essential::Collect(&map, pLoopKF, pCurKF, NonCorrected, Corrected, LoopConnections, other);
    } catch (const std::runtime_error&) {
        threw = 1;
    }
    kfs[1].mbBad = false;
    dump(out + "_threw.bin", &threw, 1);
    if (mode == "collect") return 0;
    if (mode != "run") return 2;

    const bool bFixScale = true;
    Optimizer::OptimizeEssentialGraph(&map, pLoopKF, pCurKF, NonCorrected, Corrected, LoopConnections, bFixScale);
    std::vector<float> T, P, M;
    std::vector<int32_t> counts;
    for (KeyFrame& F : kfs) {
        for (int r = 0; r < 3; r++) {
            for (int c = 0; c < 3; c++) T.push_back(F.Rcw.at<float>(r, c));
            T.push_back(F.tcw.at<float>(r));
        }
        counts.push_back(F.nSetPose);
    }
    for (MapPoint& p : mps) {
        for (int c = 0; c < 3; c++) P.push_back(p.mWorldPos.at<float>(c));
        counts.push_back(p.nSetWorldPos);
        counts.push_back(p.nUpdates);
    }
    counts.push_back(marker.nUpdateTcm); counts.push_back(marker.nSetRtwm); counts.push_back((int32_t)marker.nLastIdx);
    counts.push_back(marker.pLastKF ? (int32_t)(marker.pLastKF - kfs.data()) : -1);
    if (marker.nSetRtwm) {
        for (int i = 0; i < 9; i++) M.push_back(marker.mLastRwc.at<float>(i / 3, i % 3));
        for (int i = 0; i < 3; i++) M.push_back(marker.mLastTwc.at<float>(i));
    }
    dump(out + "_T.bin", T); dump(out + "_P.bin", P); dump(out + "_M.bin", M); dump(out + "_counts.bin", counts);
    return 0;
}
