// TEST INFRASTRUCTURE ONLY -- every shim of include/shims/ that shares the one mock tree, in ONE program: what
// tests/all_shims8_driver.cpp links plus Optimizer_essential_orbfe.cc, against the mock headers of tests/mock_orbslam_eg/ ahead of
// tests/mock_orbslam/.  It references every shim and runs the members that stay on the host; nothing here opens a device.
//   all_shims9_driver          prints one line, exit status 0
#include <cstdio>
#include <vector>

#include "ORBextractor.h"
#include "MarkerDetector.h"
#include "Frame.h"
#include "KeyFrame.h"
#include "MapPoint.h"
#include "MapAruco.h"
#include "ORBmatcher.h"
#include "Initializer.h"
#include "Sim3Solver.h"
#include "Optimizer.h"
#include "KeyFrameDatabase.h"
#include "ORBVocabulary.h"
#include "LocalMapping_orbfe.h"
#include "Optimizer_essential_orbfe.h"

using namespace ORB_SLAM2;

// the members that would need a device are referenced, not called: a volatile pointer keeps the reference in the program
static float (ORBextractor::*volatile g_extractor)() = &ORBextractor::GetScaleFactor;
static aruco::DetectionMode (aruco::MarkerDetector::*volatile g_detector)() = &aruco::MarkerDetector::getDetectionMode;
static int (ORBmatcher::*volatile g_matcher)(KeyFrame*, KeyFrame*, cv::Mat, std::vector<std::pair<size_t, size_t> >&, const bool) =
    &ORBmatcher::SearchForTriangulation;
static bool (Initializer::*volatile g_initializer)(const Frame&, const std::vector<int>&, cv::Mat&, cv::Mat&, std::vector<cv::Point3f>&,
                                                   std::vector<bool>&) = &Initializer::Initialize;
static int (*volatile g_pose)(Frame*) = &Optimizer::PoseOptimization;
static int (*volatile g_sim3_opt)(KeyFrame*, KeyFrame*, std::vector<MapPoint*>&, g2o::Sim3&, const float, const bool) = &Optimizer::OptimizeSim3;
static std::vector<std::vector<NewMapPointGeometry> > (*volatile g_new_points)(KeyFrame*, const std::vector<KeyFrame*>&, const std::function<bool()>&) =
    &CreateNewMapPointsGeometry;
static void (*volatile g_essential)(Map*, KeyFrame*, KeyFrame*, const LoopClosing::KeyFrameAndPose&, const LoopClosing::KeyFrameAndPose&,
                                    const std::map<KeyFrame*, std::set<KeyFrame*> >&, const bool&) = &Optimizer::OptimizeEssentialGraph;

static double no_score(const DBoW2::BowVector&, const DBoW2::BowVector&) { return 0; }

int main()
{
    int referenced = 0;
    referenced += g_extractor != nullptr;
    referenced += g_detector != nullptr;
    referenced += g_matcher != nullptr;
    referenced += g_initializer != nullptr;
    referenced += g_pose != nullptr;
    referenced += g_sim3_opt != nullptr;
    referenced += g_new_points != nullptr;
    referenced += g_essential != nullptr;

    KeyFrame KF1, KF2;
    KF1.Rcw = KF2.Rcw = cv::Mat(3, 3, CV_32F);
    KF1.tcw = KF2.tcw = cv::Mat(3, 1, CV_32F);
    Sim3Solver solver(&KF1, &KF2, std::vector<MapPoint*>(), true);   // no matches: iterate() has nothing to ask the library
    bool bNoMore = false;
    std::vector<bool> vbInliers;
    int nInliers = -1;
    const cv::Mat T = solver.iterate(5, bNoMore, vbInliers, nInliers);
    ORBVocabulary voc(16, no_score);
    KeyFrameDatabase db(voc);
    Frame F;
    const size_t candidates = db.DetectRelocalizationCandidates(&F).size();   // an empty database answers without the library
    const size_t lists = CreateNewMapPointsGeometry(&KF1, KF1.GetBestCovisibilityKeyFrames(20)).size();
    // the collect step of the essential graph on a map of two keyframes: one spanning-tree edge, the loop keyframe fixed
    Map map;
    KF1.mnId = 1; KF2.mnId = 2;
    KF2.mpParent = &KF1;
    map.mvpKeyFrames.push_back(&KF1);
    map.mvpKeyFrames.push_back(&KF2);
    orbfe_essential::Problem pb;
    orbfe_essential::Collect(&map, &KF1, &KF2, LoopClosing::KeyFrameAndPose(), LoopClosing::KeyFrameAndPose(), std::map<KeyFrame*, std::set<KeyFrame*> >(), pb);
    const bool collected = pb.fixed == 0 && pb.edge_i.size() == 1 && pb.edge_i[0] == 1 && pb.edge_j[0] == 0 && pb.edge_kind[0] == 1;
    if (referenced != 8 || !T.empty() || !bNoMore || nInliers != 0 || candidates != 0 || lists != 0 || !collected) return 1;
    printf("ok: 9 shims in one program\n");
    return 0;
}
