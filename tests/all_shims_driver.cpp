// TEST INFRASTRUCTURE ONLY -- every shim of include/shims/ in ONE program, as an integration links them: the two header shims and all
// class headers of tests/mock_orbslam/ in one translation unit, the eleven .cc shims linked in, ONE Optimizer, KeyFrame, MapPoint,
// MapAruco and Map declaration for the five Optimizer shims.  It references every shim and runs the members that stay on the host;
// nothing here opens a device.
//   all_shims_driver          prints one line, exit status 0
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
#include "Optimizer_localba_orbfe.h"
#include "Optimizer_globalba_orbfe.h"

using namespace ORB_SLAM2;

// the members that would need a device are referenced, not called: a volatile pointer keeps the reference in the program
static float (ORBextractor::*volatile g_extractor)() = &ORBextractor::GetScaleFactor;
static aruco::DetectionMode (aruco::MarkerDetector::*volatile g_detector)() = &aruco::MarkerDetector::getDetectionMode;
static orbfe_aruco* (aruco::MarkerDetector::*volatile g_detector_handle)() = &aruco::MarkerDetector::handle;
static int (ORBmatcher::*volatile g_matcher)(Frame&, Frame&, std::vector<cv::Point2f>&, std::vector<int>&, int) = &ORBmatcher::SearchForInitialization;
static int (ORBmatcher::*volatile g_matcher_tri)(KeyFrame*, KeyFrame*, cv::Mat, std::vector<std::pair<size_t, size_t> >&, const bool) =
    &ORBmatcher::SearchForTriangulation;
static bool (Initializer::*volatile g_initializer)(const Frame&, const std::vector<int>&, cv::Mat&, cv::Mat&, std::vector<cv::Point3f>&,
                                                   std::vector<bool>&) = &Initializer::Initialize;
static int (*volatile g_pose)(Frame*) = &Optimizer::PoseOptimization;
static int (*volatile g_pose_aruco)(Frame*) = &Optimizer::PoseOptimizationByAruco;
static int (*volatile g_sim3_opt)(KeyFrame*, KeyFrame*, std::vector<MapPoint*>&, g2o::Sim3&, const float, const bool) = &Optimizer::OptimizeSim3;
static std::vector<std::vector<NewMapPointGeometry> > (*volatile g_new_points)(KeyFrame*, const std::vector<KeyFrame*>&, const std::function<bool()>&) =
    &CreateNewMapPointsGeometry;
static void (*volatile g_essential)(Map*, KeyFrame*, KeyFrame*, const LoopClosing::KeyFrameAndPose&, const LoopClosing::KeyFrameAndPose&,
                                    const std::map<KeyFrame*, std::set<KeyFrame*> >&, const bool&) = &Optimizer::OptimizeEssentialGraph;
static void (*volatile g_local_ba)(KeyFrame*, bool*, Map*) = &Optimizer::LocalBundleAdjustment;
static void (*volatile g_global_ba)(const std::vector<KeyFrame*>&, const std::vector<MapPoint*>&, const std::vector<MapAruco*>&, int, bool*,
                                    const unsigned long, const bool) = &Optimizer::BundleAdjustment;

static double no_score(const DBoW2::BowVector&, const DBoW2::BowVector&) { return 0; }

int main()
{
    int referenced = 0;
    referenced += g_extractor != nullptr;
    referenced += g_detector != nullptr && g_detector_handle != nullptr;
    referenced += g_matcher != nullptr && g_matcher_tri != nullptr;
    referenced += g_initializer != nullptr;
    referenced += g_pose != nullptr && g_pose_aruco != nullptr;
    referenced += g_sim3_opt != nullptr;
    referenced += g_new_points != nullptr;
    referenced += g_essential != nullptr;
    referenced += g_local_ba != nullptr;
    referenced += g_global_ba != nullptr;

    // host-only members of the shims, on one Frame / KeyFrame / MapPoint / MapAruco / Map declaration
    Frame F;
    F.mK = cv::Mat(3, 3, CV_32F);
    KeyFrame KF1, KF2;
    const float identity[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
    KF1.SetPose(orbfe_shim::pose4x4(identity));   // Tcw for the bundle adjustments, Rcw and tcw for the others
    KF2.SetPose(orbfe_shim::pose4x4(identity));
    MapAruco marker;
    ORBmatcher matcher(0.6f, true);
    Initializer initializer(F, 1.0, 200);
    Sim3Solver solver(&KF1, &KF2, std::vector<MapPoint*>(), true);   // no matches: iterate() has nothing to ask the library
    bool bNoMore = false;
    std::vector<bool> vbInliers;
    int nInliers = -1;
    const cv::Mat T = solver.iterate(5, bNoMore, vbInliers, nInliers);
    ORBVocabulary voc(16, no_score);
    KeyFrameDatabase db(voc);
    db.add(&KF1);
    db.erase(&KF1);
    db.clear();
    const size_t candidates = db.DetectRelocalizationCandidates(&F).size();   // an empty database answers without the library
    // a keyframe without neighbours: the LocalMapping shim returns before it asks the library for anything
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
    // the collect steps of the two bundle adjustments on that map: KF2 with KF1 covisible, and both keyframes handed over; neither has
    // mnId 0, so both are free, and there are no points and no markers
    KF2.mvpOrderedConnectedKeyFrames.push_back(&KF1);
    const std::vector<uint8_t> both_free(2, 0);
    const std::vector<int32_t> offset0(1, 0);
    orbfe_localba::Problem lba;
    orbfe_localba::Collect(&KF2, &map, lba);
    const bool lba_collected = lba.kf_fixed == both_free && lba.obs_offset == offset0 && lba.mobs_offset == offset0;
    orbfe_globalba::Problem gba;
    orbfe_globalba::Collect(map.GetAllKeyFrames(), std::vector<MapPoint*>(), std::vector<MapAruco*>(), gba);
    const bool gba_collected = gba.kf_fixed == both_free && gba.obs_offset == offset0 && gba.mobs_offset == offset0;
    if (referenced != 10 || !T.empty() || !bNoMore || nInliers != 0 || candidates != 0 || marker.mLength != 0 || lists != 0 || !collected ||
        !lba_collected || !gba_collected)
        return 1;
    printf("ok: 11 shims in one program\n");
    return 0;
}
