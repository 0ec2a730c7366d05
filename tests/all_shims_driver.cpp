// TEST INFRASTRUCTURE ONLY -- every shim of include/shims/ in ONE program, as an integration links them: the two header shims and all
// class headers of tests/mock_orbslam/ in one translation unit, the five .cc shims linked in, one Optimizer class for both Optimizer
// shims.  It references every shim class and runs the members that stay on the host; nothing here opens a device.
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

using namespace ORB_SLAM2;

// the members that would need a device are referenced, not called: a volatile pointer keeps the reference in the program
static float (ORBextractor::*volatile g_extractor)() = &ORBextractor::GetScaleFactor;
static aruco::DetectionMode (aruco::MarkerDetector::*volatile g_detector)() = &aruco::MarkerDetector::getDetectionMode;
static orbfe_aruco* (aruco::MarkerDetector::*volatile g_detector_handle)() = &aruco::MarkerDetector::handle;
static int (ORBmatcher::*volatile g_matcher)(Frame&, Frame&, std::vector<cv::Point2f>&, std::vector<int>&, int) = &ORBmatcher::SearchForInitialization;
static bool (Initializer::*volatile g_initializer)(const Frame&, const std::vector<int>&, cv::Mat&, cv::Mat&, std::vector<cv::Point3f>&,
                                                   std::vector<bool>&) = &Initializer::Initialize;
static int (*volatile g_pose)(Frame*) = &Optimizer::PoseOptimization;
static int (*volatile g_pose_aruco)(Frame*) = &Optimizer::PoseOptimizationByAruco;
static int (*volatile g_sim3_opt)(KeyFrame*, KeyFrame*, std::vector<MapPoint*>&, g2o::Sim3&, const float, const bool) = &Optimizer::OptimizeSim3;

static double no_score(const DBoW2::BowVector&, const DBoW2::BowVector&) { return 0; }

int main()
{
    int referenced = 0;
    referenced += g_extractor != nullptr;
    referenced += g_detector != nullptr && g_detector_handle != nullptr;
    referenced += g_matcher != nullptr;
    referenced += g_initializer != nullptr;
    referenced += g_pose != nullptr && g_pose_aruco != nullptr;
    referenced += g_sim3_opt != nullptr;

    // host-only members of the shims, on one Frame / KeyFrame / MapPoint declaration
    Frame F;
    F.mK = cv::Mat(3, 3, CV_32F);
    KeyFrame KF1, KF2;
    KF1.Rcw = KF2.Rcw = cv::Mat(3, 3, CV_32F);
    KF1.tcw = KF2.tcw = cv::Mat(3, 1, CV_32F);
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
    if (referenced != 6 || !T.empty() || !bNoMore || nInliers != 0 || candidates != 0 || marker.mLength != 0) return 1;
    printf("ok: 7 shims in one program\n");
    return 0;
}
