// TEST INFRASTRUCTURE ONLY -- the fuller ORB_SLAM2::MapPoint that include/shims/Optimizer_localba_orbfe.cc touches (include/MapPoint.h
// of the reference): the observation map, the bundle adjustment marks and the setters.  This directory goes ahead of tests/mock_orbslam/
// on the include path of that shim's program alone; the guards are those of the headers it stands in for.
#ifndef MOCK_MAPPOINT_H
#define MOCK_MAPPOINT_H
#include <map>
#include <opencv2/core/core.hpp>
namespace ORB_SLAM2 {
class KeyFrame;
class MapPoint {
public:
    long unsigned int mnId = 0;
    long unsigned int mnBALocalForKF = 0;
    int forflag = 0, mArucoID = -1;
    cv::Mat mWorldPos;   // 3 x 1 CV_32F
    bool mbBad = false;
    std::map<KeyFrame*, size_t> mObservations;
    int nUpdates = 0;    // calls of UpdateNormalAndDepth, for the test
    cv::Mat GetWorldPos() { return mWorldPos.clone(); }
    void SetWorldPos(const cv::Mat& Pos) { mWorldPos = Pos.clone(); }
    bool isBad() { return mbBad; }
    std::map<KeyFrame*, size_t> GetObservations() { return mObservations; }
    void EraseObservation(KeyFrame* pKF) { mObservations.erase(pKF); }
    void UpdateNormalAndDepth() { nUpdates++; }
};
}
#endif
