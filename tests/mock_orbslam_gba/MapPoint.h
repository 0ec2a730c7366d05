// TEST INFRASTRUCTURE ONLY -- the fuller ORB_SLAM2::MapPoint of the GlobalBundleAdjustment shim (include/MapPoint.h of the reference):
// the observation map, the setters, and the members a global bundle adjustment of loop closing leaves its result in.
#ifndef MOCK_MAPPOINT_H
#define MOCK_MAPPOINT_H
#include <map>
#include <opencv2/core/core.hpp>
namespace ORB_SLAM2 {
class KeyFrame;
class MapPoint {
public:
    long unsigned int mnId = 0;
    long unsigned int mnBAGlobalForKF = 0;
    int forflag = 0, mArucoID = -1;
    cv::Mat mWorldPos;   // 3 x 1 CV_32F
    cv::Mat mPosGBA;
    bool mbBad = false;
    std::map<KeyFrame*, size_t> mObservations;
    int nUpdates = 0;    // calls of UpdateNormalAndDepth, for the test
    cv::Mat GetWorldPos() { return mWorldPos.clone(); }
    void SetWorldPos(const cv::Mat& Pos) { mWorldPos = Pos.clone(); }
    bool isBad() { return mbBad; }
    std::map<KeyFrame*, size_t> GetObservations() { return mObservations; }
    void UpdateNormalAndDepth() { nUpdates++; }
};
}
#endif
