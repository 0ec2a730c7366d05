// TEST INFRASTRUCTURE ONLY -- the fuller ORB_SLAM2::KeyFrame of the GlobalBundleAdjustment shim (include/KeyFrame.h of the reference):
// what the LocalBundleAdjustment shim's mock holds, and the members a global bundle adjustment of loop closing leaves its result in.
// This directory goes ahead of tests/mock_orbslam_lba/ and tests/mock_orbslam/ on the include path of that shim's program alone; the
// guards are those of the headers it stands in for.
#ifndef MOCK_KEYFRAME_H
#define MOCK_KEYFRAME_H
#include <vector>
#include <opencv2/core/core.hpp>
#include "MapAruco.h"
#include "MapPoint.h"
namespace ORB_SLAM2 {
class KeyFrame {
public:
    long unsigned int mnId = 0;
    long unsigned int mnBAGlobalForKF = 0;
    bool mbBad = false;
    std::vector<cv::KeyPoint> mvKeysUn;
    std::vector<float> mvuRight, mvInvLevelSigma2;
    std::vector<MapPoint*> mvpMapPoints;
    float fx = 0, fy = 0, cx = 0, cy = 0;
    cv::Mat Tcw;       // 4 x 4 CV_32F
    cv::Mat mTcwGBA;
    int NA = 0;
    std::vector<bool> mvbOldAruco;
    std::vector<MapAruco*> mvpMapArucos;
    std::vector<cv::Point2f> mvArucoUn;
    int nSetPose = 0;
    bool isBad() { return mbBad; }
    cv::Mat GetPose() { return Tcw.clone(); }
    void SetPose(const cv::Mat& T) { Tcw = T.clone(); nSetPose++; }
};
}
#endif
