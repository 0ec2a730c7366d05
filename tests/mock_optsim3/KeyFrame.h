// TEST INFRASTRUCTURE ONLY -- the members of ORB_SLAM2::KeyFrame the OptimizeSim3 shim touches (include/KeyFrame.h): the undistorted
// keypoints, the inverse level table, the calibration matrix, the pose and the map points by feature index.
#ifndef MOCK_OPTSIM3_KEYFRAME_H
#define MOCK_OPTSIM3_KEYFRAME_H
#include <vector>
#include <opencv2/core/core.hpp>
#include "MapPoint.h"
namespace ORB_SLAM2 {
class KeyFrame {
public:
    std::vector<cv::KeyPoint> mvKeysUn;
    std::vector<float> mvInvLevelSigma2;
    cv::Mat mK;          // 3 x 3 CV_32F
    cv::Mat Rcw, tcw;    // 3 x 3, 3 x 1
    std::vector<MapPoint*> mvpMapPoints;
    cv::Mat GetRotation() { return Rcw.clone(); }
    cv::Mat GetTranslation() { return tcw.clone(); }
    std::vector<MapPoint*> GetMapPointMatches() { return mvpMapPoints; }
};
}
#endif
