// TEST INFRASTRUCTURE ONLY -- the members of ORB_SLAM2::KeyFrame the Sim3Solver shim touches (include/KeyFrame.h): the undistorted
// keypoints, the level table, the calibration matrix, the pose and the map points by feature index.
#ifndef MOCK_SIM3_KEYFRAME_H
#define MOCK_SIM3_KEYFRAME_H
#include <vector>
#include <opencv2/core/core.hpp>
#include "MapPoint.h"
namespace ORB_SLAM2 {
class KeyFrame {
public:
    std::vector<cv::KeyPoint> mvKeysUn;
    std::vector<float> mvLevelSigma2;
    cv::Mat mK;          // 3 x 3 CV_32F
    cv::Mat Rcw, tcw;    // 3 x 3, 3 x 1
    std::vector<MapPoint*> mvpMapPoints;
    cv::Mat GetRotation() { return Rcw.clone(); }
    cv::Mat GetTranslation() { return tcw.clone(); }
    std::vector<MapPoint*> GetMapPointMatches() { return mvpMapPoints; }
};
}
#endif
