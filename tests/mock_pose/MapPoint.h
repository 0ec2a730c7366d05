// TEST INFRASTRUCTURE ONLY -- ORB_SLAM2::MapPoint as the pose optimization shim uses it (include/MapPoint.h): the world position.
#ifndef MOCK_POSE_MAPPOINT_H
#define MOCK_POSE_MAPPOINT_H
#include <opencv2/core/core.hpp>
namespace ORB_SLAM2 {
class MapPoint {
public:
    cv::Mat mWorldPos;   // 3 x 1 CV_32F
    cv::Mat GetWorldPos() { return mWorldPos.clone(); }
};
}
#endif
