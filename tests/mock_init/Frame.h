// TEST INFRASTRUCTURE ONLY -- the members of ORB_SLAM2::Frame the Initializer shim touches (include/Frame.h of the reference):
// the undistorted keypoints and the calibration matrix.
#ifndef MOCK_INIT_FRAME_H
#define MOCK_INIT_FRAME_H
#include <vector>
#include <opencv2/core/core.hpp>
namespace ORB_SLAM2 {
class Frame {
public:
    std::vector<cv::KeyPoint> mvKeys, mvKeysUn;
    cv::Mat mK;
};
}
#endif
