// TEST INFRASTRUCTURE ONLY -- ORB_SLAM2::MapAruco as the pose optimization shim uses it (include/MapAruco.h): the marker pose
// and its corners in the marker frame, a square of side mLength (src/MapAruco.cc's order).
#ifndef MOCK_MAPARUCO_H
#define MOCK_MAPARUCO_H
#include "Frame.h"
namespace ORB_SLAM2 {
class MapAruco {
public:
    cv::Mat mTwm;   // 4 x 4 CV_32F
    double mLength = 0;
    cv::Mat GetTwm() { return mTwm; }
    cv::Point3f get3DPointsLocalRefSystem(size_t i)
    {
        const float h = (float)(mLength / 2.);
        if (i == 0) return cv::Point3f(-h, h, 0);
        if (i == 1) return cv::Point3f(h, h, 0);
        if (i == 2) return cv::Point3f(h, -h, 0);
        return cv::Point3f(-h, -h, 0);
    }
};
}
#endif
