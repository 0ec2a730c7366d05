// TEST INFRASTRUCTURE ONLY -- the members of ORB_SLAM2::Frame the pose optimization shim touches (include/Frame.h of the
// reference), with their names and types.  Compiled against the mock OpenCV of tests/mock_cv plus cv::Point3f.
#ifndef MOCK_POSE_FRAME_H
#define MOCK_POSE_FRAME_H
#include <vector>
#include <opencv2/core/core.hpp>

namespace cv {
template <class T> struct Point3_ { T x, y, z; Point3_() : x(0), y(0), z(0) {} Point3_(T a, T b, T c) : x(a), y(b), z(c) {} };
typedef Point3_<float> Point3f;
}

namespace ORB_SLAM2 {
class MapPoint;
class MapAruco;
class Frame {
public:
    int N = 0;
    int NA = 0;
    std::vector<cv::KeyPoint> mvKeysUn;
    std::vector<float> mvuRight;
    std::vector<MapPoint*> mvpMapPoints;
    std::vector<MapAruco*> mvpMapArucos;
    std::vector<cv::Point2f> mvArucoUn;
    std::vector<bool> mvbOutlier, mvbArucoGood, mvbOldAruco;
    std::vector<float> mvInvLevelSigma2;
    cv::Mat mTcw;
    static float fx, fy, cx, cy;
    static bool mbUArucoIni;
    void SetPose(cv::Mat Tcw) { mTcw = Tcw.clone(); }
};
}
#endif
