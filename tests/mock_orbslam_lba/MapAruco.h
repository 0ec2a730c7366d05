// TEST INFRASTRUCTURE ONLY -- the fuller ORB_SLAM2::MapAruco of the LocalBundleAdjustment shim (include/MapAruco.h of the reference):
// id, bad flag, observations, the pose and its setter.
#ifndef MOCK_MAPARUCO_H
#define MOCK_MAPARUCO_H
#include <map>
#include <opencv2/core/core.hpp>
namespace ORB_SLAM2 {
class KeyFrame;
class MapAruco {
public:
    int mnArucoId = 0;
    bool mbBad = false;
    cv::Mat mTwm;   // 4 x 4 CV_32F
    double mLength = 0;
    std::map<KeyFrame*, size_t> mObservations;
    int GetMapArucoID() { return mnArucoId; }
    bool isBad() { return mbBad; }
    cv::Mat GetTwm() { return mTwm.clone(); }
    std::map<KeyFrame*, size_t> GetObservations() { return mObservations; }
    void SetRtwm(const cv::Mat& R, const cv::Mat& t)
    {
        for (int r = 0; r < 3; r++) {
            for (int c = 0; c < 3; c++) mTwm.at<float>(r, c) = R.at<float>(r, c);
            mTwm.at<float>(r, 3) = t.at<float>(r);
        }
    }
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
