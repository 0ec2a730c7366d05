// TEST INFRASTRUCTURE ONLY -- ORB_SLAM2::MapAruco of tests/mock_orbslam/ with what include/shims/Optimizer_essential_orbfe.cc calls on
// top (include/MapAruco.h): isBad, UpdateTcmByKF and SetRtwmByKeyFrame, which record their arguments for the test.
#ifndef MOCK_MAPARUCO_H
#define MOCK_MAPARUCO_H
#include "Frame.h"
namespace ORB_SLAM2 {
class KeyFrame;
class MapAruco {
public:
    cv::Mat mTwm;   // 4 x 4 CV_32F
    double mLength = 0;
    cv::Mat GetTwm() { return mTwm; }
    bool mbBad = false;
    bool isBad() { return mbBad; }
    int nUpdateTcm = 0, nSetRtwm = 0;
    KeyFrame* pLastKF = nullptr;
    size_t nLastIdx = 0;
    cv::Mat mLastRwc, mLastTwc;
    void UpdateTcmByKF(KeyFrame* pKF, size_t idx) { pLastKF = pKF; nLastIdx = idx; nUpdateTcm++; }
    void SetRtwmByKeyFrame(const cv::Mat& Rwc, const cv::Mat& twc) { mLastRwc = Rwc.clone(); mLastTwc = twc.clone(); nSetRtwm++; }
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
