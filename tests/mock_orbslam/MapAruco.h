// TEST INFRASTRUCTURE ONLY -- the members of ORB_SLAM2::MapAruco the shims of include/shims/ touch, with the reference's names and
// types (include/MapAruco.h): id, bad flag, observations, the marker pose with its setters, and the corners in the marker frame, a
// square of side mLength (src/MapAruco.cc's order).  One class for all shims.
#ifndef MOCK_MAPARUCO_H
#define MOCK_MAPARUCO_H
#include <map>
#include "Frame.h"
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
    cv::Mat GetTwm() { return mTwm; }
    std::map<KeyFrame*, size_t> GetObservations() { return mObservations; }
    // the bundle adjustments
    void SetRtwm(const cv::Mat& R, const cv::Mat& t)
    {
        for (int r = 0; r < 3; r++) {
            for (int c = 0; c < 3; c++) mTwm.at<float>(r, c) = R.at<float>(r, c);
            mTwm.at<float>(r, 3) = t.at<float>(r);
        }
    }
    // OptimizeEssentialGraph: the two calls record their arguments for the test
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
