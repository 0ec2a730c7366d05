// TEST INFRASTRUCTURE ONLY -- the fuller ORB_SLAM2::KeyFrame of the LocalBundleAdjustment shim (include/KeyFrame.h of the reference):
// the bundle adjustment marks, the covisibility list, the pose, the keypoints, and the markers of the keyframe.
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
    long unsigned int mnBALocalForKF = 0, mnBAFixedForKF = 0;
    bool mbBad = false;
    std::vector<KeyFrame*> mvpOrderedConnectedKeyFrames;
    std::vector<cv::KeyPoint> mvKeysUn;
    std::vector<float> mvuRight, mvInvLevelSigma2;
    std::vector<MapPoint*> mvpMapPoints;
    float fx = 0, fy = 0, cx = 0, cy = 0;
    cv::Mat Tcw;   // 4 x 4 CV_32F
    int NA = 0;
    std::vector<bool> mvbOldAruco;
    std::vector<MapAruco*> mvpMapArucos;
    std::vector<cv::Point2f> mvArucoUn;
    int nSetPose = 0;
    bool isBad() { return mbBad; }
    std::vector<KeyFrame*> GetVectorCovisibleKeyFrames() { return mvpOrderedConnectedKeyFrames; }
    std::vector<MapPoint*> GetMapPointMatches() { return mvpMapPoints; }
    bool isIdxArucoOld(size_t i) { return mvbOldAruco[i]; }
    MapAruco* GetMapAruco(size_t i) { return mvpMapArucos[i]; }
    cv::Mat GetPose() { return Tcw.clone(); }
    void SetPose(const cv::Mat& T) { Tcw = T.clone(); nSetPose++; }
    void EraseMapPointMatch(MapPoint* pMP)
    {
        for (size_t i = 0; i < mvpMapPoints.size(); i++)
            if (mvpMapPoints[i] == pMP) mvpMapPoints[i] = nullptr;
    }
};
}
#endif
