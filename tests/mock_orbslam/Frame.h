// TEST INFRASTRUCTURE ONLY -- the members of ORB_SLAM2::Frame the shims of include/shims/ touch, with the reference's names and
// types (include/Frame.h).  One class for all shims; its static members are defined in Frame_statics.cc, which every program links.
#ifndef MOCK_FRAME_H
#define MOCK_FRAME_H
#include <vector>
#include <opencv2/core/core.hpp>
#include "Thirdparty/DBoW2/DBoW2/BowVector.h"
#include "Thirdparty/DBoW2/DBoW2/FeatureVector.h"
namespace ORB_SLAM2 {
class MapPoint;
class MapAruco;
class Frame {
public:
    // ORBmatcher, Initializer, PoseOptimization: the keypoints (Initializer and PoseOptimization read mvKeysUn only)
    int N = 0;
    std::vector<cv::KeyPoint> mvKeys, mvKeysUn;
    // Initializer: the calibration matrix, 3 x 3 CV_32F
    cv::Mat mK;
    // ORBmatcher, PoseOptimization: map points, outlier flags, stereo coordinates, pose, intrinsics, the inverse level table
    std::vector<MapPoint*> mvpMapPoints;
    std::vector<bool> mvbOutlier;
    std::vector<float> mvuRight;
    cv::Mat mTcw;
    static float fx, fy, cx, cy, invfx, invfy;
    std::vector<float> mvScaleFactors, mvInvScaleFactors, mvLevelSigma2, mvInvLevelSigma2;
    void SetPose(cv::Mat Tcw) { mTcw = Tcw.clone(); }
    // ORBmatcher: descriptors, FeatureVector, scale pyramid, image bounds
    cv::Mat mDescriptors;
    DBoW2::FeatureVector mFeatVec;
    int mnScaleLevels = 8;
    float mfScaleFactor = 1.2f, mfLogScaleFactor = 0;
    static float mnMinX, mnMaxX, mnMinY, mnMaxY;
    // PoseOptimizationByAruco: the markers of the frame, four undistorted corners each
    int NA = 0;
    std::vector<MapAruco*> mvpMapArucos;
    std::vector<cv::Point2f> mvArucoUn;
    std::vector<bool> mvbArucoGood, mvbOldAruco;
    static bool mbUArucoIni;
    // KeyFrameDatabase: the id and the BowVector
    long unsigned int mnId = 0;
    DBoW2::BowVector mBowVec;
};
}
#endif
