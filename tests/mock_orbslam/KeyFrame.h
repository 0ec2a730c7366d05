// TEST INFRASTRUCTURE ONLY -- the members of ORB_SLAM2::KeyFrame the shims of include/shims/ touch, with the reference's names and
// types (include/KeyFrame.h).  One class for all shims.
#ifndef MOCK_KEYFRAME_H
#define MOCK_KEYFRAME_H
#include <map>
#include <set>
#include <unordered_map>
#include <vector>
#include <opencv2/core/core.hpp>
#include "Thirdparty/DBoW2/DBoW2/BowVector.h"
#include "Thirdparty/DBoW2/DBoW2/FeatureVector.h"
#include "MapAruco.h"
#include "MapPoint.h"
namespace ORB_SLAM2 {
class KeyFrame {
public:
    // ORBmatcher, Sim3Solver, OptimizeSim3, OptimizeEssentialGraph: undistorted keypoints, the pose (3 x 3, 3 x 1) and the map points
    // by feature index
    std::vector<cv::KeyPoint> mvKeys, mvKeysUn;
    cv::Mat Rcw, tcw;
    std::vector<MapPoint*> mvpMapPoints;
    cv::Mat GetRotation() { return Rcw.clone(); }
    cv::Mat GetTranslation() { return tcw.clone(); }
    std::vector<MapPoint*> GetMapPointMatches() { return mvpMapPoints; }
    // the bundle adjustments: the pose, 4 x 4 CV_32F.  SetPose fills it, Rcw, tcw and the centre, as the reference's does
    cv::Mat Tcw;
    int nSetPose = 0;   // calls, for the test
    cv::Mat GetPose() { return Tcw.clone(); }
    void SetPose(const cv::Mat& Tcw_)
    {
        Tcw = Tcw_.clone();
        Rcw = Tcw.rowRange(0, 3).colRange(0, 3);
        tcw = Tcw.rowRange(0, 3).col(3);
        Ow = cv::Mat(3, 1, CV_32F);
        for (int r = 0; r < 3; r++) {
            float s = 0;
            for (int c = 0; c < 3; c++) s -= Rcw.at<float>(c, r) * tcw.at<float>(c);
            Ow.at<float>(r) = s;
        }
        nSetPose++;
    }
    // Sim3Solver, OptimizeSim3: the calibration matrix, 3 x 3 CV_32F
    cv::Mat mK;
    // ORBmatcher and Sim3Solver read mvLevelSigma2; ORBmatcher, OptimizeSim3 and the bundle adjustments mvInvLevelSigma2
    std::vector<float> mvLevelSigma2, mvInvLevelSigma2;
    // ORBmatcher: descriptors, FeatureVector, intrinsics (the bundle adjustments too), image bounds, scale pyramid, camera centre, map
    // bookkeeping
    int N = 0;
    cv::Mat mDescriptors;
    DBoW2::FeatureVector mFeatVec;
    float fx = 0, fy = 0, cx = 0, cy = 0;
    int mnMinX = 0, mnMinY = 0, mnMaxX = 0, mnMaxY = 0;
    int mnScaleLevels = 8;
    float mfScaleFactor = 1.2f, mfLogScaleFactor = 0;
    std::vector<float> mvScaleFactors;
    cv::Mat Ow;
    cv::Mat GetCameraCenter() { return Ow.clone(); }
    std::set<MapPoint*> GetMapPoints() { std::set<MapPoint*> s; for (MapPoint* p : mvpMapPoints) if (p && !p->isBad()) s.insert(p); return s; }
    MapPoint* GetMapPoint(const size_t& idx) { return mvpMapPoints[idx]; }
    void AddMapPoint(MapPoint* pMP, const size_t& idx) { mvpMapPoints[idx] = pMP; }
    // KeyFrameDatabase: the id, the BowVector, the six query fields (written by the reference's class only), and the covisibility
    // graph as the test sets it
    long unsigned int mnId = 0;
    DBoW2::BowVector mBowVec;
    long unsigned int mnLoopQuery = 0;
    int mnLoopWords = 0;
    float mLoopScore = 0;
    long unsigned int mnRelocQuery = 0;
    int mnRelocWords = 0;
    float mRelocScore = 0;
    bool mbBad = false;
    std::vector<KeyFrame*> mvpOrderedConnectedKeyFrames;   // by weight, best first
    std::set<KeyFrame*> GetConnectedKeyFrames() { return std::set<KeyFrame*>(mvpOrderedConnectedKeyFrames.begin(), mvpOrderedConnectedKeyFrames.end()); }
    std::vector<KeyFrame*> GetVectorCovisibleKeyFrames() { return mvpOrderedConnectedKeyFrames; }
    std::vector<KeyFrame*> GetBestCovisibilityKeyFrames(const int& N)
    {
        if ((int)mvpOrderedConnectedKeyFrames.size() < N) return mvpOrderedConnectedKeyFrames;
        return std::vector<KeyFrame*>(mvpOrderedConnectedKeyFrames.begin(), mvpOrderedConnectedKeyFrames.begin() + N);
    }
    bool isBad() { return mbBad; }
    // OptimizeEssentialGraph: the spanning tree, the loop edges, the covisibility weights
    KeyFrame* mpParent = nullptr;
    std::set<KeyFrame*> mspChildrens, mspLoopEdges;
    std::map<KeyFrame*, int> mConnectedKeyFrameWeights;
    KeyFrame* GetParent() { return mpParent; }
    bool hasChild(KeyFrame* pKF) { return mspChildrens.count(pKF) != 0; }
    std::set<KeyFrame*> GetLoopEdges() { return mspLoopEdges; }
    int GetWeight(KeyFrame* pKF) { return mConnectedKeyFrameWeights.count(pKF) ? mConnectedKeyFrameWeights[pKF] : 0; }
    std::vector<KeyFrame*> GetCovisiblesByWeight(const int& w)   // mvpOrderedConnectedKeyFrames is by weight, best first
    {
        std::vector<KeyFrame*> v;
        for (KeyFrame* p : mvpOrderedConnectedKeyFrames)
            if (GetWeight(p) >= w) v.push_back(p);
        return v;
    }
    // the bundle adjustments: their marks and results, the stereo coordinates (negative: monocular), the markers of the keyframe with
    // four undistorted corners each; OptimizeEssentialGraph: the markers by id
    long unsigned int mnBALocalForKF = 0, mnBAFixedForKF = 0, mnBAGlobalForKF = 0;
    cv::Mat mTcwGBA;
    std::vector<float> mvuRight;
    int NA = 0;
    std::vector<bool> mvbOldAruco;
    std::vector<MapAruco*> mvpMapArucos;
    std::vector<cv::Point2f> mvArucoUn;
    std::unordered_map<int, int> mmArucoIdandIdx;
    bool isIdxArucoOld(const size_t& idx) { return mvbOldAruco[idx]; }
    MapAruco* GetMapAruco(const size_t& idx) { return mvpMapArucos[idx]; }
    void EraseMapPointMatch(MapPoint* pMP)
    {
        for (size_t i = 0; i < mvpMapPoints.size(); i++)
            if (mvpMapPoints[i] == pMP) mvpMapPoints[i] = nullptr;
    }
};
}
#endif
