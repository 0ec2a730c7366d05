// TEST INFRASTRUCTURE ONLY -- ORB_SLAM2::MapPoint of tests/mock_orbslam/ with what include/shims/Optimizer_essential_orbfe.cc touches
// on top (include/MapPoint.h of the reference): the setter, the loop-correction marks, the marker fields, the reference keyframe.
#ifndef MOCK_MAPPOINT_H
#define MOCK_MAPPOINT_H
#include <map>
#include <opencv2/core/core.hpp>
namespace ORB_SLAM2 {
class KeyFrame;
class MapPoint {
public:
    // every shim that takes map points (ORBmatcher, Sim3Solver, both Optimizer shims): the world position, 3 x 1 CV_32F
    cv::Mat mWorldPos;
    cv::Mat GetWorldPos() { return mWorldPos.clone(); }
    // ORBmatcher, Sim3Solver, OptimizeSim3: the bad flag and the index of the point's observation in a keyframe
    bool mbBad = false;
    std::map<KeyFrame*, size_t> mObservations;
    bool isBad() { return mbBad; }
    int GetIndexInKeyFrame(KeyFrame* pKF) { return mObservations.count(pKF) ? (int)mObservations[pKF] : -1; }
    // ORBmatcher: normal, descriptor, distance range, observation count and the map bookkeeping after a match
    cv::Mat mNormal, mDescriptor;
    float mfMinDistance = 0, mfMaxDistance = 0;
    int nObs = 1;
    MapPoint* mpReplaced = nullptr;
    cv::Mat GetNormal() { return mNormal.clone(); }
    cv::Mat GetDescriptor() { return mDescriptor.clone(); }
    int Observations() { return nObs; }
    float GetMinDistanceInvariance() { return 0.8f * mfMinDistance; }
    float GetMaxDistanceInvariance() { return 1.2f * mfMaxDistance; }
    float GetMinDistance() { return mfMinDistance; }   // the two getters the shim asks the maintainer to add
    float GetMaxDistance() { return mfMaxDistance; }
    bool IsInKeyFrame(KeyFrame* pKF) { return mObservations.count(pKF) != 0; }
    void AddObservation(KeyFrame* pKF, size_t idx) { if (!mObservations.count(pKF)) { mObservations[pKF] = idx; nObs++; } }
    void Replace(MapPoint* pMP) { if (pMP != this) { mbBad = true; mpReplaced = pMP; } }
    // ORBmatcher: the tracking fields (MapPoint.h:93-100)
    float mTrackProjX = 0, mTrackProjY = 0, mTrackProjXR = 0, mTrackViewCos = 1;
    bool mbTrackInView = false;
    int mnTrackScaleLevel = 0;
    // OptimizeEssentialGraph
    long unsigned int mnCorrectedByKF = 0, mnCorrectedReference = 0;
    bool forflag = false;
    int mArucoID = -1;
    KeyFrame* mpRefKF = nullptr;
    int nSetWorldPos = 0, nUpdates = 0;   // calls, for the test
    KeyFrame* GetReferenceKeyFrame() { return mpRefKF; }
    void SetWorldPos(const cv::Mat& Pos) { mWorldPos = Pos.clone(); nSetWorldPos++; }
    void UpdateNormalAndDepth() { nUpdates++; }
};
}
#endif
