// TEST INFRASTRUCTURE ONLY -- the members of ORB_SLAM2::MapPoint the shims of include/shims/ touch, with the reference's names and
// types (include/MapPoint.h), so that they compile and run without the SLAM system.  One class for all shims.
#ifndef MOCK_MAPPOINT_H
#define MOCK_MAPPOINT_H
#include <map>
#include <opencv2/core/core.hpp>
namespace ORB_SLAM2 {
class KeyFrame;
class MapPoint {
public:
    // every shim that takes map points: the world position, 3 x 1 CV_32F, and its setter
    cv::Mat mWorldPos;
    cv::Mat GetWorldPos() { return mWorldPos.clone(); }
    void SetWorldPos(const cv::Mat& Pos) { mWorldPos = Pos.clone(); nSetWorldPos++; }
    void UpdateNormalAndDepth() { nUpdates++; }
    int nSetWorldPos = 0, nUpdates = 0;   // calls, for the test
    // the bad flag and the observations: the index of the point's feature in every keyframe that sees it
    long unsigned int mnId = 0;
    bool mbBad = false;
    std::map<KeyFrame*, size_t> mObservations;
    bool isBad() { return mbBad; }
    int GetIndexInKeyFrame(KeyFrame* pKF) { return mObservations.count(pKF) ? (int)mObservations[pKF] : -1; }
    std::map<KeyFrame*, size_t> GetObservations() { return mObservations; }
    void EraseObservation(KeyFrame* pKF) { mObservations.erase(pKF); }
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
    // the bundle adjustments: their marks, and where a global one of loop closing leaves its result
    long unsigned int mnBALocalForKF = 0, mnBAGlobalForKF = 0;
    cv::Mat mPosGBA;
    // OptimizeEssentialGraph: the loop-correction marks, the marker fields, the reference keyframe
    long unsigned int mnCorrectedByKF = 0, mnCorrectedReference = 0;
    bool forflag = false;
    int mArucoID = -1;
    KeyFrame* mpRefKF = nullptr;
    KeyFrame* GetReferenceKeyFrame() { return mpRefKF; }
};
}
#endif
