// TEST INFRASTRUCTURE ONLY -- the members of ORB_SLAM2::MapPoint the OptimizeSim3 shim touches (include/MapPoint.h): the world
// position, the bad flag and the index of the point's observation in a keyframe.
#ifndef MOCK_OPTSIM3_MAPPOINT_H
#define MOCK_OPTSIM3_MAPPOINT_H
#include <map>
#include <opencv2/core/core.hpp>
namespace ORB_SLAM2 {
class KeyFrame;
class MapPoint {
public:
    cv::Mat mWorldPos;   // 3 x 1 CV_32F
    bool mbBad = false;
    std::map<KeyFrame*, size_t> mObservations;
    cv::Mat GetWorldPos() { return mWorldPos.clone(); }
    bool isBad() { return mbBad; }
    int GetIndexInKeyFrame(KeyFrame* pKF) { return mObservations.count(pKF) ? (int)mObservations[pKF] : -1; }
};
}
#endif
