// TEST INFRASTRUCTURE ONLY -- what the shims of include/shims/ touch of ORB_SLAM2::Map (include/Map.h of the reference): the update
// mutex (LocalBundleAdjustment, OptimizeEssentialGraph), the mean marker lengths, and the keyframes and points of the map.
#ifndef MOCK_MAP_H
#define MOCK_MAP_H
#include <map>
#include <mutex>
#include <vector>
namespace ORB_SLAM2 {
class KeyFrame;
class MapPoint;
class Map {
public:
    std::mutex mMutexMapUpdate;
    std::map<int, double> mArucoMeanLength;
    std::vector<KeyFrame*> mvpKeyFrames;
    std::vector<MapPoint*> mvpMapPoints;
    std::vector<KeyFrame*> GetAllKeyFrames() { return mvpKeyFrames; }
    std::vector<MapPoint*> GetAllMapPoints() { return mvpMapPoints; }
};
}
#endif
