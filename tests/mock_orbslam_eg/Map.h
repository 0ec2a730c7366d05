// TEST INFRASTRUCTURE ONLY -- what include/shims/Optimizer_essential_orbfe.cc touches of ORB_SLAM2::Map (include/Map.h of the reference).
#ifndef MOCK_MAP_H
#define MOCK_MAP_H
#include <mutex>
#include <vector>
namespace ORB_SLAM2 {
class KeyFrame;
class MapPoint;
class Map {
public:
    std::mutex mMutexMapUpdate;
    std::vector<KeyFrame*> mvpKeyFrames;
    std::vector<MapPoint*> mvpMapPoints;
    std::vector<KeyFrame*> GetAllKeyFrames() { return mvpKeyFrames; }
    std::vector<MapPoint*> GetAllMapPoints() { return mvpMapPoints; }
};
}
#endif
