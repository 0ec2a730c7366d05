// TEST INFRASTRUCTURE ONLY -- what the LocalBundleAdjustment shim touches of ORB_SLAM2::Map (include/Map.h of the reference).
#ifndef MOCK_MAP_H
#define MOCK_MAP_H
#include <map>
#include <mutex>
namespace ORB_SLAM2 {
class Map {
public:
    std::mutex mMutexMapUpdate;
    std::map<int, double> mArucoMeanLength;
};
}
#endif
