/*
 * Optimizer_localba_orbfe.h -- the flat problem that include/shims/Optimizer_localba_orbfe.cc collects from the map, and the collect
 * step itself, declared so that it can be run (and tested) without the library.
 */
#ifndef ORBFE_OPTIMIZER_LOCALBA_H
#define ORBFE_OPTIMIZER_LOCALBA_H

#include <cstdint>
#include <vector>

#include "Optimizer_ba_orbfe.h"

namespace ORB_SLAM2
{

class Map;

namespace orbfe_localba
{

struct Problem : orbfe_ba::Arrays {   // with the arrays of orbfe_local_bundle_adjustment
    std::vector<KeyFrame*> vpKeyFrames;   // lLocalKeyFrames in list order, then lFixedCameras in list order: the pose vertices
    size_t nLocal = 0;                    // how many of them are local
    std::vector<MapPoint*> vpMapPoints;   // lLocalMapPoints in list order
    std::vector<MapAruco*> vpMapArucos;   // vLocalMapArucosMono
    // edge e is the observation of vpEdgeMP[e] in vpEdgeKF[e], in the order g2o would have received the edges
    std::vector<KeyFrame*> vpEdgeKF;
    std::vector<MapPoint*> vpEdgeMP;
};

// Lines 777-888 of src/Optimizer.cc (the marks mnBALocalForKF / mnBAFixedForKF included) and the flat arrays of lines 907-1115.
// Throws std::runtime_error on a stereo observation.
void Collect(KeyFrame* pKF, Map* pMap, Problem& pb);

} // namespace orbfe_localba
} // namespace ORB_SLAM2

#endif
