/*
 * Optimizer_globalba_orbfe.h -- the flat problem that include/shims/Optimizer_globalba_orbfe.cc collects from the vectors it is given,
 * and the collect step itself, declared so that it can be run (and tested) without the library.
 */
#ifndef ORBFE_OPTIMIZER_GLOBALBA_H
#define ORBFE_OPTIMIZER_GLOBALBA_H

#include <cstdint>
#include <vector>

#include "Optimizer_ba_orbfe.h"

namespace ORB_SLAM2
{

namespace orbfe_globalba
{

struct Problem : orbfe_ba::Arrays {   // with the arrays of orbfe_global_bundle_adjustment
    std::vector<KeyFrame*> vpKeyFrames;   // the keyframes of vpKFs that are not bad, in their order: the pose vertices
    std::vector<MapPoint*> vpMapPoints;   // the points of vpMP that are not bad, in their order
    std::vector<MapAruco*> vpMapArucos;   // with Frame::mbUArucoIni: the markers of vpMA that are not bad, in their order
};

// Lines 76-232 of src/Optimizer.cc as flat arrays, in the order g2o would have received the vertices and edges.  Throws
// std::runtime_error on a stereo observation.
void Collect(const std::vector<KeyFrame*>& vpKFs, const std::vector<MapPoint*>& vpMP, const std::vector<MapAruco*>& vpMA, Problem& pb);

} // namespace orbfe_globalba
} // namespace ORB_SLAM2

#endif
