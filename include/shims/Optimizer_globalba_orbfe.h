/*
 * Optimizer_globalba_orbfe.h -- the flat problem that include/shims/Optimizer_globalba_orbfe.cc collects from the vectors it is given,
 * and the collect step itself, declared so that it can be run (and tested) without the library.
 */
#ifndef ORBFE_OPTIMIZER_GLOBALBA_H
#define ORBFE_OPTIMIZER_GLOBALBA_H

#include <cstdint>
#include <vector>

namespace ORB_SLAM2
{

class KeyFrame;
class MapAruco;
class MapPoint;

namespace orbfe_globalba
{

struct Problem {
    std::vector<KeyFrame*> vpKeyFrames;   // the keyframes of vpKFs that are not bad, in their order: the pose vertices
    std::vector<MapPoint*> vpMapPoints;   // the points of vpMP that are not bad, in their order
    std::vector<MapAruco*> vpMapArucos;   // with Frame::mbUArucoIni: the markers of vpMA that are not bad, in their order
    // the arrays of orbfe_global_bundle_adjustment
    std::vector<float> Tcw, x3Dw, obs_xy, Twm, marker_local, mobs_corners, inv_level_sigma2;
    std::vector<uint8_t> kf_fixed;
    std::vector<int32_t> obs_offset, obs_kf, obs_octave, mobs_offset, mobs_kf;
    float K4[4] = {0, 0, 0, 0};
};

// Lines 76-232 of src/Optimizer.cc as flat arrays, in the order g2o would have received the vertices and edges.  Throws
// std::runtime_error on a stereo observation.
void Collect(const std::vector<KeyFrame*>& vpKFs, const std::vector<MapPoint*>& vpMP, const std::vector<MapAruco*>& vpMA, Problem& pb);

} // namespace orbfe_globalba
} // namespace ORB_SLAM2

#endif
