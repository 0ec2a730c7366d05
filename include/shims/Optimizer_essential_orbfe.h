/*
 * Optimizer_essential_orbfe.h -- the flat problem that include/shims/Optimizer_essential_orbfe.cc collects from the map, and the
 * collect step itself, declared so that it can be run (and tested) without the library.
 */
#ifndef ORBFE_OPTIMIZER_ESSENTIAL_H
#define ORBFE_OPTIMIZER_ESSENTIAL_H

#include <cstdint>
#include <map>
#include <set>
#include <vector>

#include "LoopClosing.h"

namespace ORB_SLAM2
{

class KeyFrame;
class Map;
class MapPoint;

namespace orbfe_essential
{

struct Problem {
    std::vector<KeyFrame*> vpKeyFrames;   // the vertices: GetAllKeyFrames() without the bad ones, in its order ("positions")
    std::vector<MapPoint*> vpMapPoints;   // GetAllMapPoints(), bad ones included (point_ref -1)
    // the arrays of orbfe_optimize_essential_graph
    std::vector<int32_t> kf_id, corrected_pos, noncorrected_pos, edge_i, edge_j, edge_kind, point_ref;
    std::vector<float> Tcw, x3Dw;
    std::vector<double> corrected, noncorrected;
    int fixed = -1;
};

// Lines 1261-1447 of src/Optimizer.cc (which keyframes are vertices, which edges exist and in which order) and the nIDr rule of
// lines 1487-1496.  Throws std::runtime_error when pLoopKF is no vertex.
void Collect(Map* pMap, KeyFrame* pLoopKF, KeyFrame* pCurKF, const LoopClosing::KeyFrameAndPose& NonCorrectedSim3,
             const LoopClosing::KeyFrameAndPose& CorrectedSim3, const std::map<KeyFrame*, std::set<KeyFrame*> >& LoopConnections, Problem& pb);

} // namespace orbfe_essential
} // namespace ORB_SLAM2

#endif
