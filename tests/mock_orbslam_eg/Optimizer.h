// TEST INFRASTRUCTURE ONLY -- the part of ORB_SLAM2::Optimizer (include/Optimizer.h of the reference) that the shims define, with
// the reference's signatures: the two motion-only pose optimizations (include/shims/Optimizer_pose_orbfe.cc) and OptimizeSim3
// (include/shims/Optimizer_sim3_orbfe.cc).  One class, as in the reference: the shims link into one program.  This copy adds
// OptimizeEssentialGraph and goes ahead of tests/mock_orbslam/Optimizer.h on the include path.
#ifndef MOCK_OPTIMIZER_H
#define MOCK_OPTIMIZER_H
#include <vector>
#include "Frame.h"
#include "KeyFrame.h"
#include "LoopClosing.h"
#include "Map.h"
#include "MapPoint.h"
#include <map>
#include <set>
#include "Thirdparty/g2o/g2o/types/types_seven_dof_expmap.h"
namespace ORB_SLAM2 {
class Optimizer {
public:
    int static PoseOptimization(Frame* pFrame);
    int static PoseOptimizationByAruco(Frame* pFrame);
    static int OptimizeSim3(KeyFrame* pKF1, KeyFrame* pKF2, std::vector<MapPoint*>& vpMatches1, g2o::Sim3& g2oS12, const float th2,
                            const bool bFixScale);
    // include/shims/Optimizer_essential_orbfe.cc
    void static OptimizeEssentialGraph(Map* pMap, KeyFrame* pLoopKF, KeyFrame* pCurKF, const LoopClosing::KeyFrameAndPose& NonCorrectedSim3,
                                       const LoopClosing::KeyFrameAndPose& CorrectedSim3,
                                       const std::map<KeyFrame*, std::set<KeyFrame*> >& LoopConnections, const bool& bFixScale);
};
}
#endif
