// TEST INFRASTRUCTURE ONLY -- the part of ORB_SLAM2::Optimizer (include/Optimizer.h of the reference) that the shims define, with
// the reference's signatures and default arguments.  One class, as in the reference: the five Optimizer shims link into one program.
#ifndef MOCK_OPTIMIZER_H
#define MOCK_OPTIMIZER_H
#include <map>
#include <set>
#include <vector>
#include "Frame.h"
#include "KeyFrame.h"
#include "LoopClosing.h"
#include "Map.h"
#include "MapAruco.h"
#include "MapPoint.h"
#include "Thirdparty/g2o/g2o/types/types_seven_dof_expmap.h"
namespace ORB_SLAM2 {
class Optimizer {
public:
    // include/shims/Optimizer_globalba_orbfe.cc
    void static BundleAdjustment(const std::vector<KeyFrame*>& vpKF, const std::vector<MapPoint*>& vpMP, const std::vector<MapAruco*>& vpMA,
                                 int nIterations = 5, bool* pbStopFlag = NULL, const unsigned long nLoopKF = 0, const bool bRobust = true);
    // include/shims/Optimizer_localba_orbfe.cc
    void static LocalBundleAdjustment(KeyFrame* pKF, bool* pbStopFlag, Map* pMap);
    // include/shims/Optimizer_pose_orbfe.cc
    int static PoseOptimization(Frame* pFrame);
    int static PoseOptimizationByAruco(Frame* pFrame);
    // include/shims/Optimizer_essential_orbfe.cc
    void static OptimizeEssentialGraph(Map* pMap, KeyFrame* pLoopKF, KeyFrame* pCurKF, const LoopClosing::KeyFrameAndPose& NonCorrectedSim3,
                                       const LoopClosing::KeyFrameAndPose& CorrectedSim3,
                                       const std::map<KeyFrame*, std::set<KeyFrame*> >& LoopConnections, const bool& bFixScale);
    // include/shims/Optimizer_sim3_orbfe.cc
    static int OptimizeSim3(KeyFrame* pKF1, KeyFrame* pKF2, std::vector<MapPoint*>& vpMatches1, g2o::Sim3& g2oS12, const float th2,
                            const bool bFixScale);
};
}
#endif
