// TEST INFRASTRUCTURE ONLY -- the part of ORB_SLAM2::Optimizer (include/Optimizer.h of the reference) that
// include/shims/Optimizer_sim3_orbfe.cc defines: OptimizeSim3, with the reference's signature.
#ifndef MOCK_OPTSIM3_OPTIMIZER_H
#define MOCK_OPTSIM3_OPTIMIZER_H
#include <vector>
#include "KeyFrame.h"
#include "MapPoint.h"
#include "Thirdparty/g2o/g2o/types/types_seven_dof_expmap.h"
namespace ORB_SLAM2 {
class Optimizer {
public:
    static int OptimizeSim3(KeyFrame* pKF1, KeyFrame* pKF2, std::vector<MapPoint*>& vpMatches1, g2o::Sim3& g2oS12, const float th2,
                            const bool bFixScale);
};
}
#endif
