// TEST INFRASTRUCTURE ONLY -- the part of ORB_SLAM2::Optimizer that include/shims/Optimizer_globalba_orbfe.cc defines, with the
// reference's signature (include/Optimizer.h).
#ifndef MOCK_OPTIMIZER_H
#define MOCK_OPTIMIZER_H
#include <vector>
#include "Frame.h"
#include "KeyFrame.h"
#include "MapAruco.h"
#include "MapPoint.h"
namespace ORB_SLAM2 {
class Optimizer {
public:
    void static BundleAdjustment(const std::vector<KeyFrame*>& vpKF, const std::vector<MapPoint*>& vpMP, const std::vector<MapAruco*>& vpMA,
                                 int nIterations = 5, bool* pbStopFlag = NULL, const unsigned long nLoopKF = 0, const bool bRobust = true);
};
}
#endif
