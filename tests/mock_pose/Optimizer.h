// TEST INFRASTRUCTURE ONLY -- the part of ORB_SLAM2::Optimizer (include/Optimizer.h of the reference) that
// include/shims/Optimizer_pose_orbfe.cc defines: the two motion-only pose optimizations, with the reference's signatures.
#ifndef MOCK_OPTIMIZER_H
#define MOCK_OPTIMIZER_H
#include "Frame.h"
namespace ORB_SLAM2 {
class Optimizer {
public:
    int static PoseOptimization(Frame* pFrame);
    int static PoseOptimizationByAruco(Frame* pFrame);
};
}
#endif
