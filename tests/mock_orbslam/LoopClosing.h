// TEST INFRASTRUCTURE ONLY -- the one type include/shims/Optimizer_essential_orbfe.cc takes from ORB_SLAM2::LoopClosing
// (include/LoopClosing.h of the reference, where the map also names Eigen's aligned allocator).
#ifndef MOCK_LOOPCLOSING_H
#define MOCK_LOOPCLOSING_H
#include <map>
#include "KeyFrame.h"
#include "Thirdparty/g2o/g2o/types/types_seven_dof_expmap.h"
namespace ORB_SLAM2 {
class LoopClosing {
public:
    typedef std::map<KeyFrame*, g2o::Sim3, std::less<KeyFrame*> > KeyFrameAndPose;
};
}
#endif
