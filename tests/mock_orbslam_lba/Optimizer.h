// TEST INFRASTRUCTURE ONLY -- the part of ORB_SLAM2::Optimizer that include/shims/Optimizer_localba_orbfe.cc defines, with the
// reference's signature (include/Optimizer.h).
#ifndef MOCK_OPTIMIZER_H
#define MOCK_OPTIMIZER_H
#include "Frame.h"
#include "KeyFrame.h"
#include "Map.h"
#include "MapPoint.h"
namespace ORB_SLAM2 {
class Optimizer {
public:
    void static LocalBundleAdjustment(KeyFrame* pKF, bool* pbStopFlag, Map* pMap);
};
}
#endif
