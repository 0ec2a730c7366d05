// TEST INFRASTRUCTURE ONLY -- the members of ORB_SLAM2::Frame that KeyFrameDatabase touches (include/Frame.h).
#ifndef MOCK_KFDB_FRAME_H
#define MOCK_KFDB_FRAME_H
#include "Thirdparty/DBoW2/DBoW2/BowVector.h"
namespace ORB_SLAM2 {
class Frame {
public:
    Frame() : mnId(0) {}
    long unsigned int mnId;
    DBoW2::BowVector mBowVec;
};
}
#endif
