// TEST INFRASTRUCTURE ONLY -- the members of ORB_SLAM2::KeyFrame that KeyFrameDatabase touches (include/KeyFrame.h): the id, the
// BowVector, the six query fields, and the covisibility graph as the test sets it.
#ifndef MOCK_KFDB_KEYFRAME_H
#define MOCK_KFDB_KEYFRAME_H
#include <set>
#include <vector>
#include "Thirdparty/DBoW2/DBoW2/BowVector.h"
namespace ORB_SLAM2 {
class KeyFrame {
public:
    KeyFrame() : mnId(0), mnLoopQuery(0), mnLoopWords(0), mLoopScore(0), mnRelocQuery(0), mnRelocWords(0), mRelocScore(0), mbBad(false) {}
    long unsigned int mnId;
    DBoW2::BowVector mBowVec;
    long unsigned int mnLoopQuery;
    int mnLoopWords;
    float mLoopScore;
    long unsigned int mnRelocQuery;
    int mnRelocWords;
    float mRelocScore;
    bool mbBad;
    std::vector<KeyFrame*> mvpOrderedConnectedKeyFrames;   // by weight, best first
    std::set<KeyFrame*> GetConnectedKeyFrames() { return std::set<KeyFrame*>(mvpOrderedConnectedKeyFrames.begin(), mvpOrderedConnectedKeyFrames.end()); }
    std::vector<KeyFrame*> GetVectorCovisibleKeyFrames() { return mvpOrderedConnectedKeyFrames; }
    std::vector<KeyFrame*> GetBestCovisibilityKeyFrames(const int& N)
    {
        if ((int)mvpOrderedConnectedKeyFrames.size() < N) return mvpOrderedConnectedKeyFrames;
        return std::vector<KeyFrame*>(mvpOrderedConnectedKeyFrames.begin(), mvpOrderedConnectedKeyFrames.begin() + N);
    }
    bool isBad() { return mbBad; }
};
}
#endif
