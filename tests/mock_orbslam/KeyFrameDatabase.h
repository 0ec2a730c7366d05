// TEST INFRASTRUCTURE ONLY -- the class of include/KeyFrameDatabase.h as its users see it: the constructor, add / erase / clear and
// the two candidate queries, with the members the reference keeps.
#ifndef MOCK_KEYFRAMEDATABASE_H
#define MOCK_KEYFRAMEDATABASE_H
#include <list>
#include <mutex>
#include <set>
#include <vector>
#include "Frame.h"
#include "KeyFrame.h"
#include "ORBVocabulary.h"
namespace ORB_SLAM2 {
class KeyFrameDatabase {
public:
    KeyFrameDatabase(const ORBVocabulary& voc);
    void add(KeyFrame* pKF);
    void erase(KeyFrame* pKF);
    void clear();
    std::vector<KeyFrame*> DetectLoopCandidates(KeyFrame* pKF, float minScore);
    std::vector<KeyFrame*> DetectRelocalizationCandidates(Frame* F);
protected:
    const ORBVocabulary* mpVoc;
    std::vector<std::list<KeyFrame*> > mvInvertedFile;
    std::mutex mMutex;
};
}
#endif
