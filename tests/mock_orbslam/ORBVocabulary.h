// TEST INFRASTRUCTURE ONLY -- what KeyFrameDatabase asks of ORBVocabulary (include/ORBVocabulary.h): the number of words and the
// score of two BowVectors, which the test supplies as a function.
#ifndef MOCK_ORBVOCABULARY_H
#define MOCK_ORBVOCABULARY_H
#include "Thirdparty/DBoW2/DBoW2/BowVector.h"
namespace ORB_SLAM2 {
class ORBVocabulary {
public:
    typedef double (*Scorer)(const DBoW2::BowVector&, const DBoW2::BowVector&);
    ORBVocabulary(unsigned int words, Scorer s) : mWords(words), mScorer(s) {}
    unsigned int size() const { return mWords; }
    double score(const DBoW2::BowVector& a, const DBoW2::BowVector& b) const { return mScorer(a, b); }
private:
    unsigned int mWords;
    Scorer mScorer;
};
}
#endif
