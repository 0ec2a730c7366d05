// TEST INFRASTRUCTURE ONLY -- what the KeyFrameDatabase shim needs of DBoW2::BowVector (Thirdparty/DBoW2/DBoW2/BowVector.h): a map
// from word id to value.
#ifndef MOCK_BOWVECTOR_H
#define MOCK_BOWVECTOR_H
#include <map>
namespace DBoW2 {
typedef unsigned int WordId;
typedef double WordValue;
class BowVector : public std::map<WordId, WordValue> {};
}
#endif
