// TEST INFRASTRUCTURE ONLY -- DUtils::Random::SeedRandOnce (Thirdparty/DBoW2/DUtils/Random.cpp:38-45 of the reference): srand(seed)
// the first time only.
#ifndef MOCK_DUTILS_RANDOM_H
#define MOCK_DUTILS_RANDOM_H
#include <cstdlib>
namespace DUtils {
class Random {
public:
    static void SeedRandOnce(int seed)
    {
        static bool seeded = false;
        if (!seeded) { srand(seed); seeded = true; }
    }
};
}
#endif
