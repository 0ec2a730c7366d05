/*
 * Initializer_orbfe.cc (shim) -- ORB_SLAM2::Initializer (include/Initializer.h) implemented on liborbfe.so.
 * Compile it INSTEAD of src/Initializer.cc; include/Initializer.h and Frame stay the reference's own.
 *
 * The constructor keeps what the reference's keeps (mK, frame 1's mvKeysUn, sigma, iterations).  Initialize() draws the
 * iterations * 8 rand() words the reference would draw (after DUtils::Random::SeedRandOnce(0), Initializer.cc:80-97) and hands
 * them to orbfe_initialize, which does the rest of Initialize() on the GPU: the process-global rand() state advances exactly as with
 * the reference.  InitializeUseAruco() is one orbfe_initialize_check_poses call.  Library errors are thrown as std::runtime_error.
 */
#include "Initializer.h"

#include <cstdint>
#include <cstdlib>

#include "Thirdparty/DBoW2/DUtils/Random.h"
#include "orbfe_shim.h"

using namespace std;

namespace ORB_SLAM2
{

using namespace orbfe_shim;

namespace
{

// vMatches12 as the library takes it: one entry per frame-1 keypoint (the reference indexes it by them, Initializer.cc:55-63)
vector<int32_t> matches_of(const vector<int>& vMatches12, size_t n1)
{
    vector<int32_t> m(n1, -1);
    for (size_t i = 0; i < n1 && i < vMatches12.size(); i++) m[i] = vMatches12[i];
    return m;
}

void points_out(const vector<float>& p3d, const vector<uint8_t>& tri, vector<cv::Point3f>& vP3D, vector<bool>& vbTriangulated)
{
    const size_t n = tri.size();
    vP3D.resize(n);
    vbTriangulated.assign(n, false);
    for (size_t i = 0; i < n; i++) {
        vP3D[i] = cv::Point3f(p3d[3 * i], p3d[3 * i + 1], p3d[3 * i + 2]);
        vbTriangulated[i] = tri[i] != 0;
    }
}

} // namespace

Initializer::Initializer(const Frame& ReferenceFrame, float sigma, int iterations)
{
    mK = ReferenceFrame.mK.clone();
    mvKeys1 = ReferenceFrame.mvKeysUn;
    mSigma = sigma;
    mSigma2 = sigma * sigma;
    mMaxIterations = iterations;
}

bool Initializer::Initialize(const Frame& CurrentFrame, const vector<int>& vMatches12, cv::Mat& R21, cv::Mat& t21,
                             vector<cv::Point3f>& vP3D, vector<bool>& vbTriangulated)
{
    mvKeys2 = CurrentFrame.mvKeysUn;
    const size_t n1 = mvKeys1.size();
    const vector<int32_t> m12 = matches_of(vMatches12, n1);

    DUtils::Random::SeedRandOnce(0);
    vector<int32_t> words((size_t)mMaxIterations * 8);
    for (size_t i = 0; i < words.size(); i++) words[i] = rand();

    float K4[4];
    intrinsics(mK, K4);
    orbfe_init_result res;
    vector<float> p3d(n1 * 3 + 3);
    vector<uint8_t> tri(n1 + 1);
    check(orbfe_initialize(keys(mvKeys1), (int)n1, keys(mvKeys2), (int)mvKeys2.size(), m12.data(), K4, mSigma, mMaxIterations,
                           words.data(), &res, p3d.data(), tri.data(), 0));
    if (res.initialized) {
        R21 = mat32(3, 3, res.R21);
        t21 = mat32(3, 1, res.t21);
        tri.resize(n1);
        points_out(p3d, tri, vP3D, vbTriangulated);
        return true;
    }
    // ReconstructF empties R21 / t21 once it has decomposed E (Initializer.cc:562-563); ReconstructH leaves them as they were
    if (res.model == 1 && res.best_f >= 0) {
        R21 = cv::Mat();
        t21 = cv::Mat();
    }
    return false;
}

bool Initializer::InitializeUseAruco(const Frame& CurrentFrame, const vector<int>& vMatches12, vector<cv::Mat>& R21,
                                     vector<cv::Mat>& t21, vector<cv::Point3f>& vP3D, vector<bool>& vbTriangulated, int& bestIdA)
{
    if (R21.size() == 0) return false;
    mvKeys2 = CurrentFrame.mvKeysUn;
    const size_t n1 = mvKeys1.size();
    const vector<int32_t> m12 = matches_of(vMatches12, n1);
    vector<float> poses(R21.size() * 12);
    for (size_t i = 0; i < R21.size(); i++) {
        for (int r = 0; r < 3; r++)
            for (int c = 0; c < 3; c++) poses[i * 12 + r * 3 + c] = R21[i].at<float>(r, c);
        for (int r = 0; r < 3; r++) poses[i * 12 + 9 + r] = t21[i].at<float>(r);
    }
    float K4[4];
    intrinsics(mK, K4);
    orbfe_init_result res;
    vector<float> p3d(n1 * 3 + 3);
    vector<uint8_t> tri(n1 + 1);
    check(orbfe_initialize_check_poses(keys(mvKeys1), (int)n1, keys(mvKeys2), (int)mvKeys2.size(), m12.data(), K4, mSigma,
                                       poses.data(), (int)R21.size(), &res, p3d.data(), tri.data(), 0));
    if (res.best_h >= 0) {   // the reference assigns these inside its loop, also when it then returns false
        tri.resize(n1);
        points_out(p3d, tri, vP3D, vbTriangulated);
        bestIdA = res.best_h;
    }
    return res.initialized != 0;
}

} // namespace ORB_SLAM2
