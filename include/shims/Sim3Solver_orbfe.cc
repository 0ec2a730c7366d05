/*
 * Sim3Solver_orbfe.cc (shim) -- ORB_SLAM2::Sim3Solver (include/Sim3Solver.h) implemented on liborbfe.so.
 * Compile it INSTEAD of src/Sim3Solver.cc; include/Sim3Solver.h, KeyFrame and MapPoint stay the reference's own.
 *
 * The constructor flattens the two keyframes as the reference's does (Sim3Solver.cc:43-111): for every i1 with a match, the map
 * points' world positions and the keypoints mvKeysUn[GetIndexInKeyFrame] of both sides go to arrays indexed by i1, and match12[i1] =
 * i1 for a correspondence the reference keeps, -1 otherwise.  The class declares no member for flat arrays, so they are kept in the
 * cv::Mat vectors it does declare (mvX3Dc1 / mvX3Dc2: world points, pose, keypoints; mvP1im1: match12) -- a snapshot taken at
 * construction, as the reference's mvX3Dc* are.  iterate(n) draws 3 * min(n, remaining) words with rand(), which is what
 * DUtils::Random::RandomInt draws from, and makes ONE orbfe_sim3_solve call for the window, carrying mnIterations and mnBestInliers.
 *
 * Deviations: (1) the reference stops drawing at the iteration that succeeds; the shim has drawn the whole window, so after a
 * success inside a window the process's rand() state is up to 3 * (n - 1) draws further on.  (2) One level table serves both
 * sides (the library takes one): keyframes with different mvLevelSigma2 are refused.  Library errors are thrown as
 * std::runtime_error.
 */
#include "Sim3Solver.h"

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>

#include "KeyFrame.h"
#include "orbfe_shim.h"

using namespace std;

namespace ORB_SLAM2
{

using namespace orbfe_shim;

namespace
{

// [R | t] of a keyframe, 3 x 4
cv::Mat pose_of(KeyFrame* pKF)
{
    cv::Mat T(3, 4, CV_32F);
    pose34(pKF->GetRotation(), pKF->GetTranslation(), T.ptr<float>());
    return T;
}

enum { X3DW = 0, POSE = 1, KEYS = 2 };   // the slots of mvX3Dc1 / mvX3Dc2

} // namespace

Sim3Solver::Sim3Solver(KeyFrame* pKF1, KeyFrame* pKF2, const vector<MapPoint*>& vpMatched12, const bool bFixScale)
    : mnIterations(0), mnBestInliers(0), mbFixScale(bFixScale)
{
    mpKF1 = pKF1;
    mpKF2 = pKF2;
    if (pKF1->mvLevelSigma2 != pKF2->mvLevelSigma2) throw std::runtime_error("Sim3Solver (orbfe): the keyframes' level tables differ");

    vector<MapPoint*> vpKeyFrameMP1 = pKF1->GetMapPointMatches();
    mN1 = vpMatched12.size();
    mvpMatches12 = vpMatched12;

    const int n = mN1 > 0 ? mN1 : 1;
    mvX3Dc1.assign(3, cv::Mat());
    mvX3Dc2.assign(3, cv::Mat());
    mvX3Dc1[X3DW].create(n, 3, CV_32F); mvX3Dc2[X3DW].create(n, 3, CV_32F);
    mvX3Dc1[KEYS].create(n, (int)sizeof(orbfe_keypoint), CV_8U); mvX3Dc2[KEYS].create(n, (int)sizeof(orbfe_keypoint), CV_8U);
    mvX3Dc1[POSE] = pose_of(pKF1);
    mvX3Dc2[POSE] = pose_of(pKF2);
    mvP1im1.assign(1, cv::Mat());
    mvP1im1[0].create(n, (int)sizeof(int32_t), CV_8U);
    memset(mvX3Dc1[X3DW].data, 0, (size_t)n * 12); memset(mvX3Dc2[X3DW].data, 0, (size_t)n * 12);
    memset(mvX3Dc1[KEYS].data, 0, (size_t)n * sizeof(orbfe_keypoint)); memset(mvX3Dc2[KEYS].data, 0, (size_t)n * sizeof(orbfe_keypoint));
    int32_t* match12 = reinterpret_cast<int32_t*>(mvP1im1[0].data);

    mvnIndices1.clear();
    mvAllIndices.clear();
    size_t idx = 0;
    for (int i1 = 0; i1 < mN1; i1++) {
        match12[i1] = -1;
        if (!vpMatched12[i1]) continue;
        MapPoint* pMP1 = vpKeyFrameMP1[i1];
        MapPoint* pMP2 = vpMatched12[i1];
        if (!pMP1) continue;
        if (pMP1->isBad() || pMP2->isBad()) continue;
        const int indexKF1 = pMP1->GetIndexInKeyFrame(pKF1);
        const int indexKF2 = pMP2->GetIndexInKeyFrame(pKF2);
        if (indexKF1 < 0 || indexKF2 < 0) continue;
        memcpy(mvX3Dc1[KEYS].ptr(i1), &pKF1->mvKeysUn[indexKF1], sizeof(orbfe_keypoint));
        memcpy(mvX3Dc2[KEYS].ptr(i1), &pKF2->mvKeysUn[indexKF2], sizeof(orbfe_keypoint));
        point3(pMP1->GetWorldPos(), mvX3Dc1[X3DW].ptr<float>(i1));
        point3(pMP2->GetWorldPos(), mvX3Dc2[X3DW].ptr<float>(i1));
        match12[i1] = i1;
        mvpMapPoints1.push_back(pMP1);
        mvpMapPoints2.push_back(pMP2);
        mvnIndices1.push_back(i1);
        mvAllIndices.push_back(idx);
        idx++;
    }
    mK1 = pKF1->mK;
    mK2 = pKF2->mK;
    SetRansacParameters();
}

void Sim3Solver::SetRansacParameters(double probability, int minInliers, int maxIterations)
{
    mRansacProb = probability;
    mRansacMinInliers = minInliers;
    mRansacMaxIts = maxIterations;
    N = mvpMapPoints1.size();
    mvbInliersi.resize(N);
    // as the library counts (Sim3Solver.cc:125-135; a count that is not finite or below 1 is 1)
    int nIterations = 1;
    if (N > 0 && mRansacMinInliers != N) {
        const float epsilon = (float)mRansacMinInliers / N;
        const double nit = ceil(log(1 - mRansacProb) / log(1 - pow(epsilon, 3)));
        nIterations = nit >= (double)mRansacMaxIts ? mRansacMaxIts : nit >= 1 ? (int)nit : 1;
    }
    mRansacMaxIts = max(1, min(nIterations, mRansacMaxIts));
    mnIterations = 0;
}

cv::Mat Sim3Solver::iterate(int nIterations, bool& bNoMore, vector<bool>& vbInliers, int& nInliers)
{
    bNoMore = false;
    vbInliers = vector<bool>(mN1, false);
    nInliers = 0;
    if (N < mRansacMinInliers) {
        bNoMore = true;
        return cv::Mat();
    }
    const int n = min(nIterations, mRansacMaxIts - mnIterations);
    if (n <= 0) {
        if (mnIterations >= mRansacMaxIts) bNoMore = true;
        return cv::Mat();
    }
    vector<int32_t> words((size_t)n * 3);
    if (N >= 3)   // (fewer: the library reads no word and reports no_more)
        for (size_t i = 0; i < words.size(); i++) words[i] = rand();

    float K1[4], K2[4];
    intrinsics(mK1, K1);
    intrinsics(mK2, K2);
    const vector<float>& ls2 = mpKF1->mvLevelSigma2;
    orbfe_sim3_result res;
    vector<uint8_t> inl((size_t)mN1 + 1);
    check(orbfe_sim3_solve(reinterpret_cast<const orbfe_keypoint*>(mvX3Dc1[KEYS].data), mN1, mvX3Dc1[X3DW].ptr<float>(), NULL,
                           mvX3Dc1[POSE].ptr<float>(), K1, reinterpret_cast<const orbfe_keypoint*>(mvX3Dc2[KEYS].data), mN1,
                           mvX3Dc2[X3DW].ptr<float>(), NULL, mvX3Dc2[POSE].ptr<float>(), K2,
                           reinterpret_cast<const int32_t*>(mvP1im1[0].data), ls2.data(), (int)ls2.size(), mbFixScale ? 1 : 0, mRansacProb,
                           mRansacMinInliers, mRansacMaxIts, mnIterations, n, mnBestInliers, words.data(), &res, inl.data(), 0));
    if (res.best >= 0) {
        mnBestInliers = res.best_inliers;
        mBestT12 = mat32(4, 4, res.T12);
        mBestRotation = mat32(3, 3, res.R12);
        mBestTranslation = mat32(3, 1, res.t12);
        mBestScale = res.s12;
    }
    if (res.found >= 0) {
        mnIterations = res.found + 1;
        nInliers = res.n_inliers;
        mvbBestInliers.assign(N, false);
        for (int i = 0; i < N; i++) mvbBestInliers[i] = inl[mvnIndices1[i]] != 0;
        for (int i = 0; i < mN1; i++) vbInliers[i] = inl[i] != 0;
        return mBestT12;
    }
    mnIterations += n;
    if (res.no_more || mnIterations >= mRansacMaxIts) bNoMore = true;
    return cv::Mat();
}

cv::Mat Sim3Solver::find(vector<bool>& vbInliers12, int& nInliers)
{
    bool bFlag;
    return iterate(mRansacMaxIts, bFlag, vbInliers12, nInliers);
}

cv::Mat Sim3Solver::GetEstimatedRotation()
{
    return mBestRotation.clone();
}

cv::Mat Sim3Solver::GetEstimatedTranslation()
{
    return mBestTranslation.clone();
}

float Sim3Solver::GetEstimatedScale()
{
    return mBestScale;
}

} // namespace ORB_SLAM2
