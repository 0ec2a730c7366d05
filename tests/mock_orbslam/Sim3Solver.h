// TEST INFRASTRUCTURE ONLY -- the declaration of ORB_SLAM2::Sim3Solver (include/Sim3Solver.h of the reference) that
// include/shims/Sim3Solver_orbfe.cc implements: the public interface with the reference's signatures, and the members the shim
// uses, with the reference's names and types.
#ifndef MOCK_SIM3SOLVER_H
#define MOCK_SIM3SOLVER_H
#include <vector>
#include <opencv2/core/core.hpp>
#include "KeyFrame.h"

namespace ORB_SLAM2 {
class Sim3Solver {
public:
    Sim3Solver(KeyFrame* pKF1, KeyFrame* pKF2, const std::vector<MapPoint*>& vpMatched12, const bool bFixScale = true);
    void SetRansacParameters(double probability = 0.99, int minInliers = 6, int maxIterations = 300);
    cv::Mat find(std::vector<bool>& vbInliers12, int& nInliers);
    cv::Mat iterate(int nIterations, bool& bNoMore, std::vector<bool>& vbInliers, int& nInliers);
    cv::Mat GetEstimatedRotation();
    cv::Mat GetEstimatedTranslation();
    float GetEstimatedScale();

protected:
    KeyFrame *mpKF1, *mpKF2;
    std::vector<cv::Mat> mvX3Dc1, mvX3Dc2;
    std::vector<MapPoint*> mvpMapPoints1, mvpMapPoints2, mvpMatches12;
    std::vector<size_t> mvnIndices1;
    int N, mN1;
    std::vector<bool> mvbInliersi;
    int mnIterations;
    std::vector<bool> mvbBestInliers;
    int mnBestInliers;
    cv::Mat mBestT12, mBestRotation, mBestTranslation;
    float mBestScale;
    bool mbFixScale;
    std::vector<size_t> mvAllIndices;
    std::vector<cv::Mat> mvP1im1, mvP2im2;
    double mRansacProb;
    int mRansacMinInliers, mRansacMaxIts;
    cv::Mat mK1, mK2;
};
}
#endif
