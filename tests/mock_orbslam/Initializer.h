// TEST INFRASTRUCTURE ONLY -- the declaration of ORB_SLAM2::Initializer (include/Initializer.h of the reference) that
// include/shims/Initializer_orbfe.cc implements: the public interface with the reference's signatures and the members the shim
// fills.
#ifndef MOCK_INITIALIZER_H
#define MOCK_INITIALIZER_H
#include <utility>
#include <vector>
#include <opencv2/core/core.hpp>
#include "Frame.h"

namespace ORB_SLAM2 {
using std::vector;
class Initializer {
    typedef std::pair<int, int> Match;
public:
    Initializer(const Frame& ReferenceFrame, float sigma = 1.0, int iterations = 200);
    bool Initialize(const Frame& CurrentFrame, const vector<int>& vMatches12, cv::Mat& R21, cv::Mat& t21,
                    vector<cv::Point3f>& vP3D, vector<bool>& vbTriangulated);
    bool InitializeUseAruco(const Frame& CurrentFrame, const vector<int>& vMatches12, vector<cv::Mat>& R21, vector<cv::Mat>& t21,
                            vector<cv::Point3f>& vP3D, vector<bool>& vbTriangulated, int& bestIdA);
private:
    vector<cv::KeyPoint> mvKeys1, mvKeys2;
    vector<Match> mvMatches12;
    vector<bool> mvbMatched1;
    cv::Mat mK;
    float mSigma, mSigma2;
    int mMaxIterations;
    vector<vector<size_t> > mvSets;
};
}
#endif
