// TEST INFRASTRUCTURE ONLY -- drives include/shims/Optimizer_pose_orbfe.cc the way Tracking does (one Frame with map points and
// mapped markers, Optimizer::PoseOptimizationByAruco), against the mock headers of tests/mock_orbslam/, and dumps the
// results as raw arrays for tests/test_pose_opt_shim_gpu.py.
//   pose_shim_driver <in prefix> <out prefix> <side>   inputs: _kps (28-byte keypoints), _has (uint8), _x (n x 3 floats),
//                                                       _sig (floats), _K (4 floats), _mk (128-byte marker records), _T (12 floats),
//                                                       _out (uint8: mvbOutlier before the call)
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "Frame.h"
#include "MapAruco.h"
#include "MapPoint.h"
#include "Optimizer.h"
#include "shim_driver_io.hpp"

using namespace ORB_SLAM2;

int main(int argc, char** argv)
{
    if (argc != 4) return 2;
    const std::string in = argv[1], out = argv[2];
    const double side = atof(argv[3]);
    Frame F;
    F.mvKeysUn = load<cv::KeyPoint>(in + "_kps.bin");
    F.N = (int)F.mvKeysUn.size();
    const std::vector<uint8_t> has = load<uint8_t>(in + "_has.bin"), out0 = load<uint8_t>(in + "_out.bin");
    const std::vector<float> X = load<float>(in + "_x.bin"), K = load<float>(in + "_K.bin"), T = load<float>(in + "_T.bin");
    F.mvInvLevelSigma2 = load<float>(in + "_sig.bin");
    const std::vector<float> mk = load<float>(in + "_mk.bin");   // 32 floats a marker: corners, Twm, local
    Frame::fx = K[0]; Frame::fy = K[1]; Frame::cx = K[2]; Frame::cy = K[3];
    std::vector<MapPoint> mps(F.N);
    F.mvpMapPoints.assign(F.N, nullptr);
    F.mvuRight.assign(F.N, -1.f);
    F.mvbOutlier.resize(F.N);
    for (int i = 0; i < F.N; i++) {
        F.mvbOutlier[i] = out0[i] != 0;
        if (!has[i]) continue;
        mps[i].mWorldPos = cv::Mat(3, 1, CV_32F);
        for (int k = 0; k < 3; k++) mps[i].mWorldPos.at<float>(k) = X[3 * i + k];
        F.mvpMapPoints[i] = &mps[i];
    }
    // the markers, plus an old one and a bad one that must be left out
    const int nm = (int)(mk.size() / 32);
    std::vector<MapAruco> mas(nm + 2);
    F.NA = nm + 2;
    Frame::mbUArucoIni = true;
    for (int m = 0; m < nm + 2; m++) {
        const float* r = mk.data() + 32 * (m % std::max(nm, 1));
        MapAruco& a = mas[m];
        a.mLength = side;
        a.mTwm = cv::Mat(4, 4, CV_32F);
        for (int i = 0; i < 16; i++) a.mTwm.at<float>(i / 4, i % 4) = i < 12 ? (nm ? r[8 + i] : 0.f) : (i == 15 ? 1.f : 0.f);
        for (int k = 0; k < 4; k++) F.mvArucoUn.push_back(cv::Point2f(nm ? r[2 * k] + (m >= nm ? 40.f : 0.f) : 0.f, nm ? r[2 * k + 1] : 0.f));
        F.mvpMapArucos.push_back(&a);
        F.mvbOldAruco.push_back(m == nm);
        F.mvbArucoGood.push_back(m != nm + 1);
    }
    F.mTcw = cv::Mat(4, 4, CV_32F);
    for (int i = 0; i < 16; i++) F.mTcw.at<float>(i / 4, i % 4) = i < 12 ? T[i] : (i == 15 ? 1.f : 0.f);
    const int ret = Optimizer::PoseOptimizationByAruco(&F);
    std::vector<uint8_t> o(F.N);
    for (int i = 0; i < F.N; i++) o[i] = F.mvbOutlier[i] ? 1 : 0;
    dump(out + "_T.bin", F.mTcw.ptr<float>(0), 16);
    dump(out + "_out.bin", o.data(), o.size());
    dump(out + "_ret.bin", &ret, 1);
    // PoseOptimization meets a stereo observation: it throws
    int threw = 0;
    if (F.N > 0) {
        F.mvuRight[0] = 10.f;
        F.mvpMapPoints[0] = &mps[0];
        mps[0].mWorldPos = cv::Mat(3, 1, CV_32F);
        try {
            Optimizer::PoseOptimization(&F);
        } catch (const std::runtime_error&) {
            threw = 1;
        }
    }
    dump(out + "_threw.bin", &threw, 1);
    return 0;
}
