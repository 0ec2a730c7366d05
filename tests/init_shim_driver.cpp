// TEST INFRASTRUCTURE ONLY -- drives include/shims/Initializer_orbfe.cc the way Tracking::MonocularInitialization does
// (Initializer(mInitialFrame, 1.0, 200), then Initialize / InitializeUseAruco with the current frame), against the mock headers
// of tests/mock_orbslam/, and dumps results as raw arrays for tests/test_initializer_shim_gpu.py.
//   init_shim_driver <in prefix> <out prefix>      inputs: _kps1 _kps2 (28-byte keypoints), _m12 (int32), _K (4 floats),
//                                                   _poses (npose x 12 floats)
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "Initializer.h"
#include "shim_driver_io.hpp"

using namespace ORB_SLAM2;

int main(int argc, char** argv)
{
    if (argc != 3) return 2;
    const std::string in = argv[1], out = argv[2];
    Frame F1, F2;
    F1.mvKeysUn = load<cv::KeyPoint>(in + "_kps1.bin");
    F2.mvKeysUn = load<cv::KeyPoint>(in + "_kps2.bin");
    const std::vector<int> m12 = load<int>(in + "_m12.bin");
    const std::vector<float> K4 = load<float>(in + "_K.bin"), poses = load<float>(in + "_poses.bin");
    cv::Mat K(3, 3, CV_32F);
    const float k[9] = {K4[0], 0, K4[2], 0, K4[1], K4[3], 0, 0, 1};
    for (int i = 0; i < 9; i++) K.at<float>(i / 3, i % 3) = k[i];
    F1.mK = K;
    F2.mK = K;
    try {
        Initializer ini(F1, 1.0, 200);
        cv::Mat R21, t21;
        std::vector<cv::Point3f> vP3D;
        std::vector<bool> vbTri;
        const int ok = ini.Initialize(F2, m12, R21, t21, vP3D, vbTri);
        std::vector<float> Rt(12, 0.f);
        if (ok)
            for (int i = 0; i < 9; i++) Rt[i] = R21.at<float>(i / 3, i % 3), Rt[9 + i % 3] = t21.at<float>(i % 3);
        std::vector<unsigned char> tri(vbTri.begin(), vbTri.end());
        dump(out + "_ok.bin", &ok, 1);
        dump(out + "_Rt.bin", Rt.data(), Rt.size());
        dump(out + "_p3d.bin", (const float*)vP3D.data(), vP3D.size() * 3);
        dump(out + "_tri.bin", tri.data(), tri.size());

        std::vector<cv::Mat> Rs, ts;
        for (size_t i = 0; i + 12 <= poses.size(); i += 12) {
            cv::Mat R(3, 3, CV_32F), t(3, 1, CV_32F);
            for (int j = 0; j < 9; j++) R.at<float>(j / 3, j % 3) = poses[i + j];
            for (int j = 0; j < 3; j++) t.at<float>(j) = poses[i + 9 + j];
            Rs.push_back(R);
            ts.push_back(t);
        }
        std::vector<cv::Point3f> aP3D;
        std::vector<bool> aTri;
        int best = -1;
        const int aok = ini.InitializeUseAruco(F2, m12, Rs, ts, aP3D, aTri, best);
        std::vector<unsigned char> atri(aTri.begin(), aTri.end());
        const int ab[2] = {aok, best};
        dump(out + "_aruco.bin", ab, 2);
        dump(out + "_ap3d.bin", (const float*)aP3D.data(), aP3D.size() * 3);
        dump(out + "_atri.bin", atri.data(), atri.size());
    } catch (const std::exception& e) {
        fprintf(stderr, "%s\n", e.what());
        return 3;
    }
    return 0;
}
