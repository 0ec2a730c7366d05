// TEST INFRASTRUCTURE ONLY -- drives include/shims/Optimizer_sim3_orbfe.cc the way LoopClosing::ComputeSim3 does (g2oS12 built from a
// float rotation, translation and scale; OptimizeSim3(pKF1, pKF2, vpMatches1, g2oS12, th2, bFixScale)) against the mock headers of
// tests/mock_orbslam/, and dumps the results as raw arrays for tests/test_sim3_opt_shim_gpu.py.
//   sim3_opt_shim_driver <in prefix> <out prefix>
//   inputs: <in>_kps1 _kps2 (28-byte keypoints), _x1 _x2 (n x 3 floats), _v1 _v2 (bytes), _m12 (int32), _T1 _T2 (12 floats), _K (4
//   floats), _is2 (floats), _sim (13 floats: s12, R12, t12), _par (2 floats: th2, fix_scale)
//   outputs: <out>_i (int32: the return value, then 1 per match still there), _d (8 doubles: s, q x y z w, t), _sim (13 floats: the
//   similarity as the shim hands it to the library)
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <string>
#include <vector>

#include "Optimizer.h"
#include "shim_driver_io.hpp"

using namespace ORB_SLAM2;

struct Side {
    KeyFrame kf;
    std::vector<std::unique_ptr<MapPoint>> points;
};

static void fill(Side& s, const std::string& pre, const char* k)
{
    s.kf.mvKeysUn = load<cv::KeyPoint>(pre + "_kps" + k + ".bin");
    const std::vector<float> x = load<float>(pre + "_x" + k + ".bin"), T = load<float>(pre + "_T" + k + ".bin"), K4 = load<float>(pre + "_K.bin");
    const std::vector<unsigned char> v = load<unsigned char>(pre + "_v" + k + ".bin");
    s.kf.mvInvLevelSigma2 = load<float>(pre + "_is2.bin");
    s.kf.mK = cv::Mat(3, 3, CV_32F);
    const float kk[9] = {K4[0], 0, K4[2], 0, K4[1], K4[3], 0, 0, 1};
    for (int i = 0; i < 9; i++) s.kf.mK.at<float>(i / 3, i % 3) = kk[i];
    s.kf.Rcw = cv::Mat(3, 3, CV_32F);
    s.kf.tcw = cv::Mat(3, 1, CV_32F);
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) s.kf.Rcw.at<float>(r, c) = T[4 * r + c];
        s.kf.tcw.at<float>(r) = T[4 * r + 3];
    }
    for (size_t i = 0; i < s.kf.mvKeysUn.size(); i++) {
        std::unique_ptr<MapPoint> p(new MapPoint);
        p->mWorldPos = cv::Mat(3, 1, CV_32F);
        for (int c = 0; c < 3; c++) p->mWorldPos.at<float>(c) = x[3 * i + c];
        p->mbBad = v[i] == 0;
        p->mObservations[&s.kf] = i;
        s.kf.mvpMapPoints.push_back(p.get());
        s.points.push_back(std::move(p));
    }
}

int main(int argc, char** argv)
{
    if (argc != 3) return 2;
    const std::string in = argv[1], out = argv[2];
    std::vector<int> rec_i;
    std::vector<double> rec_d;
    std::vector<float> rec_sim;
    try {
        Side s1, s2;
        fill(s1, in, "1");
        fill(s2, in, "2");
        const std::vector<int> m12 = load<int>(in + "_m12.bin");
        std::vector<MapPoint*> matched(m12.size(), nullptr);
        for (size_t i = 0; i < m12.size(); i++)
            if (m12[i] >= 0) matched[i] = s2.kf.mvpMapPoints[m12[i]];
        const std::vector<float> sim = load<float>(in + "_sim.bin"), par = load<float>(in + "_par.bin");
        Eigen::Matrix3d R;
        for (int i = 0; i < 9; i++) R(i / 3, i % 3) = sim[1 + i];
        g2o::Sim3 S(R, Eigen::Vector3d(sim[10], sim[11], sim[12]), sim[0]);
        // what the shim will round to float
        const Eigen::Matrix3d Rq = S.rotation().toRotationMatrix();
        rec_sim.push_back((float)S.scale());
        for (int i = 0; i < 9; i++) rec_sim.push_back((float)Rq(i / 3, i % 3));
        for (int i = 0; i < 3; i++) rec_sim.push_back((float)S.translation()[i]);
        rec_i.push_back(Optimizer::OptimizeSim3(&s1.kf, &s2.kf, matched, S, par[0], par[1] != 0));
        for (MapPoint* p : matched) rec_i.push_back(p ? 1 : 0);
        rec_d.push_back(S.scale());
        rec_d.push_back(S.rotation().x()); rec_d.push_back(S.rotation().y()); rec_d.push_back(S.rotation().z()); rec_d.push_back(S.rotation().w());
        for (int i = 0; i < 3; i++) rec_d.push_back(S.translation()[i]);
    } catch (const std::exception& e) {
        fprintf(stderr, "%s\n", e.what());
        return 3;
    }
    dump(out + "_i.bin", rec_i);
    dump(out + "_d.bin", rec_d);
    dump(out + "_sim.bin", rec_sim);
    return 0;
}
