// TEST INFRASTRUCTURE ONLY -- drives include/shims/Sim3Solver_orbfe.cc the way LoopClosing::ComputeSim3 does (one solver per loop
// candidate, SetRansacParameters(0.99, 20, 300), then iterate(5, ...) on every candidate in turn until each has no more), against
// the mock headers of tests/mock_orbslam/, and dumps every call's results as raw arrays for
// tests/test_sim3_shim_gpu.py.  A candidate that returns a transform stays in the round (the case of an OptimizeSim3 that rejects it).
// The shim draws its words with rand().  The driver defines rand() itself (a 64-bit LCG seeded from the command line), so that the
// shim's draws are the driver's alone -- the C library's rand() state is shared with every library in the process, and the GPU
// runtime draws from it while it starts up -- and dumps every value drawn, in order, for the test to feed to the C ABI.
//   sim3_shim_driver <in prefix> <out prefix> <nsolvers> <seed>
//   inputs per solver j: <in>_<j>_kps1 _kps2 (28-byte keypoints), _x1 _x2 (n x 3 floats), _v1 _v2 (bytes), _m12 (int32), _T1 _T2
//   (12 floats), _K (4 floats), _ls2 (floats), _fix (1 int32)
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <string>
#include <vector>

#include "Sim3Solver.h"
#include "shim_driver_io.hpp"

using namespace ORB_SLAM2;

static unsigned long long g_rand_state = 1;
static std::vector<int> g_drawn;
// hidden: not in the executable's dynamic symbol table, so the shared libraries of the process keep the C library's rand()
extern "C" __attribute__((visibility("hidden"))) int rand(void) noexcept
{
    g_rand_state = g_rand_state * 6364136223846793005ULL + 1442695040888963407ULL;
    const int v = (int)((g_rand_state >> 33) & 0x7fffffffULL);   // 0 .. RAND_MAX
    g_drawn.push_back(v);
    return v;
}

struct Side {
    KeyFrame kf;
    std::vector<std::unique_ptr<MapPoint>> points;
};

static void fill(Side& s, const std::string& pre, const char* k)
{
    s.kf.mvKeysUn = load<cv::KeyPoint>(pre + "_kps" + k + ".bin");
    const std::vector<float> x = load<float>(pre + "_x" + k + ".bin"), T = load<float>(pre + "_T" + k + ".bin"), K4 = load<float>(pre + "_K.bin");
    const std::vector<unsigned char> v = load<unsigned char>(pre + "_v" + k + ".bin");
    s.kf.mvLevelSigma2 = load<float>(pre + "_ls2.bin");
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
    if (argc != 5) return 2;
    const std::string in = argv[1], out = argv[2];
    const int ns = atoi(argv[3]);
    g_rand_state = (unsigned long long)atoll(argv[4]);
    std::vector<int> rec_i;
    std::vector<float> rec_f;
    std::vector<unsigned char> rec_inl;
    try {
        std::vector<std::unique_ptr<Side>> s1, s2;
        std::vector<std::unique_ptr<Sim3Solver>> solvers;
        for (int j = 0; j < ns; j++) {
            const std::string pre = in + "_" + std::to_string(j);
            s1.emplace_back(new Side); s2.emplace_back(new Side);
            fill(*s1[j], pre, "1");
            fill(*s2[j], pre, "2");
            const std::vector<int> m12 = load<int>(pre + "_m12.bin");
            std::vector<MapPoint*> matched(m12.size(), nullptr);
            for (size_t i = 0; i < m12.size(); i++)
                if (m12[i] >= 0) matched[i] = s2[j]->kf.mvpMapPoints[m12[i]];
            solvers.emplace_back(new Sim3Solver(&s1[j]->kf, &s2[j]->kf, matched, load<int>(pre + "_fix.bin")[0] != 0));
            solvers[j]->SetRansacParameters(0.99, 20, 300);
        }
        std::vector<bool> discarded(ns, false);
        int alive = ns;
        while (alive > 0) {
            for (int j = 0; j < ns; j++) {
                if (discarded[j]) continue;
                int nInliers;
                bool bNoMore;
                std::vector<bool> vbInliers;
                cv::Mat Scm = solvers[j]->iterate(5, bNoMore, vbInliers, nInliers);
                if (bNoMore) { discarded[j] = true; alive--; }
                rec_i.push_back(j); rec_i.push_back(Scm.empty() ? 0 : 1); rec_i.push_back(bNoMore ? 1 : 0); rec_i.push_back(nInliers);
                rec_i.push_back((int)vbInliers.size());
                float f[29] = {0};
                if (!Scm.empty()) {
                    const cv::Mat R = solvers[j]->GetEstimatedRotation(), t = solvers[j]->GetEstimatedTranslation();
                    for (int i = 0; i < 16; i++) f[i] = Scm.at<float>(i / 4, i % 4);
                    for (int i = 0; i < 9; i++) f[16 + i] = R.at<float>(i / 3, i % 3);
                    for (int i = 0; i < 3; i++) f[25 + i] = t.at<float>(i);
                    f[28] = solvers[j]->GetEstimatedScale();
                }
                rec_f.insert(rec_f.end(), f, f + 29);
                for (bool b : vbInliers) rec_inl.push_back(b ? 1 : 0);
            }
        }
    } catch (const std::exception& e) {
        fprintf(stderr, "%s\n", e.what());
        return 3;
    }
    dump(out + "_i.bin", rec_i);
    dump(out + "_f.bin", rec_f);
    dump(out + "_inl.bin", rec_inl);
    dump(out + "_words.bin", g_drawn);
    return 0;
}
