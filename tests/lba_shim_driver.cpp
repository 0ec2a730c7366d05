// TEST INFRASTRUCTURE ONLY -- drives include/shims/Optimizer_localba_orbfe.cc the way LocalMapping does, on the mock map that
// tests/lba_shim_map.py describes, against the mock headers of tests/mock_orbslam/, and dumps raw
// arrays for tests/test_lba_shim_cpu.py and tests/test_lba_shim_gpu.py.
//   lba_shim_driver collect <in prefix> <out prefix>            the collect step alone (no library call): the lists and the flat arrays
//   lba_shim_driver run <in prefix> <out prefix> <use> <stop>   Optimizer::LocalBundleAdjustment with Frame::mbUArucoIni = use and
//                                                               *pbStopFlag = stop, then the state of the map
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "Optimizer.h"
#include "Optimizer_localba_orbfe.h"
#include "shim_driver_io.hpp"

using namespace ORB_SLAM2;

int main(int argc, char** argv)
{
    if (argc < 4) return 2;
    const std::string mode = argv[1], in = argv[2], out = argv[3];
    const std::vector<int32_t> kf = load<int32_t>(in + "_kf.bin"), match = load<int32_t>(in + "_match.bin"), kfmk = load<int32_t>(in + "_kfmk.bin");
    const std::vector<int32_t> obs = load<int32_t>(in + "_obs.bin"), ma = load<int32_t>(in + "_ma.bin"), maobs = load<int32_t>(in + "_maobs.bin");
    const std::vector<int32_t> cur = load<int32_t>(in + "_cur.bin");
    const std::vector<float> kfT = load<float>(in + "_kfT.bin"), corners = load<float>(in + "_kfcorners.bin"), X = load<float>(in + "_X.bin");
    const std::vector<float> maT = load<float>(in + "_maT.bin"), cam = load<float>(in + "_cam.bin");
    const std::vector<cv::KeyPoint> kps = load<cv::KeyPoint>(in + "_kps.bin");
    const std::vector<uint8_t> mpbad = load<uint8_t>(in + "_mpbad.bin");
    const size_t nk = kf.size() / 4, np = mpbad.size(), nm = ma.size() / 2;
    std::vector<KeyFrame> kfs(nk);
    std::vector<MapPoint> mps(np);
    std::vector<MapAruco> mas(nm);
    for (size_t i = 0; i < np; i++) {
        mps[i].mnId = 100 + i;
        mps[i].mbBad = mpbad[i] != 0;
        mps[i].mWorldPos = cv::Mat(3, 1, CV_32F);
        for (int c = 0; c < 3; c++) mps[i].mWorldPos.at<float>(c) = X[3 * i + c];
    }
    for (size_t m = 0; m < nm; m++) {
        mas[m].mnArucoId = ma[2 * m];
        mas[m].mbBad = ma[2 * m + 1] != 0;
        mas[m].mLength = cam[4];
        mas[m].mTwm = cv::Mat(4, 4, CV_32F);
        for (int i = 0; i < 16; i++) mas[m].mTwm.at<float>(i / 4, i % 4) = i < 12 ? maT[12 * m + i] : (i == 15 ? 1.f : 0.f);
    }
    size_t kp0 = 0, mk0 = 0;
    for (size_t k = 0; k < nk; k++) {
        KeyFrame& F = kfs[k];
        F.mnId = (long unsigned)kf[4 * k];
        F.mbBad = kf[4 * k + 1] != 0;
        const size_t n = (size_t)kf[4 * k + 2], nmk = (size_t)kf[4 * k + 3];
        F.mvKeysUn.assign(kps.begin() + (long)kp0, kps.begin() + (long)(kp0 + n));
        F.mvuRight.assign(n, -1.f);
        F.mvpMapPoints.resize(n);
        for (size_t i = 0; i < n; i++) F.mvpMapPoints[i] = &mps[(size_t)match[kp0 + i]];
        kp0 += n;
        F.mvInvLevelSigma2.assign(cam.begin() + 5, cam.end());
        F.fx = cam[0]; F.fy = cam[1]; F.cx = cam[2]; F.cy = cam[3];
        F.Tcw = cv::Mat(4, 4, CV_32F);
        for (int i = 0; i < 16; i++) F.Tcw.at<float>(i / 4, i % 4) = i < 12 ? kfT[12 * k + i] : (i == 15 ? 1.f : 0.f);
        F.NA = (int)nmk;
        for (size_t j = 0; j < nmk; j++) {
            F.mvpMapArucos.push_back(&mas[(size_t)kfmk[2 * (mk0 + j)]]);
            F.mvbOldAruco.push_back(kfmk[2 * (mk0 + j) + 1] != 0);
            for (int c = 0; c < 4; c++) F.mvArucoUn.push_back(cv::Point2f(corners[8 * (mk0 + j) + 2 * c], corners[8 * (mk0 + j) + 2 * c + 1]));
        }
        mk0 += nmk;
    }
    for (size_t o = 0; o < obs.size() / 3; o++) mps[(size_t)obs[3 * o]].mObservations[&kfs[(size_t)obs[3 * o + 1]]] = (size_t)obs[3 * o + 2];
    for (size_t o = 0; o < maobs.size() / 3; o++) mas[(size_t)maobs[3 * o]].mObservations[&kfs[(size_t)maobs[3 * o + 1]]] = (size_t)maobs[3 * o + 2];
    KeyFrame* pKF = &kfs[(size_t)cur[0]];
    for (size_t i = 1; i < cur.size(); i++) pKF->mvpOrderedConnectedKeyFrames.push_back(&kfs[(size_t)cur[i]]);
    Map map;

    if (mode == "collect") {
        orbfe_localba::Problem pb;
        orbfe_localba::Collect(pKF, &map, pb);
        std::vector<int32_t> vk, vp, vm, marks;
        for (KeyFrame* p : pb.vpKeyFrames) vk.push_back((int32_t)(p - kfs.data()));
        vk.push_back((int32_t)pb.nLocal);
        for (MapPoint* p : pb.vpMapPoints) vp.push_back((int32_t)(p - mps.data()));
        for (MapAruco* p : pb.vpMapArucos) vm.push_back((int32_t)(p - mas.data()));
        for (KeyFrame& F : kfs) {
            marks.push_back((int32_t)F.mnBALocalForKF);
            marks.push_back((int32_t)F.mnBAFixedForKF);
        }
        dump(out + "_vk.bin", vk); dump(out + "_vp.bin", vp); dump(out + "_vm.bin", vm); dump(out + "_marks.bin", marks);
        dump(out + "_Tcw.bin", pb.Tcw); dump(out + "_fixed.bin", pb.kf_fixed); dump(out + "_x.bin", pb.x3Dw); dump(out + "_off.bin", pb.obs_offset);
        dump(out + "_okf.bin", pb.obs_kf); dump(out + "_oxy.bin", pb.obs_xy); dump(out + "_ooct.bin", pb.obs_octave); dump(out + "_Twm.bin", pb.Twm);
        dump(out + "_mloc.bin", pb.marker_local); dump(out + "_moff.bin", pb.mobs_offset); dump(out + "_mkf.bin", pb.mobs_kf);
        dump(out + "_mcor.bin", pb.mobs_corners); dump(out + "_K.bin", pb.K4, 4); dump(out + "_sig.bin", pb.inv_level_sigma2);
        // a stereo observation throws
        int32_t threw = 0;
        for (MapPoint& p : mps) p.mnBALocalForKF = 0;   // a new call of a new keyframe, as far as the marks go
        pKF->mvuRight[0] = 12.f;
        try {
            orbfe_localba::Collect(pKF, &map, pb);
        } catch (const std::runtime_error&) {
            threw = 1;
        }
        dump(out + "_threw.bin", &threw, 1);
        return 0;
    }
    if (argc != 6) return 2;
    Frame::mbUArucoIni = atoi(argv[4]) != 0;
    bool stop = atoi(argv[5]) != 0;
    Optimizer::LocalBundleAdjustment(pKF, &stop, &map);
    std::vector<float> T, P, M;
    std::vector<int32_t> counts, present;
    for (KeyFrame& F : kfs) {
        for (int i = 0; i < 16; i++) T.push_back(F.Tcw.at<float>(i / 4, i % 4));
        counts.push_back(F.nSetPose);
    }
    for (MapPoint& p : mps) {
        for (int c = 0; c < 3; c++) P.push_back(p.mWorldPos.at<float>(c));
        counts.push_back(p.nUpdates);
    }
    for (MapAruco& a : mas)
        for (int i = 0; i < 12; i++) M.push_back(a.mTwm.at<float>(i / 4, i % 4));
    for (size_t o = 0; o < obs.size() / 3; o++) {
        MapPoint& p = mps[(size_t)obs[3 * o]];
        KeyFrame& F = kfs[(size_t)obs[3 * o + 1]];
        present.push_back((p.mObservations.count(&F) ? 1 : 0) + (F.mvpMapPoints[(size_t)obs[3 * o + 2]] == &p ? 2 : 0));
    }
    dump(out + "_T.bin", T); dump(out + "_P.bin", P); dump(out + "_M.bin", M); dump(out + "_counts.bin", counts); dump(out + "_present.bin", present);
    return 0;
}
