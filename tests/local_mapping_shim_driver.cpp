// TEST INFRASTRUCTURE ONLY -- drives include/shims/LocalMapping_orbfe.cc the way LocalMapping::CreateNewMapPoints does (the current
// keyframe and GetBestCovisibilityKeyFrames(20)) against the mock headers of tests/mock_orbslam/, and dumps the triples as raw arrays
// for tests/test_new_points_gpu.py.
//   local_mapping_shim_driver <in prefix> <out prefix>
//   inputs: <in>_nf (int32: keyframes, the current one first), _K (4 floats), _sf _sg (level tables), and per keyframe f: _kps<f>
//   (28-byte keypoints), _desc<f> (n x 32 bytes), _fvn<f> _fvo<f> _fvf<f> (FeatureVector: nodes, offsets, features), _x<f> (n x 3
//   floats), _v<f> (bytes: has a map point), _T<f> (12 floats)
//   outputs per neighbour p = 1 ..: <out>_i<p> (int32 pairs idx1, idx2), <out>_x<p> (3 floats a point)
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <string>
#include <vector>

#include "KeyFrame.h"
#include "LocalMapping_orbfe.h"
#include "shim_driver_io.hpp"

using namespace ORB_SLAM2;

struct Side {
    KeyFrame kf;
    std::vector<std::unique_ptr<MapPoint>> points;
};

static void fill(Side& s, const std::string& pre, const std::string& k)
{
    s.kf.mvKeysUn = load<cv::KeyPoint>(pre + "_kps" + k + ".bin");
    s.kf.N = (int)s.kf.mvKeysUn.size();
    const std::vector<unsigned char> d = load<unsigned char>(pre + "_desc" + k + ".bin"), v = load<unsigned char>(pre + "_v" + k + ".bin");
    s.kf.mDescriptors = cv::Mat(s.kf.N, 32, CV_8U);
    for (size_t i = 0; i < d.size(); i++) s.kf.mDescriptors.data[i] = d[i];
    const std::vector<unsigned> fn = load<unsigned>(pre + "_fvn" + k + ".bin"), ff = load<unsigned>(pre + "_fvf" + k + ".bin");
    const std::vector<int> fo = load<int>(pre + "_fvo" + k + ".bin");
    for (size_t j = 0; j < fn.size(); j++) s.kf.mFeatVec[fn[j]] = std::vector<unsigned>(ff.begin() + fo[j], ff.begin() + fo[j + 1]);
    const std::vector<float> x = load<float>(pre + "_x" + k + ".bin"), T = load<float>(pre + "_T" + k + ".bin"), K4 = load<float>(pre + "_K.bin");
    s.kf.fx = K4[0]; s.kf.fy = K4[1]; s.kf.cx = K4[2]; s.kf.cy = K4[3];
    s.kf.mvScaleFactors = load<float>(pre + "_sf.bin");
    s.kf.mvLevelSigma2 = load<float>(pre + "_sg.bin");
    s.kf.mnScaleLevels = (int)s.kf.mvScaleFactors.size();
    s.kf.mfScaleFactor = s.kf.mvScaleFactors.size() > 1 ? s.kf.mvScaleFactors[1] : 1.0f;
    s.kf.Rcw = cv::Mat(3, 3, CV_32F);
    s.kf.tcw = cv::Mat(3, 1, CV_32F);
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) s.kf.Rcw.at<float>(r, c) = T[4 * r + c];
        s.kf.tcw.at<float>(r) = T[4 * r + 3];
    }
    s.kf.mvpMapPoints.assign((size_t)s.kf.N, nullptr);
    for (int i = 0; i < s.kf.N; i++) {
        if (!v[i]) continue;
        std::unique_ptr<MapPoint> p(new MapPoint);
        p->mWorldPos = cv::Mat(3, 1, CV_32F);
        for (int c = 0; c < 3; c++) p->mWorldPos.at<float>(c) = x[3 * i + c];
        s.kf.mvpMapPoints[i] = p.get();
        s.points.push_back(std::move(p));
    }
}

int main(int argc, char** argv)
{
    if (argc != 3) return 2;
    const std::string in = argv[1], out = argv[2];
    try {
        const int nf = load<int>(in + "_nf.bin")[0];
        std::vector<std::unique_ptr<Side>> sides;
        for (int f = 0; f < nf; f++) {
            sides.emplace_back(new Side);
            fill(*sides.back(), in, std::to_string(f));
        }
        KeyFrame* cur = &sides[0]->kf;
        for (int f = 1; f < nf; f++) cur->mvpOrderedConnectedKeyFrames.push_back(&sides[f]->kf);
        const std::vector<KeyFrame*> neigh = cur->GetBestCovisibilityKeyFrames(20);   // :225-228, monocular
        const std::vector<std::vector<NewMapPointGeometry> > made = CreateNewMapPointsGeometry(cur, neigh);
        for (size_t p = 0; p < made.size(); p++) {
            std::vector<int> idx;
            std::vector<float> x;
            for (const NewMapPointGeometry& g : made[p]) {
                idx.push_back((int)g.idx1); idx.push_back((int)g.idx2);
                for (int c = 0; c < 3; c++) x.push_back(g.x3D.at<float>(c));
            }
            dump(out + "_i" + std::to_string(p + 1) + ".bin", idx);
            dump(out + "_x" + std::to_string(p + 1) + ".bin", x);
        }
        // the keyframes are as they were: the object graph is the maintainer's loop's business
        for (int f = 0; f < nf; f++) {
            const std::vector<unsigned char> v = load<unsigned char>(in + "_v" + std::to_string(f) + ".bin");
            for (int i = 0; i < sides[f]->kf.N; i++)
                if ((sides[f]->kf.mvpMapPoints[i] != nullptr) != (v[i] != 0)) return 4;
        }
    } catch (const std::exception& e) {
        fprintf(stderr, "%s\n", e.what());
        return 3;
    }
    return 0;
}
