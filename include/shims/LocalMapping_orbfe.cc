/*
 * LocalMapping_orbfe.cc (shim) -- the geometry of LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:222-447, monocular) on
 * liborbfe.so.  Compile it NEXT TO src/LocalMapping.cc and replace the body of the neighbour loop by the text of INTEGRATION.md: the
 * baseline gate, ComputeF12, SearchForTriangulation and the triangulation of every match become ONE orbfe_create_new_map_points call
 * per neighbour; the loop keeps the object-graph lines :449-464.
 *
 * The function flattens the keyframes on the host: mvKeysUn, mDescriptors, mFeatVec, the pose, and per feature "has a map point"
 * (GetMapPoint(i) != NULL, what ComputeSceneMedianDepth and SearchForTriangulation test) with its world position.  The current
 * keyframe's flags and points are carried from neighbour to neighbour as the library returns them, which is what the reference's
 * AddMapPoint calls do to the next neighbour's search.
 *
 * Deviations: one camera and one level table serve both keyframes (the library takes one): a neighbour whose fx, fy, cx, cy,
 * mvScaleFactors or mvLevelSigma2 differ from the current keyframe's is refused.  A triangulated point that is not finite is
 * rejected (the reference would keep it).  A neighbour without map points is skipped (the reference reads past an empty vector).
 * Library errors are thrown as std::runtime_error.
 */
#include "LocalMapping_orbfe.h"

#include <cstdint>
#include <stdexcept>

#include "KeyFrame.h"
#include "MapPoint.h"
#include "orbfe_shim.h"

using namespace std;

namespace ORB_SLAM2
{

using namespace orbfe_shim;

namespace
{

// a keyframe as the flat arrays of orbfe_create_new_map_points
struct FlatKeyFrame
{
    vector<uint32_t> node, feature;   // DBoW2::FeatureVector (std::map<NodeId, std::vector<unsigned>>)
    vector<int32_t> offset;
    vector<float> x3Dw;
    vector<uint8_t> valid;
    float Tcw[12];
    explicit FlatKeyFrame(KeyFrame* pKF) : x3Dw(3 * (size_t)pKF->N, 0.f), valid((size_t)pKF->N, 0)
    {
        offset.push_back(0);
        for (DBoW2::FeatureVector::const_iterator it = pKF->mFeatVec.begin(); it != pKF->mFeatVec.end(); ++it) {
            node.push_back(it->first);
            feature.insert(feature.end(), it->second.begin(), it->second.end());
            offset.push_back((int32_t)feature.size());
        }
        for (int i = 0; i < pKF->N; i++) {
            MapPoint* pMP = pKF->GetMapPoint(i);
            if (!pMP) continue;
            valid[i] = 1;
            point3(pMP->GetWorldPos(), &x3Dw[3 * (size_t)i]);
        }
        pose34(pKF->GetRotation(), pKF->GetTranslation(), Tcw);
    }
};

} // namespace

vector<vector<NewMapPointGeometry> > CreateNewMapPointsGeometry(KeyFrame* pCurrentKF, const vector<KeyFrame*>& vpNeighKFs,
                                                                const function<bool()>& stop)
{
    KeyFrame* pKF1 = pCurrentKF;
    vector<vector<NewMapPointGeometry> > result(vpNeighKFs.size());
    FlatKeyFrame f1(pKF1);
    const float K4[4] = {pKF1->fx, pKF1->fy, pKF1->cx, pKF1->cy};
    const float ratioFactor = 1.5f * pKF1->mfScaleFactor;   // :247
    const int n1 = pKF1->N;
    vector<int32_t> match12(n1, -1);
    vector<uint8_t> status(n1, 0);
    vector<float> x3D(3 * (size_t)n1), normal(3 * (size_t)n1), dist(2 * (size_t)n1);
    for (size_t i = 0; i < vpNeighKFs.size(); i++) {
        if (i > 0 && stop && stop()) break;   // :254-255
        KeyFrame* pKF2 = vpNeighKFs[i];
        if (pKF2->fx != K4[0] || pKF2->fy != K4[1] || pKF2->cx != K4[2] || pKF2->cy != K4[3] || pKF2->mvScaleFactors != pKF1->mvScaleFactors ||
            pKF2->mvLevelSigma2 != pKF1->mvLevelSigma2)
            throw std::runtime_error("CreateNewMapPoints (orbfe): the keyframes' cameras or level tables differ");
        FlatKeyFrame f2(pKF2);
        float F12[9], epipole[2];
        orbfe_new_points_pair prep;
        orbfe_new_points_result res;
        check(orbfe_create_new_map_points(keys(pKF1->mvKeysUn), pKF1->mDescriptors.data, n1, f1.node.data(), f1.offset.data(), f1.feature.data(),
                                          (int)f1.node.size(), f1.x3Dw.data(), f1.valid.data(), f1.Tcw, keys(pKF2->mvKeysUn),
                                          pKF2->mDescriptors.data, pKF2->N, f2.node.data(), f2.offset.data(), f2.feature.data(),
                                          (int)f2.node.size(), f2.x3Dw.data(), f2.valid.data(), f2.Tcw, K4, pKF1->mvScaleFactors.data(),
                                          pKF1->mvLevelSigma2.data(), pKF1->mnScaleLevels, ratioFactor, 0 /* ORBmatcher(0.6, false), :230 */, F12,
                                          epipole, &prep, match12.data(), status.data(), x3D.data(), normal.data(), dist.data(), &res, 0));
        result[i].reserve(res.n_new);
        for (int i1 = 0; i1 < n1; i1++) {
            if (status[i1] != ORBFE_NMP_CREATED) continue;
            NewMapPointGeometry g;
            g.idx1 = (size_t)i1;
            g.idx2 = (size_t)match12[i1];
            g.x3D = mat32(3, 1, &x3D[3 * (size_t)i1]);
            result[i].push_back(g);
        }
    }
    return result;
}

} // namespace ORB_SLAM2
