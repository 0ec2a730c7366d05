/*
 * Optimizer_ba_orbfe.h -- what the two bundle adjustment shims (Optimizer_localba_orbfe.cc, Optimizer_globalba_orbfe.cc) share: the flat
 * arrays both library calls take, and the two loops both collect steps run over a map point's and a map marker's observations.
 * Header-only; copy it along with either of the two shims.
 */
#ifndef ORBFE_OPTIMIZER_BA_H
#define ORBFE_OPTIMIZER_BA_H

#include <cstdint>
#include <map>
#include <stdexcept>
#include <string>
#include <vector>

#include "KeyFrame.h"
#include "MapAruco.h"
#include "MapPoint.h"
#include "orbfe_shim.h"

namespace ORB_SLAM2
{
namespace orbfe_ba
{

// the arrays of orbfe_local_bundle_adjustment and orbfe_global_bundle_adjustment
struct Arrays {
    std::vector<float> Tcw, x3Dw, obs_xy, Twm, marker_local, mobs_corners, inv_level_sigma2;
    std::vector<uint8_t> kf_fixed;
    std::vector<int32_t> obs_offset, obs_kf, obs_octave, mobs_offset, mobs_kf;
    float K4[4] = {0, 0, 0, 0};
};

// One map point: its position, and one monocular edge for every observer that keep(kf) lets through, in the order of the point's
// observation map; slot gives a kept keyframe's vertex.  A stereo observation throws, in the name of `who`.
template <class Keep>
void AppendPoint(MapPoint* mp, const std::map<KeyFrame*, int32_t>& slot, Keep keep, const char* who, Arrays& pb)
{
    float X[3];
    orbfe_shim::point3(mp->GetWorldPos(), X);
    pb.x3Dw.insert(pb.x3Dw.end(), X, X + 3);
    const std::map<KeyFrame*, size_t> seen = mp->GetObservations();
    for (const auto& o : seen) {
        KeyFrame* kf = o.first;
        if (!keep(kf)) continue;
        if (kf->mvuRight[o.second] >= 0) throw std::runtime_error(std::string(who) + ": stereo observations are not supported");
        const cv::KeyPoint& kp = kf->mvKeysUn[o.second];
        pb.obs_kf.push_back(slot.at(kf));
        pb.obs_xy.push_back(kp.pt.x);
        pb.obs_xy.push_back(kp.pt.y);
        pb.obs_octave.push_back(kp.octave);
    }
    pb.obs_offset.push_back((int32_t)pb.obs_kf.size());
}

// One map marker: its pose, its four corners in the marker frame, and the four observed corners in every observer that keep(kf) lets
// through, in the order of the marker's observation map.
template <class Keep>
void AppendMarker(MapAruco* ma, const std::map<KeyFrame*, int32_t>& slot, Keep keep, Arrays& pb)
{
    orbfe_shim::append_pose(ma->GetTwm(), pb.Twm);
    for (size_t k = 0; k < 4; k++) {
        const cv::Point3f c = ma->get3DPointsLocalRefSystem(k);
        pb.marker_local.push_back(c.x);
        pb.marker_local.push_back(c.y);
        pb.marker_local.push_back(c.z);
    }
    const std::map<KeyFrame*, size_t> seen = ma->GetObservations();
    for (const auto& o : seen) {
        KeyFrame* kf = o.first;
        if (!keep(kf)) continue;
        pb.mobs_kf.push_back(slot.at(kf));
        for (size_t k = 0; k < 4; k++) {
            const cv::Point2f& c = kf->mvArucoUn[4 * o.second + k];
            pb.mobs_corners.push_back(c.x);
            pb.mobs_corners.push_back(c.y);
        }
    }
    pb.mobs_offset.push_back((int32_t)pb.mobs_kf.size());
}

} // namespace orbfe_ba
} // namespace ORB_SLAM2

#endif
