/*
 * LocalMapping_orbfe.h (shim) -- the geometry of LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:222-447, monocular) on
 * liborbfe.so, as one free function.  Implemented in LocalMapping_orbfe.cc; INTEGRATION.md has the loop that calls it.
 */
#ifndef LOCALMAPPING_ORBFE_H
#define LOCALMAPPING_ORBFE_H

#include <cstddef>
#include <functional>
#include <vector>

#include <opencv2/core/core.hpp>

namespace ORB_SLAM2
{

class KeyFrame;

// what lines :299-447 leave for one successful triangulation: the two feature indices and the point (3 x 1, CV_32F)
struct NewMapPointGeometry
{
    size_t idx1, idx2;
    cv::Mat x3D;
};

/* For each neighbour, in order, the triples of the points CreateNewMapPoints would create, in the reference's creation order
 * (ascending idx1).  A feature of the current keyframe that received a point from an earlier neighbour of the list is not matched
 * again, as in the reference, where the loop has called AddMapPoint by then; the keyframes themselves are not modified.
 * stop, when given, is asked before every neighbour but the first (the reference's CheckNewKeyFrames()): true ends the list, the
 * remaining entries of the result stay empty. */
std::vector<std::vector<NewMapPointGeometry> > CreateNewMapPointsGeometry(KeyFrame* pCurrentKF, const std::vector<KeyFrame*>& vpNeighKFs,
                                                                          const std::function<bool()>& stop = std::function<bool()>());

} // namespace ORB_SLAM2

#endif
