/*
 * orbfe_shim.h -- the plumbing the shims of this directory share: the error check that throws, and the copies between OpenCV's types
 * and the flat arrays of include/orbfe.h.  Header-only; copy it along with whichever shim you take.  Only what at
 * least two shims use lives here.
 */
#ifndef ORBFE_SHIM_H
#define ORBFE_SHIM_H

#include <stdexcept>

#include <opencv2/core/core.hpp>

#include "orbfe.h"

namespace orbfe_shim
{

// library errors are thrown as std::runtime_error
inline void check(int rc)
{
    if (rc != ORBFE_OK) throw std::runtime_error(orbfe_last_error());
}

// cv::KeyPoint is 28 bytes: pt, size, angle, response, octave, class_id -- the layout of orbfe_keypoint
inline const orbfe_keypoint* keys(const std::vector<cv::KeyPoint>& v)
{
    static_assert(sizeof(cv::KeyPoint) == sizeof(orbfe_keypoint), "cv::KeyPoint layout");
    return reinterpret_cast<const orbfe_keypoint*>(v.data());
}
inline orbfe_keypoint* keys(std::vector<cv::KeyPoint>& v)   // for the extractor, which writes them
{
    return const_cast<orbfe_keypoint*>(keys(const_cast<const std::vector<cv::KeyPoint>&>(v)));
}

// rows x cols floats as a CV_32F matrix
inline cv::Mat mat32(int rows, int cols, const float* v)
{
    cv::Mat m(rows, cols, CV_32F);
    for (int r = 0; r < rows; r++)
        for (int c = 0; c < cols; c++) m.at<float>(r, c) = v[r * cols + c];
    return m;
}

// [R | t] (3 x 3 and 3 x 1, CV_32F) as the 12 floats of a row-major 3 x 4 pose
inline void pose34(const cv::Mat& R, const cv::Mat& t, float T[12])
{
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) T[4 * r + c] = R.at<float>(r, c);
        T[4 * r + 3] = t.at<float>(r);
    }
}

// the top three rows of a 4 x 4 (or 3 x 4) CV_32F pose, appended as 12 floats
inline void append_pose(const cv::Mat& T, std::vector<float>& out)
{
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 4; c++) out.push_back(T.at<float>(r, c));
}

// the 12 floats of a row-major 3 x 4 pose as the 4 x 4 CV_32F matrix KeyFrame::SetPose takes
inline cv::Mat pose4x4(const float* T12)
{
    cv::Mat pose(4, 4, CV_32F);
    for (int i = 0; i < 16; i++) pose.at<float>(i / 4, i % 4) = i < 12 ? T12[i] : (i == 15 ? 1.f : 0.f);
    return pose;
}

// the information the reference's bundle adjustments give a marker corner edge
const float kMarkerInformation = 25.f;

// {fx, fy, cx, cy} of a 3 x 3 CV_32F calibration matrix
inline void intrinsics(const cv::Mat& K, float K4[4])
{
    K4[0] = K.at<float>(0, 0);
    K4[1] = K.at<float>(1, 1);
    K4[2] = K.at<float>(0, 2);
    K4[3] = K.at<float>(1, 2);
}

// a 3 x 1 CV_32F position (MapPoint::GetWorldPos) as three floats
inline void point3(const cv::Mat& X, float x[3])
{
    for (int k = 0; k < 3; k++) x[k] = X.at<float>(k);
}

} // namespace orbfe_shim

#endif
