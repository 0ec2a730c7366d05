// sim3_points.hpp -- the camera-frame points of a keyframe pair, as both loop-closing solvers (sim3_solver.hip, sim3_optimizer.hip)
// build them: X3Dc = Rcw x + tcw in OpenCV's CV_32F convention (a Mat product: double sums of float products in index order, plus
// C, rounded once).
#pragma once

namespace orbfe {
namespace {

// d = A x + t for a 3 x 4 row-major [A | t]: the Mat product with C (alpha = beta = 1)
__device__ __forceinline__ void rigid(const float* T, float x, float y, float z, float* d)
{
    for (int r = 0; r < 3; r++)
        d[r] = (float)((((double)T[4 * r] * x + (double)T[4 * r + 1] * y) + (double)T[4 * r + 2] * z) + (double)T[4 * r + 3]);
}

} // namespace
} // namespace orbfe
