// ba_edges.hpp -- the edges of the two bundle adjustments on the device (local_ba.hip, global_ba.hip): EdgeSE3ProjectXYZ with g2o's
// analytic Jacobians, EdgeMarker with g2o's numeric ones, the blocks an edge adds to its vertices, the wave-level sums, and the steps
// the passes of the two share: the observation decode of setup, a marker corner edge's linearisation, the damped 3 x 3 inverse, the
// Schur pair item, the point update, the unpacking of a vertex's sums.
#pragma once
#include "lm_dense.hpp"
#include "se3_quat.hpp"

namespace orbfe {
namespace {

__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

__device__ __forceinline__ double wave_max(double v)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v = fmax(v, __shfl_xor(v, off, 64));
    return v;
}

__device__ __forceinline__ bool finite_f(float v) { return isfinite(v); }

struct MonoLin {
    double err[2], Jp[2][6], Jx[2][3];
};

// EdgeSE3ProjectXYZ: computeError and linearizeOplus (types_six_dof_expmap.cpp:103-139)
__device__ __noinline__ void lba_mono_linearize(const SE3& T, const double (&Xw)[3], double ox, double oy, const Cam& K, MonoLin& o)
{
    double Xc[3], R[3][3];
    map(T, Xw, Xc);
    project_error(Xc, ox, oy, K, o.err);
    const double x = Xc[0], y = Xc[1], z = Xc[2], z_2 = z * z;
    const double s = -1. / z;
    const double t0[3] = {s * K.fx, s * 0., s * (-x / z * K.fx)}, t1[3] = {s * 0., s * K.fy, s * (-y / z * K.fy)};
    rot_of(T.q, R);
    for (int c = 0; c < 3; c++) {
        o.Jx[0][c] = t0[0] * R[0][c] + t0[1] * R[1][c] + t0[2] * R[2][c];
        o.Jx[1][c] = t1[0] * R[0][c] + t1[1] * R[1][c] + t1[2] * R[2][c];
    }
    o.Jp[0][0] = x * y / z_2 * K.fx;
    o.Jp[0][1] = -(1 + (x * x / z_2)) * K.fx;
    o.Jp[0][2] = y / z * K.fx;
    o.Jp[0][3] = -1. / z * K.fx;
    o.Jp[0][4] = 0;
    o.Jp[0][5] = x / z_2 * K.fx;
    o.Jp[1][0] = (1 + y * y / z_2) * K.fy;
    o.Jp[1][1] = -x * y / z_2 * K.fy;
    o.Jp[1][2] = -x / z * K.fy;
    o.Jp[1][3] = 0;
    o.Jp[1][4] = -1. / z * K.fy;
    o.Jp[1][5] = y / z_2 * K.fy;
}

__device__ __noinline__ void lba_mono_error(const SE3& T, const double (&Xw)[3], double ox, double oy, const Cam& K, double (&err)[2])
{
    double Xc[3];
    map(T, Xw, Xc);
    project_error(Xc, ox, oy, K, err);
}

// EdgeMarker::computeError: obs - pi((c2g g2m) point)
__device__ __noinline__ void lba_marker_error(const SE3& Tc, const SE3& Tm, const double (&pm)[3], double ox, double oy, const Cam& K,
                                              double (&err)[2])
{
    const SE3 Tcm = mul(Tc, Tm);
    double Xc[3];
    map(Tcm, pm, Xc);
    project_error(Xc, ox, oy, K, err);
}

// BaseBinaryEdge::linearizeOplus for one vertex: central differences through exp(+-1e-9 e_d) * estimate
__device__ __noinline__ void lba_marker_jacobian(const SE3& Tc, const SE3& Tm, bool camera, const double (&pm)[3], double ox, double oy,
                                                 const Cam& K, double (&J)[2][6])
{
    const double delta = 1e-9, scalar = 1.0 / (2 * delta);
    for (int d = 0; d < 6; d++) {
        double u[6] = {0, 0, 0, 0, 0, 0}, ep[2], em[2];
        u[d] = delta;
        SE3 E = se3_exp(u);
        if (camera) lba_marker_error(mul(E, Tc), Tm, pm, ox, oy, K, ep);
        else lba_marker_error(Tc, mul(E, Tm), pm, ox, oy, K, ep);
        u[d] = -delta;
        E = se3_exp(u);
        if (camera) lba_marker_error(mul(E, Tc), Tm, pm, ox, oy, K, em);
        else lba_marker_error(Tc, mul(E, Tm), pm, ox, oy, K, em);
        J[0][d] = scalar * (ep[0] - em[0]);
        J[1][d] = scalar * (ep[1] - em[1]);
    }
}

__device__ __forceinline__ bool all_finite(const double* v, int n)
{
    bool ok = true;
    for (int i = 0; i < n; i++) ok = ok && isfinite(v[i]);
    return ok;
}

// upper triangle of Ja^T w Ja (21) and Ja^T r (6)
__device__ __noinline__ void lba_diag_block(const double (&J)[2][6], double w, double r0, double r1, double* out)
{
    int k = 0;
    for (int a = 0; a < 6; a++)
        for (int c = a; c < 6; c++, k++) out[k] = J[0][a] * (w * J[0][c]) + J[1][a] * (w * J[1][c]);
    for (int a = 0; a < 6; a++) out[21 + a] = J[0][a] * r0 + J[1][a] * r1;
}

// ------------------------------------------------------------------------------------- the passes' shared steps --
// The pieces below are what k_lba_* and k_gba_* state once: none knows which of the two calls it.  All __forceinline__, the same
// expressions in the order the kernels had them.
__device__ __forceinline__ bool stop_set(const uint8_t* stop) { return stop && *(const volatile uint8_t*)stop != 0; }

// the point of observation slot i: the last point whose range starts at or before i (np > 0)
__device__ __forceinline__ int obs_point(const int32_t* obs_offset, int np, int i)
{
    int lo = 0, hi = np - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (obs_offset[mid] <= i) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// The pixel and octave of observation slot i of keyframe kf (in range) in either form -- (obs_xy, obs_oct), or obs_feat into the
// keyframe's `capacity` keypoints -- and whether they can be used: the feature and the octave in range (else 0), the pixel finite.
struct ObsPixel {
    float x = 0.f, y = 0.f;
    int oct = 0;
    bool ok = true;
};
__device__ __forceinline__ ObsPixel obs_pixel(int i, int kf, const float* obs_xy, const int32_t* obs_oct, const int32_t* obs_feat, const orbfe_keypoint* kps,
                                              int capacity, int nlevels)
{
    ObsPixel o;
    if (obs_xy) {
        o.x = obs_xy[(size_t)i * 2];
        o.y = obs_xy[(size_t)i * 2 + 1];
        o.oct = obs_oct[i];
    } else {
        const int f = obs_feat[i];
        if (f < 0 || f >= capacity) o.ok = false;
        else {
            const orbfe_keypoint kp = kps[(size_t)kf * capacity + f];
            o.x = kp.x; o.y = kp.y; o.oct = kp.octave;
        }
    }
    if (o.oct < 0 || o.oct >= nlevels) {
        o.ok = false;
        o.oct = 0;
    }
    if (!finite_f(o.x) || !finite_f(o.y)) o.ok = false;
    return o;
}

// (What a monocular edge adds to H, b and its block stays in the two linearisation kernels: as a shared function it doubled
// k_lba_linearize's scratch reloads, 57 to 118, and that kernel ran 204 us instead of 155: DESIGN.md 4k.)

// corner k of observation o of marker m: the corner in the marker's frame and its pixel
struct MarkerCorner {
    double pm[3], ox, oy;
};
__device__ __forceinline__ MarkerCorner marker_corner(const float* mlocal, const float* mobs_corners, int m, int o, int k)
{
    return MarkerCorner{{mlocal[(size_t)m * 12 + 3 * k], mlocal[(size_t)m * 12 + 3 * k + 1], mlocal[(size_t)m * 12 + 3 * k + 2]},
                        mobs_corners[(size_t)o * 8 + 2 * k], mobs_corners[(size_t)o * 8 + 2 * k + 1]};
}

// One marker corner edge linearised: chi2 and the kernel's rho[0] (chi2 itself unless robust), and, when everything is finite (the
// return value), the edge's blocks in blk: Acc, bc, Amm, bm, Acm.  A fixed camera has a zero Jacobian.
__device__ __forceinline__ bool marker_edge_linearize(const SE3& Tc, const SE3& Tm, const MarkerCorner& mc, const Cam& K, bool camfree, bool robust,
                                                      double marker_info, double delta, double* blk, double& chi2, double& rho0)
{
    double err[2], Jc[2][6], Jm[2][6];
    lba_marker_error(Tc, Tm, mc.pm, mc.ox, mc.oy, K, err);
    chi2 = chi2_of(err, marker_info);
    double rho[2] = {chi2, 1.};
    if (robust) huber(chi2, delta, rho);
    rho0 = rho[0];
    for (int a = 0; a < 6; a++) Jc[0][a] = Jc[1][a] = 0;
    if (camfree) lba_marker_jacobian(Tc, Tm, true, mc.pm, mc.ox, mc.oy, K, Jc);
    lba_marker_jacobian(Tc, Tm, false, mc.pm, mc.ox, mc.oy, K, Jm);
    const bool fin = all_finite(err, 2) && all_finite(&Jc[0][0], 12) && all_finite(&Jm[0][0], 12) && isfinite(rho[1]);
    if (fin) {
        const double w = rho[1] * marker_info;
        const double r0 = rho[1] * -(marker_info * err[0]), r1 = rho[1] * -(marker_info * err[1]);
        lba_diag_block(Jc, w, r0, r1, blk);
        lba_diag_block(Jm, w, r0, r1, blk + 27);
        for (int a = 0; a < 6; a++)
            for (int cc = 0; cc < 6; cc++) blk[54 + a * 6 + cc] = Jc[0][a] * (w * Jm[0][cc]) + Jc[1][a] * (w * Jm[1][cc]);
    }
    return fin;
}

// D = (H + lambda I)^-1 of a point's packed Hll (00 01 02 11 12 22) by cofactors (Eigen's 3 x 3 inverse)
__device__ __forceinline__ void damped_inverse3(const double* H, double lambda, double* D)
{
    const double m00 = H[0] + lambda, m01 = H[1], m02 = H[2], m11 = H[3] + lambda, m12 = H[4], m22 = H[5] + lambda;
    const double c00 = m11 * m22 - m12 * m12, c10 = m12 * m02 - m01 * m22, c20 = m01 * m12 - m11 * m02;
    const double det = c00 * m00 + c10 * m01 + c20 * m02, id = 1. / det;
    D[0] = c00 * id; D[1] = c10 * id; D[2] = c20 * id;
    D[3] = D[1]; D[4] = (m00 * m22 - m02 * m02) * id; D[5] = (m02 * m01 - m00 * m12) * id;
    D[6] = D[2]; D[7] = D[5]; D[8] = (m00 * m11 - m01 * m01) * id;
}

// one point both vertices of a pair see: acc += W_i D^-1 W_j^T, and on the diagonal accb += W_i D^-1 bl
__device__ __forceinline__ void pair_item_add(const double* Wi, const double* Wj, const double* D, const double* bl, bool diag, double (&acc)[36],
                                              double (&accb)[6])
{
    for (int a = 0; a < 6; a++) {
        double Y[3];
        for (int cc = 0; cc < 3; cc++) Y[cc] = Wi[a * 3] * D[cc] + Wi[a * 3 + 1] * D[3 + cc] + Wi[a * 3 + 2] * D[6 + cc];
        for (int bb = 0; bb < 6; bb++) acc[a * 6 + bb] += Y[0] * Wj[bb * 3] + Y[1] * Wj[bb * 3 + 1] + Y[2] * Wj[bb * 3 + 2];
        if (diag) accb[a] += Y[0] * bl[0] + Y[1] * bl[1] + Y[2] * bl[2];
    }
}

// the point's update xl = D^-1 r, r = bl - sum W^T x over its edges: one edge's term, then the product
__device__ __forceinline__ void point_rhs_sub(const double* W, const double* x, double (&r)[3])
{
    for (int cc = 0; cc < 3; cc++) {
        double s = 0;
        for (int a = 0; a < 6; a++) s += W[a * 3 + cc] * x[a];
        r[cc] -= s;
    }
}
__device__ __forceinline__ void point_solve(const double* D, const double (&r)[3], double* xl)
{
    for (int a = 0; a < 3; a++) xl[a] = D[a * 3] * r[0] + D[a * 3 + 1] * r[1] + D[a * 3 + 2] * r[2];
}

// a vertex's 27 sums (the upper triangle of Hpp row by row, then bp) into H (6 x 6, both triangles) and bp; returns the largest
// |diagonal entry|
__device__ __forceinline__ double unpack_pose_sums(const double* s, double* H, double* bp)
{
    int k = 0;
    double md = 0;
    for (int a = 0; a < 6; a++)
        for (int cc = a; cc < 6; cc++, k++) H[a * 6 + cc] = H[cc * 6 + a] = s[k];
    for (int a = 0; a < 6; a++) {
        bp[a] = s[21 + a];
        md = fmax(md, fabs(H[a * 6 + a]));
    }
    return md;
}

} // namespace
} // namespace orbfe
