// sim3_solver.hip -- the Sim3 RANSAC of loop closing (ORB_SLAM2::Sim3Solver, src/Sim3Solver.cc) on gfx950.
//
// One problem = one Sim3Solver: two keyframes, the map points matched between them (SearchByBoW's vpMatches12), and a window of
// RANSAC iterations, each a closed-form Horn alignment of 3 correspondences scored over all N of them.  Launches, every one over
// all problems of a call:
//   k_sim3_prep     1 workgroup per problem:  the constructor (:43-111) -- correspondences compacted in index order (ballot prefix),
//                                  X3Dc = Rcw x + tcw, the chi-square gates, FromCameraToImage; SetRansacParameters (:114-138); the
//                                  3-index sets of the window decoded from the caller's rand() words (ransac_sets.hpp)
//   k_sim3_models   1 lane per hypothesis:   ComputeSim3 (:226-337): centroids, M, N, the 4 x 4 eigenproblem, Rodrigues, scale, T12, T21
//   k_sim3_inliers  1 wave per hypothesis:   Project + CheckInliers (:340-403), lanes over correspondences, the flags as a bit mask
//                                  (ballot), the count by popcount
//   k_sim3_select   1 workgroup per problem:  iterate()'s sequential acceptance (:183-200) as a scan in iteration order, the result
//                                  record, vbInliers scattered through indices1
//
// Numerics: OpenCV 3.4 restated for CV_32F, in the conventions of initializer.hip (Mat products: double sums of float products in
// index order, scaled by alpha, plus beta C, rounded once).  Chosen here:
//   cv::reduce(SUM) + C / 3     float sums left to right, then * (float)(1.0 / 3)  (a scaled assignment multiplies in float)
//   N11 .. N44                  sums of M's floats in double, then rounded to float (:247-265)
//   cv::eigen                   the classical Jacobi method in float: pivot = the largest off-diagonal element of the upper
//                               triangle (row-major scan, first wins), stop at |p| <= FLT_EPSILON or 30 n^2 rotations,
//                               y = (W[l] - W[k]) / 2, t = |y| + hypot(p, y), s = hypot(p, t), c = t / s, s = p / s, t = p / t * p,
//                               hypot(a, b) = max * sqrt(1 + (min / max)^2); eigenvalues sorted descending with their vectors
//   cv::norm (L2)               double sum of squares, sqrt in double;  atan2 in double
//   2 * ang * vec / norm        alpha = (2 ang) * (1 / norm) in double, rounded to float, vec * alpha in float
//   cv::Rodrigues               in double: theta = |r|, R = cos I + (1 - cos) r r' + sin [r]x on r / theta, rounded to float
//   Mat::dot                    double sum of float products in row-major order;  cv::pow(P3, 2): float x * x;  den: double sum
//   s * R, (1 / s) * R'         float products with (float)s and (float)(1.0 / s)
//   O1 - s R O2                 one product: (sum R O2) * (-s) + O1 in double, rounded once;  -sRinv * t: (sum) * (-1)
// The chi-square gates: the reference keeps mvnMaxError1 / 2 in std::vector<size_t> (include/Sim3Solver.h:78-79), so
// 9.210 * sigma2 (double * float) is TRUNCATED to an integer there, and err < gate compares floats; the gate here is that
// integer as a float (9 at level 0, 13 at 1.2^2, ...).
// The rotation sequence of cv::eigen depends on stale pivot caches that are not restated; eigenvectors agree with it to float
// accuracy where the two leading eigenvalues are separated.
//
// Defined where the reference is undefined: N < 3 with min_inliers <= N -> as N < min_inliers (no_more = 1, nothing found, no
// word read); a hypothesis whose quaternion has no imaginary part (norm 0 or not finite: 0 / 0 at :280) -> zero model, zero
// inliers, and it never becomes `best`; a point with z = 0 projects to inf / NaN and is never an inlier; an iteration count that
// is not finite or below 1 (log of a negative number: N < min_inliers, min_inliers = 0) -> 1.
#include "host_stage.hpp"
#include "orbfe_common.hpp"
#include "ransac_sets.hpp"
#include "sim3_points.hpp"
#include <cfloat>
#include <cmath>

namespace orbfe {
namespace {

constexpr int SIM3_MODEL = 40;      // floats per hypothesis: s12, R12[9], t12[3], T12 3 x 4, T21 3 x 4 (37) + padding
constexpr int SIM3_MAX_LEVELS = 32;

struct Sim3State {
    int N;          // correspondences kept
    int max_its;    // mRansacMaxIts
    int count;      // iterations of this call's window (0: nothing to run)
    int status;     // ORBFE_OK or ORBFE_ERR_INVALID (an octave outside the level table)
};

struct Sim3Args {
    // per-frame blocks of `capacity` (x3Dw: x 3; Tcw: 12 floats a frame)
    const orbfe_keypoint* kps;
    const int32_t* nk;
    const float* x3Dw;
    const uint8_t* valid;        // may be NULL: every feature has a good map point
    const float* Tcw;
    const int32_t *pair1, *pair2; // frames of problem p; NULL: p and p + 1
    const int32_t* m12;          // problem p at m12 + p * capacity
    const int32_t* words;        // problem p at words + p * iters * 3
    int capacity, iters;         // iters: hypothesis slots per problem (the window of the host call, max_iterations of the batch)
    int nlevels, fix_scale, min_inliers, max_iterations, first, best_in;
    double probability;
    float K1[4], K2[4];          // fx, fy, cx, cy
    float ls2[SIM3_MAX_LEVELS];
    // scratch, per problem
    Sim3State* st;
    int32_t* idx1;               // capacity
    float *X1, *X2;              // capacity * 3
    float *P1, *P2;              // capacity * 2
    float *e1, *e2;              // capacity
    int32_t* sets;               // iters * 3
    float* models;               // iters * SIM3_MODEL
    int32_t* counts;             // iters (-1: degenerate hypothesis)
    unsigned long long* masks;   // iters * mwords
    int mwords;                  // ceil(capacity / 64)
    // outputs
    orbfe_sim3_result* res;
    uint8_t* inl;                // capacity per problem
};

// FromCameraToImage / the tail of Project (:394-402, :415-422)
__device__ __forceinline__ void to_image(const float* X, const float* K, float* uv)
{
    const float invz = 1 / X[2];
    const float x = X[0] * invz, y = X[1] * invz;
    uv[0] = K[0] * x + K[2];
    uv[1] = K[1] * y + K[3];
}

__global__ __launch_bounds__(256) void k_sim3_prep(Sim3Args a)
{
    const int p = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int cap = a.capacity;
    const int f1 = a.pair1 ? a.pair1[p] : p, f2 = a.pair2 ? a.pair2[p] : p + 1;
    const int n1 = clampn(a.nk[f1], cap), n2 = clampn(a.nk[f2], cap);
    const orbfe_keypoint* k1 = a.kps + (size_t)f1 * cap;
    const orbfe_keypoint* k2 = a.kps + (size_t)f2 * cap;
    const float* x1 = a.x3Dw + (size_t)f1 * cap * 3;
    const float* x2 = a.x3Dw + (size_t)f2 * cap * 3;
    const uint8_t* v1 = a.valid ? a.valid + (size_t)f1 * cap : nullptr;
    const uint8_t* v2 = a.valid ? a.valid + (size_t)f2 * cap : nullptr;
    const int32_t* m12 = a.m12 + (size_t)p * cap;
    const size_t o = (size_t)p * cap;
    __shared__ int s_cnt[4], s_base, s_bad;
    __shared__ float sT[24];
    if (tid < 12) sT[tid] = a.Tcw[(size_t)f1 * 12 + tid];
    else if (tid < 24) sT[tid] = a.Tcw[(size_t)f2 * 12 + tid - 12];
    if (tid == 0) { s_base = 0; s_bad = 0; }
    __syncthreads();
    for (int base = 0; base < n1; base += 256) {
        const int i1 = base + tid;
        int i2 = -1;
        bool keep = false;
        if (i1 < n1) {
            i2 = m12[i1];      // an index outside frame 2 counts as "no match"
            keep = i2 >= 0 && i2 < n2 && (!v1 || (v1[i1] != 0 && v2[i2] != 0));
        }
        const unsigned long long b = __ballot(keep);
        if (lane == 0) s_cnt[wv] = __popcll(b);
        __syncthreads();
        if (keep) {
            int idx = s_base + __popcll(b & ((1ull << lane) - 1ull));
            for (int w = 0; w < wv; w++) idx += s_cnt[w];
            const int o1 = k1[i1].octave, o2 = k2[i2].octave;
            const bool bad = o1 < 0 || o1 >= a.nlevels || o2 < 0 || o2 >= a.nlevels;
            if (bad) s_bad = 1;
            // (size_t)(9.210 * sigma2), compared as a float (see the header)
            a.e1[o + idx] = bad ? 0.f : (float)(unsigned long long)(9.210 * a.ls2[o1]);
            a.e2[o + idx] = bad ? 0.f : (float)(unsigned long long)(9.210 * a.ls2[o2]);
            a.idx1[o + idx] = i1;
            float X[3], uv[2];
            rigid(sT, x1[3 * i1], x1[3 * i1 + 1], x1[3 * i1 + 2], X);
            to_image(X, a.K1, uv);
            for (int r = 0; r < 3; r++) a.X1[(o + idx) * 3 + r] = X[r];
            a.P1[(o + idx) * 2] = uv[0]; a.P1[(o + idx) * 2 + 1] = uv[1];
            rigid(sT + 12, x2[3 * i2], x2[3 * i2 + 1], x2[3 * i2 + 2], X);
            to_image(X, a.K2, uv);
            for (int r = 0; r < 3; r++) a.X2[(o + idx) * 3 + r] = X[r];
            a.P2[(o + idx) * 2] = uv[0]; a.P2[(o + idx) * 2 + 1] = uv[1];
        }
        __syncthreads();
        if (tid == 0) s_base += s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
        __syncthreads();
    }
    const int N = s_base;
    __shared__ int s_count;
    if (tid == 0) {
        // SetRansacParameters: epsilon is a float, its cube and the logarithms are doubles
        int max_its = 1;
        if (N > 0 && a.min_inliers != N) {
            const float epsilon = (float)a.min_inliers / N;
            const double nit = ceil(log(1 - a.probability) / log(1 - pow((double)epsilon, 3)));
            max_its = nit >= (double)a.max_iterations ? a.max_iterations : nit >= 1 ? (int)nit : 1;
        }
        int count = max_its - a.first;
        count = count > a.iters ? a.iters : count < 0 ? 0 : count;
        if (N < a.min_inliers || N < 3 || s_bad) count = 0;
        Sim3State* st = a.st + p;
        st->N = N; st->max_its = max_its; st->count = count; st->status = s_bad ? ORBFE_ERR_INVALID : ORBFE_OK;
        s_count = count;
    }
    __syncthreads();
    const int32_t* w = a.words + (size_t)p * a.iters * 3;
    int32_t* sets = a.sets + (size_t)p * a.iters * 3;
    for (int it = tid; it < s_count; it += 256) decode_set<3>(w + it * 3, N, sets + it * 3);
}

// -------------------------------------------------------------------------------- cv::eigen, 4 x 4 --
__device__ __forceinline__ float cv_hypot(float a, float b)
{
    a = fabsf(a);
    b = fabsf(b);
    if (a > b) {
        b /= a;
        return a * sqrtf(1 + b * b);
    }
    if (b > 0) {
        a /= b;
        return b * sqrtf(1 + a * a);
    }
    return 0;
}

// one Jacobi rotation of the pivot (K, L), K < L, on the upper triangle of A; W the diagonal, V the eigenvectors in rows.
// Compile-time indices: everything stays in registers.
template <int K, int L>
__device__ __forceinline__ void jacobi_rotate(float (&A)[4][4], float (&W)[4], float (&V)[4][4])
{
    const float p = A[K][L];
    const float y = (float)((W[L] - W[K]) * 0.5);
    float t = fabsf(y) + cv_hypot(p, y);
    float s = cv_hypot(p, t);
    const float c = t / s;
    s = p / s;
    t = (p / t) * p;
    if (y < 0) { s = -s; t = -t; }
    A[K][L] = 0;
    W[K] -= t;
    W[L] += t;
#define ORBFE_ROT(v0, v1) { const float a0 = v0, b0 = v1; v0 = a0 * c - b0 * s; v1 = a0 * s + b0 * c; }
#pragma unroll
    for (int i = 0; i < 4; i++) {
        if (i < K) ORBFE_ROT(A[i][K], A[i][L])
        else if (i > K && i < L) ORBFE_ROT(A[K][i], A[i][L])
        else if (i > L) ORBFE_ROT(A[K][i], A[L][i])
    }
#pragma unroll
    for (int i = 0; i < 4; i++) ORBFE_ROT(V[K][i], V[L][i])
#undef ORBFE_ROT
}

// eigenvector of the largest eigenvalue of the symmetric Nm -> q[4]
__device__ void eigen4_leading(const float (&Nm)[4][4], float* q)
{
    float A[4][4], V[4][4], W[4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
#pragma unroll
        for (int j = 0; j < 4; j++) { A[i][j] = Nm[i][j]; V[i][j] = i == j ? 1.f : 0.f; }
        W[i] = Nm[i][i];
    }
    for (int iters = 0; iters < 4 * 4 * 30; iters++) {
        int piv = 0;
        float mv = fabsf(A[0][1]);
        if (mv < fabsf(A[0][2])) { mv = fabsf(A[0][2]); piv = 1; }
        if (mv < fabsf(A[0][3])) { mv = fabsf(A[0][3]); piv = 2; }
        if (mv < fabsf(A[1][2])) { mv = fabsf(A[1][2]); piv = 3; }
        if (mv < fabsf(A[1][3])) { mv = fabsf(A[1][3]); piv = 4; }
        if (mv < fabsf(A[2][3])) { mv = fabsf(A[2][3]); piv = 5; }
        if (!(mv > FLT_EPSILON)) break;    // also ends on NaN
        switch (piv) {
        case 0: jacobi_rotate<0, 1>(A, W, V); break;
        case 1: jacobi_rotate<0, 2>(A, W, V); break;
        case 2: jacobi_rotate<0, 3>(A, W, V); break;
        case 3: jacobi_rotate<1, 2>(A, W, V); break;
        case 4: jacobi_rotate<1, 3>(A, W, V); break;
        default: jacobi_rotate<2, 3>(A, W, V); break;
        }
    }
    // the sort's first step: the first largest eigenvalue goes to row 0
    int m = 0;
    float wm = W[0];
    if (wm < W[1]) { wm = W[1]; m = 1; }
    if (wm < W[2]) { wm = W[2]; m = 2; }
    if (wm < W[3]) { wm = W[3]; m = 3; }
#pragma unroll
    for (int i = 0; i < 4; i++) q[i] = m == 0 ? V[0][i] : m == 1 ? V[1][i] : m == 2 ? V[2][i] : V[3][i];
}

__global__ __launch_bounds__(64) void k_sim3_models(Sim3Args a)
{
    const int p = blockIdx.y;
    const int h = blockIdx.x * 64 + threadIdx.x;
    const Sim3State* st = a.st + p;
    if (h >= st->count) return;
    const size_t o = (size_t)p * a.capacity;
    const int32_t* set = a.sets + ((size_t)p * a.iters + h) * 3;
    float* mo = a.models + ((size_t)p * a.iters + h) * SIM3_MODEL;
    int32_t* cnt = a.counts + (size_t)p * a.iters + h;
    // P[r][i]: coordinate r of point i (the columns of P3Dc1i / P3Dc2i)
    float P1[3][3], P2[3][3], O1[3], O2[3];
    for (int i = 0; i < 3; i++)
        for (int r = 0; r < 3; r++) {
            P1[r][i] = a.X1[(o + set[i]) * 3 + r];
            P2[r][i] = a.X2[(o + set[i]) * 3 + r];
        }
    const float third = (float)(1.0 / 3);
    for (int r = 0; r < 3; r++) {
        O1[r] = ((P1[r][0] + P1[r][1]) + P1[r][2]) * third;
        O2[r] = ((P2[r][0] + P2[r][1]) + P2[r][2]) * third;
        for (int i = 0; i < 3; i++) { P1[r][i] -= O1[r]; P2[r][i] -= O2[r]; }
    }
    // M = Pr2 * Pr1'
    float M[3][3];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++)
            M[i][j] = (float)(((double)P2[i][0] * P1[j][0] + (double)P2[i][1] * P1[j][1]) + (double)P2[i][2] * P1[j][2]);
    const double N11 = (double)M[0][0] + M[1][1] + M[2][2];
    const double N12 = (double)M[1][2] - M[2][1];
    const double N13 = (double)M[2][0] - M[0][2];
    const double N14 = (double)M[0][1] - M[1][0];
    const double N22 = (double)M[0][0] - M[1][1] - M[2][2];
    const double N23 = (double)M[0][1] + M[1][0];
    const double N24 = (double)M[2][0] + M[0][2];
    const double N33 = -(double)M[0][0] + M[1][1] - M[2][2];
    const double N34 = (double)M[1][2] + M[2][1];
    const double N44 = -(double)M[0][0] - M[1][1] + M[2][2];
    const float Nm[4][4] = {{(float)N11, (float)N12, (float)N13, (float)N14},
                            {(float)N12, (float)N22, (float)N23, (float)N24},
                            {(float)N13, (float)N23, (float)N33, (float)N34},
                            {(float)N14, (float)N24, (float)N34, (float)N44}};
    float q[4];
    eigen4_leading(Nm, q);
    const double nrm = sqrt(((double)q[1] * q[1] + (double)q[2] * q[2]) + (double)q[3] * q[3]);
    if (!(nrm > 0) || !(nrm < (double)INFINITY)) {
        for (int i = 0; i < 37; i++) mo[i] = 0;
        *cnt = -1;
        return;
    }
    const double ang = atan2(nrm, (double)q[0]);
    const float alpha = (float)((2 * ang) * (1.0 / nrm));
    const float v[3] = {q[1] * alpha, q[2] * alpha, q[3] * alpha};
    // cv::Rodrigues
    float R[3][3];
    {
        double rx = v[0], ry = v[1], rz = v[2];
        const double theta = sqrt(rx * rx + ry * ry + rz * rz);
        if (theta < DBL_EPSILON) {
            for (int i = 0; i < 3; i++)
                for (int j = 0; j < 3; j++) R[i][j] = i == j ? 1.f : 0.f;
        } else {
            const double c = cos(theta), s = sin(theta), c1 = 1. - c, itheta = 1. / theta;
            rx *= itheta; ry *= itheta; rz *= itheta;
            const double rrt[9] = {rx * rx, rx * ry, rx * rz, rx * ry, ry * ry, ry * rz, rx * rz, ry * rz, rz * rz};
            const double r_x[9] = {0, -rz, ry, rz, 0, -rx, -ry, rx, 0};
            for (int k = 0; k < 9; k++) R[k / 3][k % 3] = (float)((c * (k % 4 == 0 ? 1. : 0.) + c1 * rrt[k]) + s * r_x[k]);
        }
    }
    float s12 = 1.0f;
    if (!a.fix_scale) {
        // P3 = R * Pr2; nom = Pr1 . P3; den = sum of P3^2
        double nom = 0, den = 0;
        for (int r = 0; r < 3; r++)
            for (int i = 0; i < 3; i++) {
                const float p3 = (float)(((double)R[r][0] * P2[0][i] + (double)R[r][1] * P2[1][i]) + (double)R[r][2] * P2[2][i]);
                nom += (double)P1[r][i] * p3;
                den += (double)(p3 * p3);
            }
        s12 = (float)(nom / den);
    }
    float t[3];
    for (int r = 0; r < 3; r++)
        t[r] = (float)((((double)R[r][0] * O2[0] + (double)R[r][1] * O2[1]) + (double)R[r][2] * O2[2]) * (-(double)s12) + (double)O1[r]);
    const float sinv = (float)(1.0 / s12);
    float sRi[3][3], ti[3];
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) sRi[r][c] = R[c][r] * sinv;
    for (int r = 0; r < 3; r++)
        ti[r] = (float)((((double)sRi[r][0] * t[0] + (double)sRi[r][1] * t[1]) + (double)sRi[r][2] * t[2]) * -1.0);
    mo[0] = s12;
    for (int k = 0; k < 9; k++) mo[1 + k] = R[k / 3][k % 3];
    for (int r = 0; r < 3; r++) {
        mo[10 + r] = t[r];
        for (int c = 0; c < 3; c++) {
            mo[13 + 4 * r + c] = R[r][c] * s12;
            mo[25 + 4 * r + c] = sRi[r][c];
        }
        mo[13 + 4 * r + 3] = t[r];
        mo[25 + 4 * r + 3] = ti[r];
    }
    *cnt = 0;
}

__global__ __launch_bounds__(64) void k_sim3_inliers(Sim3Args a)
{
    const int p = blockIdx.y, h = blockIdx.x, lane = threadIdx.x;
    const Sim3State* st = a.st + p;
    if (h >= st->count) return;
    int32_t* cnt = a.counts + (size_t)p * a.iters + h;
    if (*cnt < 0) return;     // degenerate hypothesis: no model
    const int N = st->N;
    const size_t o = (size_t)p * a.capacity;
    const float* mo = a.models + ((size_t)p * a.iters + h) * SIM3_MODEL;
    unsigned long long* mask = a.masks + ((size_t)p * a.iters + h) * a.mwords;
    float T12[12], T21[12];
    for (int k = 0; k < 12; k++) { T12[k] = mo[13 + k]; T21[k] = mo[25 + k]; }
    int total = 0;
    for (int base = 0; base < N; base += 64) {
        const int i = base + lane;
        bool ok = false;
        if (i < N) {
            float X[3], uv[2];
            rigid(T12, a.X2[(o + i) * 3], a.X2[(o + i) * 3 + 1], a.X2[(o + i) * 3 + 2], X);   // vP2im1
            to_image(X, a.K1, uv);
            const float d1x = a.P1[(o + i) * 2] - uv[0], d1y = a.P1[(o + i) * 2 + 1] - uv[1];
            rigid(T21, a.X1[(o + i) * 3], a.X1[(o + i) * 3 + 1], a.X1[(o + i) * 3 + 2], X);   // vP1im2
            to_image(X, a.K2, uv);
            const float d2x = uv[0] - a.P2[(o + i) * 2], d2y = uv[1] - a.P2[(o + i) * 2 + 1];
            const float err1 = (float)((double)d1x * d1x + (double)d1y * d1y);
            const float err2 = (float)((double)d2x * d2x + (double)d2y * d2y);
            ok = err1 < a.e1[o + i] && err2 < a.e2[o + i];
        }
        const unsigned long long b = __ballot(ok);
        if (lane == 0) mask[base >> 6] = b;
        total += __popcll(b);
    }
    if (lane == 0) *cnt = total;
}

__global__ __launch_bounds__(256) void k_sim3_select(Sim3Args a)
{
    const int p = blockIdx.x, tid = threadIdx.x;
    const Sim3State* st = a.st + p;
    const int cap = a.capacity;
    const int f1 = a.pair1 ? a.pair1[p] : p;
    const int n1 = clampn(a.nk[f1], cap);
    const int N = st->N, count = st->count;
    const int32_t* counts = a.counts + (size_t)p * a.iters;
    orbfe_sim3_result* res = a.res + p;
    uint8_t* inl = a.inl + (size_t)p * cap;
    __shared__ int s_c[1024];
    __shared__ int s_best, s_besti, s_found;
    if (st->status != ORBFE_OK) {
        // the batch call's skipped problem: status and nothing else
        if (tid == 0) {
            orbfe_sim3_result r{};
            r.status = st->status;
            *res = r;
        }
        return;
    }
    if (tid == 0) { s_best = a.best_in; s_besti = -1; s_found = -1; }
    __syncthreads();
    for (int base = 0; base < count; base += 1024) {
        for (int i = tid; i < 1024 && base + i < count; i += 256) s_c[i] = counts[base + i];
        __syncthreads();
        if (tid == 0) {
            int best = s_best, besti = s_besti, found = -1;
            const int n = count - base < 1024 ? count - base : 1024;
            for (int i = 0; i < n; i++) {
                const int c = s_c[i];
                if (c >= best) {
                    best = c; besti = base + i;
                    if (c > a.min_inliers) { found = base + i; break; }
                }
            }
            s_best = best; s_besti = besti; s_found = found;
        }
        __syncthreads();
        if (s_found >= 0) break;
    }
    const int found = s_found, besti = s_besti;
    if (tid == 0) {
        orbfe_sim3_result r{};
        r.n = N;
        r.max_iterations = st->max_its;
        r.found = found >= 0 ? a.first + found : -1;
        r.n_inliers = found >= 0 ? s_best : 0;
        r.best = besti >= 0 ? a.first + besti : -1;
        r.best_inliers = s_best;
        r.no_more = (N < a.min_inliers || N < 3) ? 1 : (found < 0 && a.first + count >= st->max_its) ? 1 : 0;
        if (besti >= 0) {
            const float* mo = a.models + ((size_t)p * a.iters + besti) * SIM3_MODEL;
            r.s12 = mo[0];
            for (int k = 0; k < 9; k++) r.R12[k] = mo[1 + k];
            for (int k = 0; k < 3; k++) r.t12[k] = mo[10 + k];
            for (int k = 0; k < 12; k++) r.T12[k] = mo[13 + k];
            r.T12[15] = 1.f;
        }
        r.status = ORBFE_OK;
        *res = r;
    }
    for (int i = tid; i < n1; i += 256) inl[i] = 0;
    __syncthreads();
    if (found >= 0) {
        const unsigned long long* mask = a.masks + ((size_t)p * a.iters + found) * a.mwords;
        const int32_t* idx1 = a.idx1 + (size_t)p * cap;
        for (int i = tid; i < N; i += 256)
            if ((mask[i >> 6] >> (i & 63)) & 1ull) inl[idx1[i]] = 1;
    }
}

// ------------------------------------------------------------------------------------------- host --
thread_local ThreadWorkspaces<HostStage> tl_stages;

int carve(DevBuf& buf, Sim3Args& a, int npairs)
{
    const size_t cap = (size_t)a.capacity, P = (size_t)npairs, it = (size_t)a.iters;
    a.mwords = (int)((cap + 63) / 64);
    IoLayout l;
    const size_t o_st = l.take(P * sizeof(Sim3State)), o_idx = l.take(P * cap * 4), o_X1 = l.take(P * cap * 12), o_X2 = l.take(P * cap * 12);
    const size_t o_P1 = l.take(P * cap * 8), o_P2 = l.take(P * cap * 8), o_e1 = l.take(P * cap * 4), o_e2 = l.take(P * cap * 4);
    const size_t o_sets = l.take(P * it * 12), o_mod = l.take(P * it * SIM3_MODEL * 4), o_cnt = l.take(P * it * 4);
    const size_t o_mask = l.take(P * it * (size_t)a.mwords * 8);
    int rc = buf.ensure(l.end());
    if (rc) return rc;
    uint8_t* b = buf.as<uint8_t>();
    a.st = (Sim3State*)(b + o_st);
    a.idx1 = (int32_t*)(b + o_idx);
    a.X1 = (float*)(b + o_X1); a.X2 = (float*)(b + o_X2);
    a.P1 = (float*)(b + o_P1); a.P2 = (float*)(b + o_P2);
    a.e1 = (float*)(b + o_e1); a.e2 = (float*)(b + o_e2);
    a.sets = (int32_t*)(b + o_sets);
    a.models = (float*)(b + o_mod);
    a.counts = (int32_t*)(b + o_cnt);
    a.masks = (unsigned long long*)(b + o_mask);
    return ORBFE_OK;
}

int launch(const Sim3Args& a, int npairs, hipStream_t s)
{
    hipLaunchKernelGGL(k_sim3_prep, dim3(npairs), dim3(256), 0, s, a);
    hipLaunchKernelGGL(k_sim3_models, dim3((a.iters + 63) / 64, npairs), dim3(64), 0, s, a);
    hipLaunchKernelGGL(k_sim3_inliers, dim3(a.iters, npairs), dim3(64), 0, s, a);
    hipLaunchKernelGGL(k_sim3_select, dim3(npairs), dim3(256), 0, s, a);
    ORBFE_HIP(hipGetLastError());
    return ORBFE_OK;
}

int check_common(const char* name, const float* K4_1, const float* K4_2, const float* level_sigma2, int nlevels, double probability,
                 int min_inliers, int max_iterations)
{
    if (!K4_1 || !K4_2 || !level_sigma2) return fail(ORBFE_ERR_INVALID, "%s: NULL K4 or level_sigma2", name);
    if (nlevels <= 0 || nlevels > SIM3_MAX_LEVELS) return fail(ORBFE_ERR_INVALID, "%s: nlevels = %d is not in 1 .. %d", name, nlevels, SIM3_MAX_LEVELS);
    if (!(probability > 0 && probability < 1)) return fail(ORBFE_ERR_INVALID, "%s: probability is not in (0, 1)", name);
    if (min_inliers < 0 || max_iterations <= 0 || max_iterations > 100000)
        return fail(ORBFE_ERR_INVALID, "%s: min_inliers < 0, or max_iterations not in 1 .. 100000", name);
    for (int i = 0; i < 4; i++)
        if (!std::isfinite(K4_1[i]) || !std::isfinite(K4_2[i])) return fail(ORBFE_ERR_INVALID, "%s: K is not finite", name);
    return ORBFE_OK;
}

void fill_common(Sim3Args& a, const float* K4_1, const float* K4_2, const float* level_sigma2, int nlevels, int fix_scale,
                 double probability, int min_inliers, int max_iterations)
{
    for (int i = 0; i < 4; i++) { a.K1[i] = K4_1[i]; a.K2[i] = K4_2[i]; }
    for (int i = 0; i < nlevels; i++) a.ls2[i] = level_sigma2[i];
    a.nlevels = nlevels;
    a.fix_scale = fix_scale != 0;
    a.probability = probability;
    a.min_inliers = min_inliers;
    a.max_iterations = max_iterations;
}

struct Sim3HostCall {
    const orbfe_keypoint *kps1, *kps2;
    int n1, n2;
    const float *x1, *x2;
    const uint8_t *v1, *v2;
    const float *Tcw1, *Tcw2, *K1, *K2;
    const int32_t* m12;
    const float* ls2;
    int nlevels, fix_scale;
    double probability;
    int min_inliers, max_iterations, first, n_iterations, best_in;
    const int32_t* words;
    orbfe_sim3_result* res;
    uint8_t* inl;
    // orbfe_sim3_inspect, NULL / false when not wanted
    bool inspect;
    int32_t *n_out, *indices1;
    float *X3Dc1, *X3Dc2, *P1im1, *P2im2, *maxError1, *maxError2;
    int32_t* sets;
    float* models;
    int32_t* counts;
};

int sim3_host_call(const Sim3HostCall& c, int device, const char* name)
{
    if (c.n1 < 0 || c.n2 < 0 || !c.res || !c.Tcw1 || !c.Tcw2 || !c.words || (c.n1 && (!c.kps1 || !c.m12 || !c.x1 || !c.inl)) ||
        (c.n2 && (!c.kps2 || !c.x2)) || ((c.v1 == nullptr) != (c.v2 == nullptr)))
        return fail(ORBFE_ERR_INVALID, "%s: invalid argument (NULL pointer or negative size)", name);
    int rc = check_common(name, c.K1, c.K2, c.ls2, c.nlevels, c.probability, c.min_inliers, c.max_iterations);
    if (rc) return rc;
    if (c.first < 0 || c.n_iterations <= 0 || c.n_iterations > 100000 || c.best_in < 0)
        return fail(ORBFE_ERR_INVALID, "%s: first_iteration < 0, n_iterations not in 1 .. 100000 or best_inliers_in < 0", name);
    for (int i = 0; i < c.n1; i++) {
        const int j = c.m12[i];
        if (j >= c.n2 || j < -1) return fail(ORBFE_ERR_INVALID, "%s: match12[%d] = %d is not in [-1, n2)", name, i, j);
        if (j < 0 || (c.v1 && (!c.v1[i] || !c.v2[j]))) continue;
        const int o1 = c.kps1[i].octave, o2 = c.kps2[j].octave;
        if (o1 < 0 || o1 >= c.nlevels || o2 < 0 || o2 >= c.nlevels)
            return fail(ORBFE_ERR_INVALID, "%s: correspondence %d -> %d has an octave outside [0, %d)", name, i, j, c.nlevels);
    }
    for (int i = 0; i < c.n_iterations * 3; i++)
        if (c.words[i] < 0) return fail(ORBFE_ERR_INVALID, "%s: rand_words[%d] is negative (rand() returns 0 .. RAND_MAX)", name, i);
    if ((rc = use_device(device))) return rc;
    HostStage& w = tl_stages.get();
    Sim3Args a{};
    a.capacity = std::max(std::max(c.n1, c.n2), 1);
    a.iters = c.n_iterations;
    a.first = c.first;
    a.best_in = c.best_in;
    fill_common(a, c.K1, c.K2, c.ls2, c.nlevels, c.fix_scale, c.probability, c.min_inliers, c.max_iterations);
    const size_t cap = (size_t)a.capacity, nw = (size_t)c.n_iterations * 3, kb = sizeof(orbfe_keypoint);
    // device io: [kps 2 cap | n | x3Dw 2 cap x 3 | valid 2 cap | Tcw 24 | m12 cap | words] [res | inliers cap]
    IoLayout l;
    const size_t i_kps = l.take(2 * cap * kb), i_n = l.take(8), i_x = l.take(2 * cap * 12), i_v = l.take(2 * cap);
    const size_t i_T = l.take(96), i_m = l.take(cap * 4), i_w = l.take(nw * 4);
    l.outputs();
    const size_t o_res = l.take(sizeof(orbfe_sim3_result)), o_inl = l.take(cap);
    if ((rc = w.begin(l)) || (rc = carve(w.host_scratch, a, 1))) return rc;
    const hipStream_t s = w.stream;
    const int32_t nn[2] = {c.n1, c.n2};
    w.put(i_kps, c.kps1, (size_t)c.n1 * kb);
    w.put(i_kps + cap * kb, c.kps2, (size_t)c.n2 * kb);
    w.put(i_n, nn, 8);
    w.put(i_x, c.x1, (size_t)c.n1 * 12);
    w.put(i_x + cap * 12, c.x2, (size_t)c.n2 * 12);
    if (c.v1) {
        w.put(i_v, c.v1, (size_t)c.n1);
        w.put(i_v + cap, c.v2, (size_t)c.n2);
    }
    w.put(i_T, c.Tcw1, 48);
    w.put(i_T + 48, c.Tcw2, 48);
    w.put(i_m, c.m12, (size_t)c.n1 * 4);
    w.put(i_w, c.words, nw * 4);
    if ((rc = w.upload())) return rc;
    a.kps = w.dev<const orbfe_keypoint>(i_kps); a.nk = w.dev<const int32_t>(i_n); a.x3Dw = w.dev<const float>(i_x);
    a.valid = c.v1 ? w.dev<const uint8_t>(i_v) : nullptr;
    a.Tcw = w.dev<const float>(i_T); a.m12 = w.dev<const int32_t>(i_m); a.words = w.dev<const int32_t>(i_w);
    a.res = w.dev<orbfe_sim3_result>(o_res); a.inl = w.dev<uint8_t>(o_inl);
    if ((rc = launch(a, 1, s)) || (rc = w.download())) return rc;
    std::vector<float> mod;
    if (c.inspect) {
        // the intermediate results, straight from the scratch (a diagnostic path: one copy per array)
        const size_t n1 = (size_t)c.n1, it = (size_t)c.n_iterations;
        mod.resize(it * SIM3_MODEL);
        ORBFE_HIP(hipMemcpyAsync(c.n_out, &a.st->N, 4, hipMemcpyDeviceToHost, s));
        if (n1) {
            ORBFE_HIP(hipMemcpyAsync(c.indices1, a.idx1, n1 * 4, hipMemcpyDeviceToHost, s));
            ORBFE_HIP(hipMemcpyAsync(c.X3Dc1, a.X1, n1 * 12, hipMemcpyDeviceToHost, s));
            ORBFE_HIP(hipMemcpyAsync(c.X3Dc2, a.X2, n1 * 12, hipMemcpyDeviceToHost, s));
            ORBFE_HIP(hipMemcpyAsync(c.P1im1, a.P1, n1 * 8, hipMemcpyDeviceToHost, s));
            ORBFE_HIP(hipMemcpyAsync(c.P2im2, a.P2, n1 * 8, hipMemcpyDeviceToHost, s));
            ORBFE_HIP(hipMemcpyAsync(c.maxError1, a.e1, n1 * 4, hipMemcpyDeviceToHost, s));
            ORBFE_HIP(hipMemcpyAsync(c.maxError2, a.e2, n1 * 4, hipMemcpyDeviceToHost, s));
        }
        ORBFE_HIP(hipMemcpyAsync(c.sets, a.sets, it * 12, hipMemcpyDeviceToHost, s));
        ORBFE_HIP(hipMemcpyAsync(mod.data(), a.models, it * SIM3_MODEL * 4, hipMemcpyDeviceToHost, s));
        ORBFE_HIP(hipMemcpyAsync(c.counts, a.counts, it * 4, hipMemcpyDeviceToHost, s));
    }
    if ((rc = w.sync())) return rc;
    const orbfe_sim3_result* r = w.host<const orbfe_sim3_result>(o_res);
    *c.res = *r;
    if (c.n1) memcpy(c.inl, w.host<uint8_t>(o_inl), (size_t)c.n1);
    if (c.inspect) {
        // entries past N and hypotheses the window did not run (it ends at max_iterations, or at N < 3 / N < min_inliers) are 0.
        // Every hypothesis of the window is computed and scored, also those after the one that was found.
        const int N = *c.n_out;
        const int ran = (N < c.min_inliers || N < 3) ? 0 : std::max(0, std::min(c.n_iterations, r->max_iterations - c.first));
        for (int i = N; i < c.n1; i++) {
            c.indices1[i] = 0; c.maxError1[i] = c.maxError2[i] = 0;
            for (int k = 0; k < 3; k++) c.X3Dc1[3 * i + k] = c.X3Dc2[3 * i + k] = 0;
            for (int k = 0; k < 2; k++) c.P1im1[2 * i + k] = c.P2im2[2 * i + k] = 0;
        }
        for (int h = 0; h < c.n_iterations; h++) {
            const bool live = h < ran;
            for (int k = 0; k < 3; k++) c.sets[3 * h + k] = live ? c.sets[3 * h + k] : 0;
            for (int k = 0; k < 13; k++) c.models[13 * h + k] = live ? mod[(size_t)h * SIM3_MODEL + k] : 0.f;
            c.counts[h] = live && c.counts[h] > 0 ? c.counts[h] : 0;
        }
    }
    return ORBFE_OK;
}

// the arguments orbfe_sim3_solve and orbfe_sim3_inspect share, as a call
Sim3HostCall solve_call(const orbfe_keypoint* kps1, int n1, const float* x3Dw1, const uint8_t* valid1, const float* Tcw1, const float* K4_1,
                        const orbfe_keypoint* kps2, int n2, const float* x3Dw2, const uint8_t* valid2, const float* Tcw2, const float* K4_2,
                        const int32_t* match12, const float* level_sigma2, int nlevels, int fix_scale, double probability, int min_inliers,
                        int max_iterations, int first_iteration, int n_iterations, int best_inliers_in, const int32_t* rand_words,
                        orbfe_sim3_result* res, uint8_t* inliers12)
{
    Sim3HostCall c{};
    c.kps1 = kps1; c.n1 = n1; c.x1 = x3Dw1; c.v1 = valid1; c.Tcw1 = Tcw1; c.K1 = K4_1;
    c.kps2 = kps2; c.n2 = n2; c.x2 = x3Dw2; c.v2 = valid2; c.Tcw2 = Tcw2; c.K2 = K4_2;
    c.m12 = match12; c.ls2 = level_sigma2; c.nlevels = nlevels; c.fix_scale = fix_scale; c.probability = probability;
    c.min_inliers = min_inliers; c.max_iterations = max_iterations; c.first = first_iteration; c.n_iterations = n_iterations;
    c.best_in = best_inliers_in; c.words = rand_words; c.res = res; c.inl = inliers12;
    return c;
}

} // namespace
} // namespace orbfe

using namespace orbfe;

int orbfe_sim3_solve(const orbfe_keypoint* kps1, int n1, const float* x3Dw1, const uint8_t* valid1, const float* Tcw1, const float* K4_1,
                     const orbfe_keypoint* kps2, int n2, const float* x3Dw2, const uint8_t* valid2, const float* Tcw2, const float* K4_2,
                     const int32_t* match12, const float* level_sigma2, int nlevels, int fix_scale, double probability, int min_inliers,
                     int max_iterations, int first_iteration, int n_iterations, int best_inliers_in, const int32_t* rand_words,
                     orbfe_sim3_result* res, uint8_t* inliers12, int device)
{
    const Sim3HostCall c = solve_call(kps1, n1, x3Dw1, valid1, Tcw1, K4_1, kps2, n2, x3Dw2, valid2, Tcw2, K4_2, match12, level_sigma2, nlevels,
                                              fix_scale, probability, min_inliers, max_iterations, first_iteration, n_iterations, best_inliers_in,
                                              rand_words, res, inliers12);
    return sim3_host_call(c, device, "orbfe_sim3_solve");
}

int orbfe_sim3_inspect(const orbfe_keypoint* kps1, int n1, const float* x3Dw1, const uint8_t* valid1, const float* Tcw1, const float* K4_1,
                       const orbfe_keypoint* kps2, int n2, const float* x3Dw2, const uint8_t* valid2, const float* Tcw2, const float* K4_2,
                       const int32_t* match12, const float* level_sigma2, int nlevels, int fix_scale, double probability, int min_inliers,
                       int max_iterations, int first_iteration, int n_iterations, int best_inliers_in, const int32_t* rand_words,
                       orbfe_sim3_result* res, uint8_t* inliers12, int32_t* n, int32_t* indices1, float* X3Dc1, float* X3Dc2, float* P1im1,
                       float* P2im2, float* maxError1, float* maxError2, int32_t* sets, float* models, int32_t* counts, int device)
{
    if (!n || !sets || !models || !counts || (n1 > 0 && (!indices1 || !X3Dc1 || !X3Dc2 || !P1im1 || !P2im2 || !maxError1 || !maxError2)))
        return fail(ORBFE_ERR_INVALID, "orbfe_sim3_inspect: null output");
    Sim3HostCall c = solve_call(kps1, n1, x3Dw1, valid1, Tcw1, K4_1, kps2, n2, x3Dw2, valid2, Tcw2, K4_2, match12, level_sigma2, nlevels,
                                        fix_scale, probability, min_inliers, max_iterations, first_iteration, n_iterations, best_inliers_in,
                                        rand_words, res, inliers12);
    c.inspect = true; c.n_out = n; c.indices1 = indices1; c.X3Dc1 = X3Dc1; c.X3Dc2 = X3Dc2; c.P1im1 = P1im1; c.P2im2 = P2im2;
    c.maxError1 = maxError1; c.maxError2 = maxError2; c.sets = sets; c.models = models; c.counts = counts;
    return sim3_host_call(c, device, "orbfe_sim3_inspect");
}

int orbfe_sim3_solve_batch_device(const orbfe_keypoint* d_kps, const int32_t* d_n, int capacity, const float* d_x3Dw, const uint8_t* d_valid,
                                  const float* d_Tcw, const int32_t* d_pair1, const int32_t* d_pair2, int npairs, const int32_t* d_match12,
                                  const float* K4, const float* level_sigma2, int nlevels, int fix_scale, double probability,
                                  int min_inliers, int max_iterations, const int32_t* d_rand_words, orbfe_sim3_result* d_res,
                                  uint8_t* d_inliers12, void* stream)
{
    const char* name = "orbfe_sim3_solve_batch_device";
    if (!d_kps || !d_n || !d_x3Dw || !d_Tcw || !d_match12 || !d_rand_words || !d_res || !d_inliers12 || capacity <= 0 || npairs <= 0 ||
        ((d_pair1 == nullptr) != (d_pair2 == nullptr)))
        return fail(ORBFE_ERR_INVALID, "%s: invalid argument", name);
    int rc = check_common(name, K4, K4, level_sigma2, nlevels, probability, min_inliers, max_iterations);
    if (rc) return rc;
    const hipStream_t s = (hipStream_t)stream;
    HostStage& w = tl_stages.get(s);
    Sim3Args a{};
    a.kps = d_kps; a.nk = d_n; a.x3Dw = d_x3Dw; a.valid = d_valid; a.Tcw = d_Tcw; a.pair1 = d_pair1; a.pair2 = d_pair2;
    a.m12 = d_match12; a.words = d_rand_words;
    a.capacity = capacity;
    a.iters = max_iterations;
    a.first = 0;
    a.best_in = 0;
    fill_common(a, K4, K4, level_sigma2, nlevels, fix_scale, probability, min_inliers, max_iterations);
    a.res = d_res; a.inl = d_inliers12;
    if ((rc = carve(w.scratch, a, npairs))) return rc;
    return launch(a, npairs, s);
}
