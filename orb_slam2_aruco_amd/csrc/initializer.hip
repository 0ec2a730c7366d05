// initializer.hip -- the monocular two-view initializer (ORB_SLAM2::Initializer, src/Initializer.cc) on gfx950.
//
// One frame pair = the reference's Initialize(): 2 x `iterations` eight-point hypotheses (H and F), each scored over all N matches,
// the H / F choice (RH = SH / (SH + SF) > 0.40), then the 8 (H) or 4 (F) motion hypotheses triangulated and checked (CheckRT).
// Launches, per pair:
//   k_init_prep     1 workgroup:   matches12 -> match list in index order; Normalize() of both sides (serial float sums, the
//                                  reference's order); the 8-index sets decoded from the caller's rand() words
//   k_init_models   1 thread per hypothesis: ComputeH21 / ComputeF21 (16x9 / 8x9 one-sided Jacobi SVD), denormalisation, H12 = H21^-1,
//                                  rank-2 F
//   k_init_score    1 wave per hypothesis: CheckHomography / CheckFundamental, lanes over matches, the score summed in match order
//   k_init_select   1 workgroup:   first strict maximum of each model, RH, inlier flags of the chosen model, DecomposeE / the
//                                  Faugeras decomposition -> motion hypotheses
//   k_init_checkrt  1 workgroup per motion hypothesis: Triangulate + the gates of CheckRT, nGood, parallax (radix select)
//   k_init_finalize 1 workgroup:   ReconstructH / ReconstructF acceptance (or InitializeUseAruco's), vP3D / vbTriangulated of the winner
// The numerics restate OpenCV 3.4 for CV_32F: cv::SVD is its one-sided Jacobi (double sums of float products, float rotations,
// FLT_EPSILON*2), Mat products accumulate in double and round once, 3x3 inv / determinant are the cofactor formulas in double.
#include "host_stage.hpp"
#include "orbfe_common.hpp"
#include "ransac_sets.hpp"
#include "svd_jacobi.hpp"
#include <cfloat>
#include <cmath>

namespace orbfe {
namespace {

constexpr int INIT_MAX_MOT = 12;   // 8 (ReconstructH) or 4 (ReconstructF) motions; InitializeUseAruco runs in chunks of this many

// ---------------------------------------------------------------- OpenCV 3.4 restated (device) --
// cv::SVD (JacobiSVDImpl_<float>): svd_jacobi.hpp
// C = A * B (3x3, row-major), GEMMSingleMul<float, double>: double sums in k order, one rounding; alpha applied before it
__device__ __forceinline__ void mm3(const float* A, const float* B, float* C, double alpha = 1.0)
{
    float R[9];
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 3; c++) {
            double s = 0;
#pragma unroll
            for (int k = 0; k < 3; k++) s += (double)A[r * 3 + k] * B[k * 3 + c];
            R[r * 3 + c] = (float)(s * alpha);
        }
#pragma unroll
    for (int i = 0; i < 9; i++) C[i] = R[i];
}

__device__ __forceinline__ double det3(const float* m)
{
    return m[0] * ((double)m[4] * m[8] - (double)m[5] * m[7]) - m[1] * ((double)m[3] * m[8] - (double)m[5] * m[6]) +
           m[2] * ((double)m[3] * m[7] - (double)m[4] * m[6]);
}

// Mat::inv() (DECOMP_LU) for 3x3 float: the cofactor formula in double; a singular matrix gives zeros
__device__ __forceinline__ void inv3(const float* S, float* D)
{
    double d = det3(S);
    if (d == 0.) {
#pragma unroll
        for (int i = 0; i < 9; i++) D[i] = 0;
        return;
    }
    d = 1. / d;
    double t[9];
    t[0] = ((double)S[4] * S[8] - (double)S[5] * S[7]) * d;
    t[1] = ((double)S[2] * S[7] - (double)S[1] * S[8]) * d;
    t[2] = ((double)S[1] * S[5] - (double)S[2] * S[4]) * d;
    t[3] = ((double)S[5] * S[6] - (double)S[3] * S[8]) * d;
    t[4] = ((double)S[0] * S[8] - (double)S[2] * S[6]) * d;
    t[5] = ((double)S[2] * S[3] - (double)S[0] * S[5]) * d;
    t[6] = ((double)S[3] * S[7] - (double)S[4] * S[6]) * d;
    t[7] = ((double)S[1] * S[6] - (double)S[0] * S[7]) * d;
    t[8] = ((double)S[0] * S[4] - (double)S[1] * S[3]) * d;
#pragma unroll
    for (int i = 0; i < 9; i++) D[i] = (float)t[i];
}

// cv::SVD::compute of a 3x3 float matrix: w, u, vt (row-major)
__device__ __forceinline__ void svd3(const float* A, float* w, float* u, float* vt)
{
    float At[3][3], W[3], Vt[3][3];
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 3; c++) At[c][r] = A[r * 3 + c];
    svd_jacobi<3, 3, 3, true>(At, W, Vt);
#pragma unroll
    for (int r = 0; r < 3; r++) {
        w[r] = W[r];
#pragma unroll
        for (int c = 0; c < 3; c++) { u[r * 3 + c] = At[c][r]; vt[r * 3 + c] = Vt[r][c]; }
    }
}

// alpha of a MatExpr "m / s" as convertTo applies it to CV_32F
__device__ __forceinline__ void scale_by_inverse_norm3(float* t)
{
    const double n = sqrt((double)t[0] * t[0] + (double)t[1] * t[1] + (double)t[2] * t[2]);
    const float a = (float)(1. / n);
    t[0] = t[0] * a; t[1] = t[1] * a; t[2] = t[2] * a;
}

// ------------------------------------------------------------------------------ the pair's scratch --
struct PairState {
    int N;            // matches
    int nmot;         // motion hypotheses to check (0: Reconstruct* returned before CheckRT)
    int ninl;         // inliers of the chosen model (Reconstruct*'s N)
    int branch;       // 0 H, 1 F, 2 InitializeUseAruco, -1 nothing to do
    float T1[9], T2[9];
    float R[INIT_MAX_MOT][9], t[INIT_MAX_MOT][3];
    int ngood[INIT_MAX_MOT];
    float parallax[INIT_MAX_MOT];
    int written;      // finalize wrote p3d / triangulated
};

struct InitArgs {
    const orbfe_keypoint* kps;   // frame f at kps + f * capacity
    const int32_t* nk;           // keypoints per frame
    const int32_t* m12;          // pair p at m12 + p * capacity
    const int32_t* words;        // pair p at words + p * iters * 8
    int capacity, iters;
    float fx, fy, cx, cy, sigma;
    // scratch, per pair
    PairState* st;
    int2* mlist;                 // capacity
    float2* pn;                  // 2 * capacity: side 1, side 2
    int32_t* sets;               // iters * 8
    float* models;               // iters * 27: H21, H12, F21
    float* scores;               // 2 * iters: H then F
    uint8_t* inl;                // capacity, indexed by frame-1 keypoint
    float* cosbuf;               // INIT_MAX_MOT * capacity
    // outputs
    orbfe_init_result* res;      // one per pair
    float* p3d;                  // capacity * 3 per pair
    uint8_t* tri;                // capacity per pair
    // InitializeUseAruco
    const float* poses;          // npose x 12 (R row-major, t)
    int npose;
};

// Normalize (Initializer.cc:816-863) of one side, serial sums in index order
__device__ void normalize_side(const orbfe_keypoint* k, int n, float2* out, float* T)
{
    float meanX = 0, meanY = 0;
    for (int i = 0; i < n; i++) { meanX += k[i].x; meanY += k[i].y; }
    meanX = meanX / n;
    meanY = meanY / n;
    float meanDevX = 0, meanDevY = 0;
    for (int i = 0; i < n; i++) {
        const float x = k[i].x - meanX, y = k[i].y - meanY;
        out[i] = make_float2(x, y);
        meanDevX += fabsf(x);
        meanDevY += fabsf(y);
    }
    meanDevX = meanDevX / n;
    meanDevY = meanDevY / n;
    const float sX = (float)(1.0 / meanDevX), sY = (float)(1.0 / meanDevY);
    for (int i = 0; i < n; i++) out[i] = make_float2(out[i].x * sX, out[i].y * sY);
    T[0] = sX; T[1] = 0; T[2] = -meanX * sX;
    T[3] = 0; T[4] = sY; T[5] = -meanY * sY;
    T[6] = 0; T[7] = 0; T[8] = 1;
}

__global__ __launch_bounds__(64) void k_init_prep(InitArgs a)
{
    const int p = blockIdx.x;
    const int cap = a.capacity;
    PairState* st = a.st + p;
    const orbfe_keypoint* k1 = a.kps + (size_t)p * cap;
    const orbfe_keypoint* k2 = a.kps + (size_t)(p + 1) * cap;
    const int n1 = clampn(a.nk[p], cap), n2 = clampn(a.nk[p + 1], cap);
    const int32_t* m12 = a.m12 + (size_t)p * cap;
    int2* ml = a.mlist + (size_t)p * cap;
    __shared__ int sN;
    if (threadIdx.x == 0) {
        int N = 0;
        for (int i = 0; i < n1; i++) {
            const int j = m12[i];
            if (j >= 0 && j < n2) ml[N++] = make_int2(i, j);   // an index outside frame 2 counts as "no match"
        }
        sN = N;
        st->N = N;
        st->nmot = 0;
        st->ninl = 0;
        st->written = 0;
        st->branch = N < 8 && a.iters > 0 ? -1 : 0;   // (iters = 0: InitializeUseAruco, which draws no sets)
    } else if (threadIdx.x == 1 && n1 > 0) {
        normalize_side(k1, n1, a.pn + (size_t)p * 2 * cap, st->T1);
    } else if (threadIdx.x == 2 && n2 > 0) {
        normalize_side(k2, n2, a.pn + (size_t)p * 2 * cap + cap, st->T2);
    }
    __syncthreads();
    const int N = sN;
    if (N < 8) return;
    // the sets (Initializer.cc:80-97): RandomInt(0, size - 1) on the caller's word, then swap-with-back removal from [0, N)
    const int32_t* w = a.words + (size_t)p * a.iters * 8;
    int32_t* sets = a.sets + (size_t)p * a.iters * 8;
    for (int it = threadIdx.x; it < a.iters; it += blockDim.x) decode_set<8>(w + it * 8, N, sets + it * 8);
}

__global__ __launch_bounds__(64) void k_init_models(InitArgs a)
{
    const int p = blockIdx.y;
    const int h = blockIdx.x * 64 + threadIdx.x;
    const PairState* st = a.st + p;
    if (h >= 2 * a.iters || st->branch < 0) return;
    const int it = h < a.iters ? h : h - a.iters;
    const int cap = a.capacity;
    const int2* ml = a.mlist + (size_t)p * cap;
    const float2* pn1 = a.pn + (size_t)p * 2 * cap;
    const float2* pn2 = pn1 + cap;
    const int32_t* set = a.sets + ((size_t)p * a.iters + it) * 8;
    float* out = a.models + ((size_t)p * a.iters + it) * 27;
    float u1[8], v1[8], u2[8], v2[8];
#pragma unroll
    for (int j = 0; j < 8; j++) {
        const int2 m = ml[set[j]];
        u1[j] = pn1[m.x].x; v1[j] = pn1[m.x].y;
        u2[j] = pn2[m.y].x; v2[j] = pn2[m.y].y;
    }
    if (h < a.iters) {
        // ComputeH21 (:293-333): A 16 x 9, m >= n: At = A^T, vt.row(8)
        float At[9][16], W[9], Vt[9][9];
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const float r0[9] = {0.f, 0.f, 0.f, -u1[j], -v1[j], -1.f, v2[j] * u1[j], v2[j] * v1[j], v2[j]};
            const float r1[9] = {u1[j], v1[j], 1.f, 0.f, 0.f, 0.f, -u2[j] * u1[j], -u2[j] * v1[j], -u2[j]};
#pragma unroll
            for (int c = 0; c < 9; c++) { At[c][2 * j] = r0[c]; At[c][2 * j + 1] = r1[c]; }
        }
        svd_jacobi<16, 9, 9, false>(At, W, Vt);
        float T2inv[9], H21[9], H12[9];
        inv3(st->T2, T2inv);
        mm3(T2inv, Vt[8], H21);
        mm3(H21, st->T1, H21);
        inv3(H21, H12);
#pragma unroll
        for (int i = 0; i < 9; i++) { out[i] = H21[i]; out[9 + i] = H12[i]; }
    } else {
        // ComputeF21 (:335-370): A 8 x 9, m < n: the transposed problem, vt = U of it, row 8 from the null-space completion
        float At[9][9], W[8], Vt[8][8];
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const float r[9] = {u2[j] * u1[j], u2[j] * v1[j], u2[j], v2[j] * u1[j], v2[j] * v1[j], v2[j], u1[j], v1[j], 1.f};
#pragma unroll
            for (int c = 0; c < 9; c++) At[j][c] = r[c];
        }
#pragma unroll
        for (int c = 0; c < 9; c++) At[8][c] = 0;
        svd_jacobi<9, 8, 9, true>(At, W, Vt);
        float w[3], u[9], vt[9], ud[9], Fn[9], T2t[9], F21[9];
        svd3(At[8], w, u, vt);
        w[2] = 0;
        const float dg[9] = {w[0], 0.f, 0.f, 0.f, w[1], 0.f, 0.f, 0.f, w[2]};
        mm3(u, dg, ud);
        mm3(ud, vt, Fn);
#pragma unroll
        for (int r = 0; r < 3; r++)
#pragma unroll
            for (int c = 0; c < 3; c++) T2t[r * 3 + c] = st->T2[c * 3 + r];
        mm3(T2t, Fn, F21);
        mm3(F21, st->T1, F21);
#pragma unroll
        for (int i = 0; i < 9; i++) out[18 + i] = F21[i];
    }
}

// one match's CheckHomography terms (:372-455); returns the inlier flag
__device__ __forceinline__ bool h_terms(const float* H, const float* Hi, float u1, float v1, float u2, float v2, float inv_s2,
                                        float& t1, float& t2)
{
    const float th = 5.991f;
    bool in = true;
    const float w2in1inv = (float)(1.0 / (Hi[6] * u2 + Hi[7] * v2 + Hi[8]));
    const float u2in1 = (Hi[0] * u2 + Hi[1] * v2 + Hi[2]) * w2in1inv;
    const float v2in1 = (Hi[3] * u2 + Hi[4] * v2 + Hi[5]) * w2in1inv;
    const float sq1 = (u1 - u2in1) * (u1 - u2in1) + (v1 - v2in1) * (v1 - v2in1);
    const float chi1 = sq1 * inv_s2;
    if (chi1 > th) { in = false; t1 = 0; } else t1 = th - chi1;
    const float w1in2inv = (float)(1.0 / (H[6] * u1 + H[7] * v1 + H[8]));
    const float u1in2 = (H[0] * u1 + H[1] * v1 + H[2]) * w1in2inv;
    const float v1in2 = (H[3] * u1 + H[4] * v1 + H[5]) * w1in2inv;
    const float sq2 = (u2 - u1in2) * (u2 - u1in2) + (v2 - v1in2) * (v2 - v1in2);
    const float chi2 = sq2 * inv_s2;
    if (chi2 > th) { in = false; t2 = 0; } else t2 = th - chi2;
    return in;
}

// one match's CheckFundamental terms (:457-535)
__device__ __forceinline__ bool f_terms(const float* F, float u1, float v1, float u2, float v2, float inv_s2, float& t1, float& t2)
{
    const float th = 3.841f, thScore = 5.991f;
    bool in = true;
    const float a2 = F[0] * u1 + F[1] * v1 + F[2];
    const float b2 = F[3] * u1 + F[4] * v1 + F[5];
    const float c2 = F[6] * u1 + F[7] * v1 + F[8];
    const float num2 = a2 * u2 + b2 * v2 + c2;
    const float sq1 = num2 * num2 / (a2 * a2 + b2 * b2);
    const float chi1 = sq1 * inv_s2;
    if (chi1 > th) { in = false; t1 = 0; } else t1 = thScore - chi1;
    const float a1 = F[0] * u2 + F[3] * v2 + F[6];
    const float b1 = F[1] * u2 + F[4] * v2 + F[7];
    const float c1 = F[2] * u2 + F[5] * v2 + F[8];
    const float num1 = a1 * u1 + b1 * v1 + c1;
    const float sq2 = num1 * num1 / (a1 * a1 + b1 * b1);
    const float chi2 = sq2 * inv_s2;
    if (chi2 > th) { in = false; t2 = 0; } else t2 = thScore - chi2;
    return in;
}

__global__ __launch_bounds__(64) void k_init_score(InitArgs a)
{
    const int p = blockIdx.y, h = blockIdx.x, lane = threadIdx.x;
    const PairState* st = a.st + p;
    if (st->branch < 0) return;
    const int N = st->N, cap = a.capacity;
    const bool isH = h < a.iters;
    const int it = isH ? h : h - a.iters;
    const float* mdl = a.models + ((size_t)p * a.iters + it) * 27;
    float M[18];
#pragma unroll
    for (int i = 0; i < 18; i++) M[i] = isH ? mdl[i] : (i < 9 ? mdl[18 + i] : 0.f);
    const int2* ml = a.mlist + (size_t)p * cap;
    const orbfe_keypoint* k1 = a.kps + (size_t)p * cap;
    const orbfe_keypoint* k2 = k1 + cap;
    const float inv_s2 = (float)(1.0 / (a.sigma * a.sigma));
    __shared__ float terms[128];
    float score = 0;   // meaningful in lane 0: the reference's `score +=` in match order
    for (int base = 0; base < N; base += 64) {
        const int i = base + lane;
        float t1 = 0, t2 = 0;
        if (i < N) {
            const int2 m = ml[i];
            const float u1 = k1[m.x].x, v1 = k1[m.x].y, u2 = k2[m.y].x, v2 = k2[m.y].y;
            if (isH) h_terms(M, M + 9, u1, v1, u2, v2, inv_s2, t1, t2);
            else f_terms(M, u1, v1, u2, v2, inv_s2, t1, t2);
        }
        terms[2 * lane] = t1;
        terms[2 * lane + 1] = t2;
        __syncthreads();
        if (lane == 0) {
            const int cnt = 2 * min(64, N - base);
            for (int q = 0; q < cnt; q++) score += terms[q];   // a rejected side adds +0: the sum is unchanged
        }
        __syncthreads();
    }
    if (lane == 0) a.scores[(size_t)p * 2 * a.iters + h] = score;
}

__device__ void motions_H(const float* H21, const float* K, PairState* st)
{
    // ReconstructH (:639-799) up to the CheckRT loop
    float invK[9], A[9], w[3], U[9], Vt[9];
    inv3(K, invK);
    mm3(invK, H21, A);
    mm3(A, K, A);
    svd3(A, w, U, Vt);
    const float s = (float)(det3(U) * det3(Vt));
    const float d1 = w[0], d2 = w[1], d3 = w[2];
    if (d1 / d2 < 1.00001 || d2 / d3 < 1.00001) { st->nmot = 0; return; }
    const float aux1 = sqrtf((d1 * d1 - d2 * d2) / (d1 * d1 - d3 * d3));
    const float aux3 = sqrtf((d2 * d2 - d3 * d3) / (d1 * d1 - d3 * d3));
    const float x1[4] = {aux1, aux1, -aux1, -aux1};
    const float x3[4] = {aux3, -aux3, aux3, -aux3};
    const float aux_stheta = sqrtf((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 + d3) * d2);
    const float ctheta = (d2 * d2 + d1 * d3) / ((d1 + d3) * d2);
    const float stheta[4] = {aux_stheta, -aux_stheta, -aux_stheta, aux_stheta};
    const float aux_sphi = sqrtf((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 - d3) * d2);
    const float cphi = (d1 * d3 - d2 * d2) / ((d1 - d3) * d2);
    const float sphi[4] = {aux_sphi, -aux_sphi, -aux_sphi, aux_sphi};
    for (int m = 0; m < 8; m++) {
        const int i = m & 3;
        float Rp[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, tp[3];
        if (m < 4) {
            Rp[0] = ctheta; Rp[2] = -stheta[i]; Rp[6] = stheta[i]; Rp[8] = ctheta;
            const float f = d1 - d3;
            tp[0] = x1[i] * f; tp[1] = 0 * f; tp[2] = -x3[i] * f;
        } else {
            Rp[0] = cphi; Rp[2] = sphi[i]; Rp[4] = -1; Rp[6] = sphi[i]; Rp[8] = -cphi;
            const float f = d1 + d3;
            tp[0] = x1[i] * f; tp[1] = 0 * f; tp[2] = x3[i] * f;
        }
        float UR[9];
        mm3(U, Rp, UR, (double)s);
        mm3(UR, Vt, st->R[m]);
        float t[3];
#pragma unroll
        for (int r = 0; r < 3; r++) {
            double acc = 0;
#pragma unroll
            for (int k = 0; k < 3; k++) acc += (double)U[r * 3 + k] * tp[k];
            t[r] = (float)acc;
        }
        scale_by_inverse_norm3(t);
        st->t[m][0] = t[0]; st->t[m][1] = t[1]; st->t[m][2] = t[2];
    }
    st->nmot = 8;
}

__device__ void motions_F(const float* F21, const float* K, PairState* st)
{
    // ReconstructF (:537-637): E21 = K^T F21 K, DecomposeE (:976-998); order (R1,t) (R2,t) (R1,-t) (R2,-t)
    float Kt[9], E[9], w[3], u[9], vt[9], R1[9], R2[9], t[3];
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 3; c++) Kt[r * 3 + c] = K[c * 3 + r];
    mm3(Kt, F21, E);
    mm3(E, K, E);
    svd3(E, w, u, vt);
    t[0] = u[2]; t[1] = u[5]; t[2] = u[8];
    scale_by_inverse_norm3(t);
    const float W[9] = {0, -1, 0, 1, 0, 0, 0, 0, 1}, Wt[9] = {0, 1, 0, -1, 0, 0, 0, 0, 1};
    mm3(u, W, R1); mm3(R1, vt, R1);
    if (det3(R1) < 0) for (int i = 0; i < 9; i++) R1[i] = -R1[i];
    mm3(u, Wt, R2); mm3(R2, vt, R2);
    if (det3(R2) < 0) for (int i = 0; i < 9; i++) R2[i] = -R2[i];
    for (int m = 0; m < 4; m++) {
        const float* R = (m & 1) ? R2 : R1;
        const float sg = m < 2 ? 1.f : -1.f;
        for (int i = 0; i < 9; i++) st->R[m][i] = R[i];
        for (int i = 0; i < 3; i++) st->t[m][i] = sg * t[i];
    }
    st->nmot = 4;
}

__global__ __launch_bounds__(256) void k_init_select(InitArgs a)
{
    const int p = blockIdx.x, cap = a.capacity;
    PairState* st = a.st + p;
    orbfe_init_result* res = a.res + p;
    const float K[9] = {a.fx, 0, a.cx, 0, a.fy, a.cy, 0, 0, 1};
    __shared__ int s_branch, s_best;
    __shared__ int s_ninl;
    if (threadIdx.x == 0) {
        const float* sc = a.scores + (size_t)p * 2 * a.iters;
        float SH = 0, SF = 0;
        int bh = -1, bf = -1;
        if (st->branch >= 0)
            for (int it = 0; it < a.iters; it++) {
                if (sc[it] > SH) { SH = sc[it]; bh = it; }
                if (sc[a.iters + it] > SF) { SF = sc[a.iters + it]; bf = it; }
            }
        const float RH = SH / (SH + SF);
        int branch = RH > 0.40 ? 0 : 1;
        // no F hypothesis with a positive score (and RH <= 0.40, or NaN when both scores are 0): ReconstructF would read an empty
        // inlier vector in the reference; here nothing is reconstructed
        if (st->branch < 0 || (branch == 1 && bf < 0)) branch = -1;
        memset(res, 0, sizeof(*res));
        res->model = st->branch < 0 ? 0 : RH > 0.40 ? 0 : 1;
        res->SH = SH; res->SF = SF; res->RH = st->branch < 0 ? 0.f : RH;
        res->best_h = bh; res->best_f = bf;
        for (int i = 0; i < 9; i++) {
            res->H21[i] = bh >= 0 ? a.models[((size_t)p * a.iters + bh) * 27 + i] : 0.f;
            res->F21[i] = bf >= 0 ? a.models[((size_t)p * a.iters + bf) * 27 + 18 + i] : 0.f;
        }
        st->branch = branch;
        st->nmot = 0;
        s_branch = branch;
        s_best = branch == 0 ? bh : bf;
        s_ninl = 0;
    }
    __syncthreads();
    const int branch = s_branch;
    if (branch < 0) return;
    // the inlier flags of the winner, by frame-1 keypoint (CheckRT visits matches by index; the order does not matter to it)
    const float* mdl = a.models + ((size_t)p * a.iters + s_best) * 27;
    const int2* ml = a.mlist + (size_t)p * cap;
    const orbfe_keypoint* k1 = a.kps + (size_t)p * cap;
    const orbfe_keypoint* k2 = k1 + cap;
    uint8_t* inl = a.inl + (size_t)p * cap;
    const float inv_s2 = (float)(1.0 / (a.sigma * a.sigma));
    int cnt = 0;
    for (int i = threadIdx.x; i < st->N; i += blockDim.x) {
        const int2 m = ml[i];
        const float u1 = k1[m.x].x, v1 = k1[m.x].y, u2 = k2[m.y].x, v2 = k2[m.y].y;
        float t1, t2;
        const bool in = branch == 0 ? h_terms(mdl, mdl + 9, u1, v1, u2, v2, inv_s2, t1, t2) : f_terms(mdl + 18, u1, v1, u2, v2, inv_s2, t1, t2);
        inl[m.x] = in;
        cnt += in;
    }
    atomicAdd(&s_ninl, cnt);
    __syncthreads();
    if (threadIdx.x == 0) {
        st->ninl = s_ninl;
        if (branch == 0) motions_H(mdl, K, st);
        else motions_F(mdl + 18, K, st);
    }
}

struct RTPoint {
    float x, y, z, cosp;
    int status;   // 0 rejected, 1 counted (nGood), 2 counted and vbGood
};

// Triangulate (:801-814) + the gates of CheckRT (:865-974) for one match
__device__ __forceinline__ RTPoint check_point(const float* R, const float* t, const float* P2, const float* O2, const float* K,
                                              float kx1, float ky1, float kx2, float ky2, float th2)
{
    RTPoint r{0, 0, 0, 0, 0};
    const float P1[12] = {K[0], K[1], K[2], 0, K[3], K[4], K[5], 0, K[6], K[7], K[8], 0};
    float At[4][4], W[4], Vt[4][4];
#pragma unroll
    for (int c = 0; c < 4; c++) {   // A rows, stored transposed (m >= n: At = A^T)
        At[c][0] = (float)((double)P1[8 + c] * kx1 - (double)P1[c]);
        At[c][1] = (float)((double)P1[8 + c] * ky1 - (double)P1[4 + c]);
        At[c][2] = (float)((double)P2[8 + c] * kx2 - (double)P2[c]);
        At[c][3] = (float)((double)P2[8 + c] * ky2 - (double)P2[4 + c]);
    }
    svd_jacobi<4, 4, 4, false>(At, W, Vt);
    const float iw = (float)(1. / (double)Vt[3][3]);
    const float X = Vt[3][0] * iw, Y = Vt[3][1] * iw, Z = Vt[3][2] * iw;
    if (!isfinite(X) || !isfinite(Y) || !isfinite(Z)) return r;
    const float dist1 = (float)sqrt((double)X * X + (double)Y * Y + (double)Z * Z);
    const float n2x = X - O2[0], n2y = Y - O2[1], n2z = Z - O2[2];
    const float dist2 = (float)sqrt((double)n2x * n2x + (double)n2y * n2y + (double)n2z * n2z);
    const double dot = (double)X * n2x + (double)Y * n2y + (double)Z * n2z;
    const float cosp = (float)(dot / (double)(dist1 * dist2));
    if (Z <= 0 && cosp < 0.99998) return r;
    float c2[3];
#pragma unroll
    for (int i = 0; i < 3; i++) c2[i] = (float)((double)R[i * 3] * X + (double)R[i * 3 + 1] * Y + (double)R[i * 3 + 2] * Z + (double)t[i]);
    if (c2[2] <= 0 && cosp < 0.99998) return r;
    const float fx = K[0], fy = K[4], cx = K[2], cy = K[5];
    const float invZ1 = (float)(1.0 / Z);
    const float im1x = fx * X * invZ1 + cx, im1y = fy * Y * invZ1 + cy;
    const float se1 = (im1x - kx1) * (im1x - kx1) + (im1y - ky1) * (im1y - ky1);
    if (se1 > th2) return r;
    const float invZ2 = (float)(1.0 / c2[2]);
    const float im2x = fx * c2[0] * invZ2 + cx, im2y = fy * c2[1] * invZ2 + cy;
    const float se2 = (im2x - kx2) * (im2x - kx2) + (im2y - ky2) * (im2y - ky2);
    if (se2 > th2) return r;
    r.x = X; r.y = Y; r.z = Z; r.cosp = cosp;
    r.status = cosp < 0.99998 ? 2 : 1;
    return r;
}

// P2 = K [R | t] and O2 = -R^T t, as CheckRT builds them
__device__ __forceinline__ void camera2(const float* R, const float* t, const float* K, float* P2, float* O2)
{
    const float Rt[12] = {R[0], R[1], R[2], t[0], R[3], R[4], R[5], t[1], R[6], R[7], R[8], t[2]};
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 4; c++) {
            double s = 0;
#pragma unroll
            for (int k = 0; k < 3; k++) s += (double)K[r * 3 + k] * Rt[k * 4 + c];
            P2[r * 4 + c] = (float)s;
        }
#pragma unroll
    for (int r = 0; r < 3; r++) {
        double s = 0;
#pragma unroll
        for (int k = 0; k < 3; k++) s += (double)R[k * 3 + r] * t[k];
        O2[r] = (float)(s * -1.0);
    }
}

__device__ __forceinline__ uint32_t order_key(float f)
{
    const uint32_t b = __float_as_uint(f);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

// motion m of pair p (or pose base + m of InitializeUseAruco): nGood and parallax
__global__ __launch_bounds__(256) void k_init_checkrt(InitArgs a, int pose_base)
{
    const int p = blockIdx.y, m = blockIdx.x, cap = a.capacity;
    PairState* st = a.st + p;
    const bool aruco = a.poses != nullptr;
    if (aruco ? pose_base + m >= a.npose || st->branch < 0 : m >= st->nmot) return;
    float R[9], t[3], P2[12], O2[3];
    const float K[9] = {a.fx, 0, a.cx, 0, a.fy, a.cy, 0, 0, 1};
    for (int i = 0; i < 9; i++) R[i] = aruco ? a.poses[(size_t)(pose_base + m) * 12 + i] : st->R[m][i];
    for (int i = 0; i < 3; i++) t[i] = aruco ? a.poses[(size_t)(pose_base + m) * 12 + 9 + i] : st->t[m][i];
    camera2(R, t, K, P2, O2);
    const float th2 = (float)(4.0 * (a.sigma * a.sigma));
    const int2* ml = a.mlist + (size_t)p * cap;
    const orbfe_keypoint* k1 = a.kps + (size_t)p * cap;
    const orbfe_keypoint* k2 = k1 + cap;
    const uint8_t* inl = a.inl + (size_t)p * cap;
    float* cosb = a.cosbuf + ((size_t)p * INIT_MAX_MOT + m) * cap;
    __shared__ int s_n;
    __shared__ uint32_t hist[256];
    __shared__ uint32_t s_prefix;
    __shared__ int s_k;
    if (threadIdx.x == 0) s_n = 0;
    __syncthreads();
    const int N = st->N;
    for (int i = threadIdx.x; i < N; i += blockDim.x) {
        const int2 mm = ml[i];
        if (!aruco && !inl[mm.x]) continue;
        const RTPoint q = check_point(R, t, P2, O2, K, k1[mm.x].x, k1[mm.x].y, k2[mm.y].x, k2[mm.y].y, th2);
        if (q.status) cosb[atomicAdd(&s_n, 1)] = q.cosp;
    }
    __syncthreads();
    const int n = s_n;
    // parallax = acos(sorted cos[min(50, n - 1)]): radix select, 8 bits per pass, on order-preserving keys
    uint32_t prefix = 0;
    int k = n < 51 ? n - 1 : 50;
    if (n > 0) {
        for (int shift = 24; shift >= 0; shift -= 8) {
            for (int b = threadIdx.x; b < 256; b += blockDim.x) hist[b] = 0;
            __syncthreads();
            const uint32_t hmask = shift == 24 ? 0u : ~0u << (shift + 8);
            for (int i = threadIdx.x; i < n; i += blockDim.x) {
                const uint32_t key = order_key(cosb[i]);
                if ((key & hmask) == prefix) atomicAdd(&hist[(key >> shift) & 255u], 1u);
            }
            __syncthreads();
            if (threadIdx.x == 0) {
                int b = 0, kk = k;
                while ((int)hist[b] <= kk) { kk -= (int)hist[b]; b++; }
                s_prefix = prefix | ((uint32_t)b << shift);
                s_k = kk;
            }
            __syncthreads();
            prefix = s_prefix;
            k = s_k;
            __syncthreads();
        }
    }
    if (threadIdx.x == 0) {
        float par = 0;
        if (n > 0) {
            const uint32_t b = (prefix & 0x80000000u) ? (prefix & 0x7fffffffu) : ~prefix;
            par = (float)((double)(acosf(__uint_as_float(b)) * 180) / 3.14159265358979323846);
        }
        st->ngood[m] = n;
        st->parallax[m] = par;
    }
}

// vP3D / vbTriangulated of motion (R, t) over all n1 keypoints of frame 1, as CheckRT leaves them
__device__ void write_points(const InitArgs& a, int p, const float* R, const float* t, bool aruco)
{
    const int cap = a.capacity;
    const int n1 = clampn(a.nk[p], cap), n2 = clampn(a.nk[p + 1], cap);
    float P2[12], O2[3];
    const float K[9] = {a.fx, 0, a.cx, 0, a.fy, a.cy, 0, 0, 1};
    camera2(R, t, K, P2, O2);
    const float th2 = (float)(4.0 * (a.sigma * a.sigma));
    const orbfe_keypoint* k1 = a.kps + (size_t)p * cap;
    const orbfe_keypoint* k2 = k1 + cap;
    const int32_t* m12 = a.m12 + (size_t)p * cap;
    const uint8_t* inl = a.inl + (size_t)p * cap;
    float* p3 = a.p3d + (size_t)p * cap * 3;
    uint8_t* tri = a.tri + (size_t)p * cap;
    for (int i = threadIdx.x; i < n1; i += blockDim.x) {
        const int j = m12[i];
        RTPoint q{0, 0, 0, 0, 0};
        if (j >= 0 && j < n2 && (aruco || inl[i])) q = check_point(R, t, P2, O2, K, k1[i].x, k1[i].y, k2[j].x, k2[j].y, th2);
        p3[3 * i] = q.x; p3[3 * i + 1] = q.y; p3[3 * i + 2] = q.z;
        tri[i] = q.status == 2;
    }
}

__global__ __launch_bounds__(256) void k_init_finalize(InitArgs a)
{
    const int p = blockIdx.x;
    PairState* st = a.st + p;
    orbfe_init_result* res = a.res + p;
    __shared__ int s_win;
    if (threadIdx.x == 0) {
        int win = -1;
        const int branch = st->branch;
        if (branch == 0 && st->nmot == 8) {
            int bestGood = 0, second = 0, bi = -1;
            float bestPar = -1;
            for (int i = 0; i < 8; i++) {
                const int g = st->ngood[i];
                if (g > bestGood) { second = bestGood; bestGood = g; bi = i; bestPar = st->parallax[i]; }
                else if (g > second) second = g;
            }
            res->n_good = bestGood;
            res->parallax = bi >= 0 ? bestPar : 0.f;
            const int N = st->ninl;
            if (second < 0.75 * bestGood && bestPar >= 1.0f && bestGood > 50 && bestGood > 0.9 * N) win = bi;
        } else if (branch == 1 && st->nmot == 4) {
            const int* g = st->ngood;
            const int maxGood = max(g[0], max(g[1], max(g[2], g[3])));
            const int N = st->ninl;
            const int nMinGood = max((int)(0.9 * N), 50);
            int nsimilar = 0;
            for (int i = 0; i < 4; i++) nsimilar += g[i] > 0.7 * maxGood;
            int first = 0;
            while (g[first] != maxGood) first++;
            res->n_good = maxGood;
            res->parallax = st->parallax[first];
            if (!(maxGood < nMinGood || nsimilar > 1) && st->parallax[first] > 1.0f) win = first;
        }
        if (win >= 0) {
            res->initialized = 1;
            for (int i = 0; i < 9; i++) res->R21[i] = st->R[win][i];
            for (int i = 0; i < 3; i++) res->t21[i] = st->t[win][i];
        }
        st->written = win >= 0;
        s_win = win;
    }
    __syncthreads();
    const int win = s_win;
    if (win >= 0) write_points(a, p, st->R[win], st->t[win], false);
}

// InitializeUseAruco: the first strict maximum of nGood over this chunk of poses, folded into the running best (res->best_h holds
// its index, res->n_good its nGood); the last chunk applies bestGood < 0.7 N
__global__ __launch_bounds__(256) void k_init_poses_fold(InitArgs a, int pose_base, int last)
{
    const int p = blockIdx.x;
    PairState* st = a.st + p;
    orbfe_init_result* res = a.res + p;
    __shared__ int s_win;
    if (threadIdx.x == 0) {
        if (pose_base == 0) {
            memset(res, 0, sizeof(*res));
            res->model = 2;
            res->best_h = -1;
            res->best_f = -1;
        }
        int win = -1;
        if (st->branch >= 0)
            for (int m = 0; m < INIT_MAX_MOT && pose_base + m < a.npose; m++)
                if (st->ngood[m] > res->n_good) {
                    res->n_good = st->ngood[m];
                    res->parallax = st->parallax[m];
                    res->best_h = pose_base + m;
                    win = m;
                }
        if (last) {
            res->initialized = st->branch >= 0 && !(res->n_good < 0.7 * st->N);
            if (res->initialized && res->best_h >= 0) {
                for (int i = 0; i < 9; i++) res->R21[i] = a.poses[(size_t)res->best_h * 12 + i];
                for (int i = 0; i < 3; i++) res->t21[i] = a.poses[(size_t)res->best_h * 12 + 9 + i];
            }
        }
        s_win = win;
    }
    __syncthreads();
    if (s_win >= 0) write_points(a, p, a.poses + (size_t)(pose_base + s_win) * 12, a.poses + (size_t)(pose_base + s_win) * 12 + 9, true);
}

// ------------------------------------------------------------------------------------------- host --
thread_local ThreadWorkspaces<HostStage> tl_stages;

// carve the scratch of npairs pairs out of buf
int carve(DevBuf& buf, InitArgs& a, int npairs)
{
    const size_t cap = (size_t)a.capacity, P = (size_t)npairs, it = (size_t)a.iters;
    IoLayout l;
    const size_t o_st = l.take(P * sizeof(PairState)), o_ml = l.take(P * cap * sizeof(int2)), o_pn = l.take(P * 2 * cap * sizeof(float2));
    const size_t o_sets = l.take(P * it * 8 * 4), o_mod = l.take(P * it * 27 * 4), o_sc = l.take(P * 2 * it * 4), o_inl = l.take(P * cap);
    const size_t o_cos = l.take(P * INIT_MAX_MOT * cap * 4);
    int rc = buf.ensure(l.end());
    if (rc) return rc;
    uint8_t* b = buf.as<uint8_t>();
    a.st = (PairState*)(b + o_st);
    a.mlist = (int2*)(b + o_ml);
    a.pn = (float2*)(b + o_pn);
    a.sets = (int32_t*)(b + o_sets);
    a.models = (float*)(b + o_mod);
    a.scores = (float*)(b + o_sc);
    a.inl = b + o_inl;
    a.cosbuf = (float*)(b + o_cos);
    return ORBFE_OK;
}

int launch_main(const InitArgs& a, int npairs, hipStream_t s)
{
    hipLaunchKernelGGL(k_init_prep, dim3(npairs), dim3(64), 0, s, a);
    hipLaunchKernelGGL(k_init_models, dim3((2 * a.iters + 63) / 64, npairs), dim3(64), 0, s, a);
    hipLaunchKernelGGL(k_init_score, dim3(2 * a.iters, npairs), dim3(64), 0, s, a);
    hipLaunchKernelGGL(k_init_select, dim3(npairs), dim3(256), 0, s, a);
    hipLaunchKernelGGL(k_init_checkrt, dim3(8, npairs), dim3(256), 0, s, a, 0);
    hipLaunchKernelGGL(k_init_finalize, dim3(npairs), dim3(256), 0, s, a);
    ORBFE_HIP(hipGetLastError());
    return ORBFE_OK;
}

int check_K(const float* K4, float sigma)
{
    if (!K4 || !(sigma > 0) || !std::isfinite(sigma)) return fail(ORBFE_ERR_INVALID, "orbfe_initialize: invalid K or sigma");
    for (int i = 0; i < 4; i++)
        if (!std::isfinite(K4[i])) return fail(ORBFE_ERR_INVALID, "orbfe_initialize: K is not finite");
    if (K4[0] == 0 || K4[1] == 0) return fail(ORBFE_ERR_INVALID, "orbfe_initialize: fx or fy is 0");
    return ORBFE_OK;
}

// The host-pointer entry points: stage [kps1 | kps2 | n | m12 | words | poses] in one upload, run, download [res | p3d | tri | debug].
struct HostCall {
    const orbfe_keypoint *kps1, *kps2;
    int n1, n2;
    const int32_t* m12;
    const float* K4;
    float sigma;
    int iters;
    const int32_t* words;
    const float* poses;
    int npose;
    orbfe_init_result* res;
    float* p3d;
    uint8_t* tri;
    // debug outputs (orbfe_initialize_inspect), NULL when not wanted
    int32_t* sets;
    float *T12, *pn1, *pn2, *models, *scores;
    int32_t* nmatch;
};

int host_call(const HostCall& c, int device, const char* name)
{
    if (c.n1 < 0 || c.n2 < 0 || !c.res || (c.n1 && (!c.kps1 || !c.m12)) || (c.n2 && !c.kps2) || c.iters <= 0 || c.iters > 100000)
        return fail(ORBFE_ERR_INVALID, "%s: invalid argument", name);
    if (!c.poses && !c.words) return fail(ORBFE_ERR_INVALID, "%s: rand_words is NULL", name);
    int rc = check_K(c.K4, c.sigma);
    if (rc) return rc;
    int N = 0;
    for (int i = 0; i < c.n1; i++) {
        if (c.m12[i] >= c.n2 || c.m12[i] < -1) return fail(ORBFE_ERR_INVALID, "%s: matches12[%d] = %d is not in [-1, n2)", name, i, c.m12[i]);
        N += c.m12[i] >= 0;
    }
    if (c.words)
        for (int i = 0; i < c.iters * 8; i++)
            if (c.words[i] < 0) return fail(ORBFE_ERR_INVALID, "%s: rand_words[%d] is negative (rand() returns 0 .. RAND_MAX)", name, i);
    if ((rc = use_device(device))) return rc;
    HostStage& w = tl_stages.get();
    InitArgs a{};
    a.capacity = std::max(std::max(c.n1, c.n2), 1);
    a.iters = c.iters;
    a.fx = c.K4[0]; a.fy = c.K4[1]; a.cx = c.K4[2]; a.cy = c.K4[3];
    a.sigma = c.sigma;
    a.npose = c.npose;
    const size_t cap = (size_t)a.capacity, nw = c.words ? (size_t)c.iters * 8 : 0, np = c.poses ? (size_t)c.npose * 12 : 0;
    const size_t kb = sizeof(orbfe_keypoint);
    // device io: [kps 2 cap | n | m12 cap | words | poses] [res | p3d 3 cap | tri cap]
    IoLayout l;
    const size_t i_kps = l.take(2 * cap * kb), i_n = l.take(8), i_m = l.take(cap * 4), i_w = l.take(nw * 4), i_p = l.take(np * 4);
    l.outputs();
    const size_t o_res = l.take(sizeof(orbfe_init_result)), o_p3 = l.take(cap * 12), o_tri = l.take(cap);
    if ((rc = w.begin(l)) || (rc = carve(w.host_scratch, a, 1))) return rc;
    const hipStream_t s = w.stream;
    const int32_t nn[2] = {c.n1, c.n2};
    w.put(i_kps, c.kps1, (size_t)c.n1 * kb);
    w.put(i_kps + cap * kb, c.kps2, (size_t)c.n2 * kb);
    w.put(i_n, nn, 8);
    w.put(i_m, c.m12, (size_t)c.n1 * 4);
    w.put(i_w, c.words, nw * 4);
    w.put(i_p, c.poses, np * 4);
    if ((rc = w.upload())) return rc;
    a.kps = w.dev<const orbfe_keypoint>(i_kps); a.nk = w.dev<const int32_t>(i_n); a.m12 = w.dev<const int32_t>(i_m);
    a.words = nw ? w.dev<const int32_t>(i_w) : nullptr;
    a.poses = np ? w.dev<const float>(i_p) : nullptr;
    a.res = w.dev<orbfe_init_result>(o_res); a.p3d = w.dev<float>(o_p3); a.tri = w.dev<uint8_t>(o_tri);
    if (c.poses) {
        // InitializeUseAruco: the words are not used; prep compacts and normalises (normalisation is not used either)
        InitArgs a0 = a;
        a0.iters = 0;
        hipLaunchKernelGGL(k_init_prep, dim3(1), dim3(64), 0, s, a0);
        for (int base = 0; base < c.npose; base += INIT_MAX_MOT) {
            hipLaunchKernelGGL(k_init_checkrt, dim3(INIT_MAX_MOT, 1), dim3(256), 0, s, a, base);
            hipLaunchKernelGGL(k_init_poses_fold, dim3(1), dim3(256), 0, s, a, base, base + INIT_MAX_MOT >= c.npose ? 1 : 0);
        }
        ORBFE_HIP(hipGetLastError());
    } else if ((rc = launch_main(a, 1, s))) {
        return rc;
    }
    if ((rc = w.download())) return rc;
    if (c.sets) {
        // orbfe_initialize_inspect: the intermediate results, straight from the scratch
        const uint8_t* st0 = (const uint8_t*)a.st;
        static_assert(offsetof(PairState, T2) == offsetof(PairState, T1) + 36, "T1, T2 adjacent");
        ORBFE_HIP(hipMemcpyAsync(c.T12, st0 + offsetof(PairState, T1), 72, hipMemcpyDeviceToHost, s));
        ORBFE_HIP(hipMemcpyAsync(c.nmatch, st0 + offsetof(PairState, N), 4, hipMemcpyDeviceToHost, s));
        if (N >= 8) {
            ORBFE_HIP(hipMemcpyAsync(c.sets, a.sets, (size_t)c.iters * 32, hipMemcpyDeviceToHost, s));
            ORBFE_HIP(hipMemcpyAsync(c.models, a.models, (size_t)c.iters * 27 * 4, hipMemcpyDeviceToHost, s));
            ORBFE_HIP(hipMemcpyAsync(c.scores, a.scores, (size_t)c.iters * 8, hipMemcpyDeviceToHost, s));
        }
        if (c.n1) ORBFE_HIP(hipMemcpyAsync(c.pn1, a.pn, (size_t)c.n1 * 8, hipMemcpyDeviceToHost, s));
        if (c.n2) ORBFE_HIP(hipMemcpyAsync(c.pn2, a.pn + cap, (size_t)c.n2 * 8, hipMemcpyDeviceToHost, s));
    }
    if ((rc = w.sync())) return rc;
    const orbfe_init_result* r = w.host<const orbfe_init_result>(o_res);
    *c.res = *r;
    // p3d / triangulated: written only where the reference assigns vP3D / vbTriangulated
    const bool wrote = c.poses ? r->best_h >= 0 : r->initialized != 0;
    if (wrote && c.n1) {
        if (c.p3d) memcpy(c.p3d, w.host<uint8_t>(o_p3), (size_t)c.n1 * 12);
        if (c.tri) memcpy(c.tri, w.host<uint8_t>(o_tri), (size_t)c.n1);
    }
    return ORBFE_OK;
}

// the fields every public wrapper sets
HostCall pair_call(const orbfe_keypoint* kps1, int n1, const orbfe_keypoint* kps2, int n2, const int32_t* m12, const float* K4, float sigma,
                   int iters, orbfe_init_result* res)
{
    HostCall c{};
    c.kps1 = kps1; c.kps2 = kps2; c.n1 = n1; c.n2 = n2; c.m12 = m12; c.K4 = K4; c.sigma = sigma; c.iters = iters; c.res = res;
    return c;
}

} // namespace
} // namespace orbfe

using namespace orbfe;

int orbfe_initialize(const orbfe_keypoint* kps1, int n1, const orbfe_keypoint* kps2, int n2, const int32_t* matches12, const float* K4,
                     float sigma, int iterations, const int32_t* rand_words, orbfe_init_result* res, float* p3d, uint8_t* triangulated,
                     int device)
{
    HostCall c = pair_call(kps1, n1, kps2, n2, matches12, K4, sigma, iterations, res);
    c.words = rand_words; c.p3d = p3d; c.tri = triangulated;
    return host_call(c, device, "orbfe_initialize");
}

int orbfe_initialize_inspect(const orbfe_keypoint* kps1, int n1, const orbfe_keypoint* kps2, int n2, const int32_t* matches12,
                             const float* K4, float sigma, int iterations, const int32_t* rand_words, orbfe_init_result* res,
                             int32_t* nmatches, int32_t* sets, float* T12, float* pn1, float* pn2, float* models, float* scores, int device)
{
    if (!nmatches || !sets || !T12 || (n1 > 0 && !pn1) || (n2 > 0 && !pn2) || !models || !scores)
        return fail(ORBFE_ERR_INVALID, "orbfe_initialize_inspect: null output");
    HostCall c = pair_call(kps1, n1, kps2, n2, matches12, K4, sigma, iterations, res);
    c.words = rand_words;
    c.sets = sets; c.T12 = T12; c.pn1 = pn1; c.pn2 = pn2; c.models = models; c.scores = scores; c.nmatch = nmatches;
    return host_call(c, device, "orbfe_initialize_inspect");
}

int orbfe_initialize_check_poses(const orbfe_keypoint* kps1, int n1, const orbfe_keypoint* kps2, int n2, const int32_t* matches12,
                                 const float* K4, float sigma, const float* poses, int npose, orbfe_init_result* res, float* p3d,
                                 uint8_t* triangulated, int device)
{
    if (npose < 0 || (npose > 0 && !poses) || !res) return fail(ORBFE_ERR_INVALID, "orbfe_initialize_check_poses: invalid argument");
    if (npose == 0) {
        // InitializeUseAruco returns false at once when R21 is empty
        if (n1 < 0 || n2 < 0) return fail(ORBFE_ERR_INVALID, "orbfe_initialize_check_poses: invalid argument");
        memset(res, 0, sizeof(*res));
        res->model = 2;
        res->best_h = res->best_f = -1;
        return ORBFE_OK;
    }
    for (int i = 0; i < npose * 12; i++)
        if (!std::isfinite(poses[i])) return fail(ORBFE_ERR_INVALID, "orbfe_initialize_check_poses: pose %d is not finite", i / 12);
    HostCall c = pair_call(kps1, n1, kps2, n2, matches12, K4, sigma, 1, res);
    c.poses = poses; c.npose = npose; c.p3d = p3d; c.tri = triangulated;
    return host_call(c, device, "orbfe_initialize_check_poses");
}

int orbfe_initialize_batch_device(const orbfe_keypoint* d_kps, const int32_t* d_n, int capacity, int npairs, const int32_t* d_matches12,
                                  const float* K4, float sigma, int iterations, const int32_t* d_rand_words, orbfe_init_result* d_res,
                                  float* d_p3d, uint8_t* d_triangulated, void* stream)
{
    if (!d_kps || !d_n || !d_matches12 || !d_rand_words || !d_res || !d_p3d || !d_triangulated || capacity <= 0 || npairs <= 0 ||
        iterations <= 0 || iterations > 100000)
        return fail(ORBFE_ERR_INVALID, "orbfe_initialize_batch_device: invalid argument");
    int rc = check_K(K4, sigma);
    if (rc) return rc;
    const hipStream_t s = (hipStream_t)stream;
    HostStage& w = tl_stages.get(s);
    InitArgs a{};
    a.kps = d_kps; a.nk = d_n; a.m12 = d_matches12; a.words = d_rand_words;
    a.capacity = capacity; a.iters = iterations;
    a.fx = K4[0]; a.fy = K4[1]; a.cx = K4[2]; a.cy = K4[3];
    a.sigma = sigma;
    a.res = d_res; a.p3d = d_p3d; a.tri = d_triangulated;
    if ((rc = carve(w.scratch, a, npairs))) return rc;
    return launch_main(a, npairs, s);
}
