// new_map_points.hip -- the geometry of LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:222-467, monocular) on gfx950.
//
//   k_nmp_prepare      1 workgroup per (current keyframe, neighbour): camera centres, baseline, ComputeSceneMedianDepth(2) of the
//                      neighbour (radix select on order-preserving keys in LDS), the baseline / depth gate, ComputeF12, the epipole
//   k_nmp_triangulate  1 thread per side-1 feature of a pair: the parallax gate, the 4 x 4 DLT (svd_jacobi.hpp), the cheirality,
//                      chi-square and scale gates, UpdateNormalAndDepth of the new point, the map state in place
// The chain of the product call is prepare once, then per pair the search (bow_vocabulary.hip) and the triangulation, all on one stream.
// The numerics restate OpenCV 3.4 for CV_32F, as initializer.hip does: Mat products and dots accumulate in double and round once,
// cv::norm is a double sum and a double square root, 3 x 3 inverses are cofactor formulas in double.
#include "host_stage.hpp"
#include "new_points_plan.hpp"
#include "orbfe_common.hpp"
#include "ransac_sets.hpp"
#include "svd_jacobi.hpp"
#include <cfloat>
#include <cmath>

namespace orbfe {
namespace {

// C = A * B (3 x 3, row-major): double sums in k order, one rounding
__device__ __forceinline__ void nmp_mm3(const float* A, const float* B, float* C)
{
    float R[9];
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 3; c++) {
            double s = 0;
#pragma unroll
            for (int k = 0; k < 3; k++) s += (double)A[r * 3 + k] * B[k * 3 + c];
            R[r * 3 + c] = (float)s;
        }
#pragma unroll
    for (int i = 0; i < 9; i++) C[i] = R[i];
}

// Mat::inv() (DECOMP_LU) for 3 x 3 float: the cofactor formula in double; a singular matrix gives zeros
__device__ __forceinline__ void nmp_inv3(const float* S, float* D)
{
    double d = S[0] * ((double)S[4] * S[8] - (double)S[5] * S[7]) - S[1] * ((double)S[3] * S[8] - (double)S[5] * S[6]) +
               S[2] * ((double)S[3] * S[7] - (double)S[4] * S[6]);
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

// Ow = -Rwc * tcw (KeyFrame::SetPose): a product with alpha = -1, T = [R | t] 3 x 4 row-major
__device__ __forceinline__ void nmp_centre(const float* T, float* O)
{
#pragma unroll
    for (int r = 0; r < 3; r++) {
        double s = 0;
#pragma unroll
        for (int k = 0; k < 3; k++) s += (double)T[k * 4 + r] * T[k * 4 + 3];
        O[r] = (float)(s * -1.0);
    }
}

__device__ __forceinline__ float nmp_norm3(float x, float y, float z) { return (float)sqrt((double)x * x + (double)y * y + (double)z * z); }

__device__ __forceinline__ uint32_t nmp_order_key(float f)
{
    const uint32_t b = __float_as_uint(f);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

struct NmpPrepArgs {
    const int32_t* nk;
    int capacity;
    const float* x3Dw;
    const uint8_t* valid;   // may be NULL: every feature has a map point
    const float* Tcw;
    const int32_t *pair1, *pair2;
    float fx, fy, cx, cy;
    float* F12;
    float* epipole;
    orbfe_new_points_pair* prep;
};

__global__ __launch_bounds__(NMP_THREADS) void k_nmp_prepare(NmpPrepArgs a)
{
    const int p = blockIdx.x, cap = a.capacity;
    const int f1 = a.pair1 ? a.pair1[p] : p, f2 = a.pair2 ? a.pair2[p] : p + 1;
    const int n2 = clampn(a.nk[f2], cap);
    __shared__ float s_z[NMP_MAX_CAPACITY];
    __shared__ uint32_t hist[256];
    __shared__ int s_m, s_k;
    __shared__ uint32_t s_prefix;
    float T1[12], T2[12];
#pragma unroll
    for (int i = 0; i < 12; i++) { T1[i] = a.Tcw[(size_t)f1 * 12 + i]; T2[i] = a.Tcw[(size_t)f2 * 12 + i]; }
    if (threadIdx.x == 0) s_m = 0;
    __syncthreads();
    // KeyFrame::ComputeSceneMedianDepth(2): z = Rcw2.dot(x3Dw) + zcw, the dot in double
    const float* X = a.x3Dw + (size_t)f2 * cap * 3;
    const uint8_t* valid = a.valid ? a.valid + (size_t)f2 * cap : nullptr;
    for (int i = threadIdx.x; i < n2; i += NMP_THREADS) {
        if (valid && !valid[i]) continue;
        const double d = (double)T2[8] * X[3 * i] + (double)T2[9] * X[3 * i + 1] + (double)T2[10] * X[3 * i + 2];
        s_z[atomicAdd(&s_m, 1)] = (float)(d + (double)T2[11]);
    }
    __syncthreads();
    const int m = s_m;
    // the (m - 1) / 2-th smallest: radix select, 8 bits per pass, on order-preserving keys
    uint32_t prefix = 0;
    int k = (m - 1) / 2;
    if (m > 0) {
        for (int shift = 24; shift >= 0; shift -= 8) {
            for (int b = threadIdx.x; b < 256; b += NMP_THREADS) hist[b] = 0;
            __syncthreads();
            const uint32_t hmask = shift == 24 ? 0u : ~0u << (shift + 8);
            for (int i = threadIdx.x; i < m; i += NMP_THREADS) {
                const uint32_t key = nmp_order_key(s_z[i]);
                if ((key & hmask) == prefix) atomicAdd(&hist[(key >> shift) & 255u], 1u);
            }
            __syncthreads();
            if (threadIdx.x == 0) {
                int b = 0, kk = k;
                while (b < 255 && (int)hist[b] <= kk) { kk -= (int)hist[b]; b++; }
                s_prefix = prefix | ((uint32_t)b << shift);
                s_k = kk;
            }
            __syncthreads();
            prefix = s_prefix;
            k = s_k;
            __syncthreads();
        }
    }
    if (threadIdx.x != 0) return;
    float O1[3], O2[3];
    nmp_centre(T1, O1);
    nmp_centre(T2, O2);
    orbfe_new_points_pair rec;
    rec.baseline = nmp_norm3(O2[0] - O1[0], O2[1] - O1[1], O2[2] - O1[2]);
    rec.median_depth = m > 0 ? __uint_as_float((prefix & 0x80000000u) ? (prefix & 0x7fffffffu) : ~prefix) : 0.f;
    rec.n_depths = m;
    const float ratio = rec.baseline / rec.median_depth;
    rec.skipped = (m == 0 || (double)ratio < 0.01) ? 1 : 0;
    a.prep[p] = rec;
    float F[9], e[2];
    if (rec.skipped) {
#pragma unroll
        for (int i = 0; i < 9; i++) F[i] = 0;
        e[0] = e[1] = 0;
    } else {
        // ComputeF12 (:904-921)
        float R1[9], R2t[9], R12[9], M[9], t12[3];
#pragma unroll
        for (int r = 0; r < 3; r++)
#pragma unroll
            for (int c = 0; c < 3; c++) { R1[r * 3 + c] = T1[r * 4 + c]; R2t[r * 3 + c] = T2[c * 4 + r]; }
        nmp_mm3(R1, R2t, R12);
#pragma unroll
        for (int r = 0; r < 3; r++)
#pragma unroll
            for (int c = 0; c < 3; c++) {   // -R1w * R2w.t(): the same sums with alpha = -1
                double s = 0;
#pragma unroll
                for (int kk = 0; kk < 3; kk++) s += (double)R1[r * 3 + kk] * R2t[kk * 3 + c];
                M[r * 3 + c] = (float)(s * -1.0);
            }
#pragma unroll
        for (int r = 0; r < 3; r++) {       // (...) * t2w + t1w: one gemm, the addend inside the rounding
            double s = 0;
#pragma unroll
            for (int kk = 0; kk < 3; kk++) s += (double)M[r * 3 + kk] * T2[kk * 4 + 3];
            t12[r] = (float)(s + (double)T1[r * 4 + 3]);
        }
        const float t12x[9] = {0, -t12[2], t12[1], t12[2], 0, -t12[0], -t12[1], t12[0], 0};
        const float Kt[9] = {a.fx, 0, 0, 0, a.fy, 0, a.cx, a.cy, 1}, K[9] = {a.fx, 0, a.cx, 0, a.fy, a.cy, 0, 0, 1};
        float Kti[9], Ki[9], A[9];
        nmp_inv3(Kt, Kti);
        nmp_inv3(K, Ki);
        nmp_mm3(Kti, t12x, A);
        nmp_mm3(A, R12, A);
        nmp_mm3(A, Ki, F);
        // the epipole in the neighbour's image (ORBmatcher.cc:668-674)
        float C2[3];
#pragma unroll
        for (int r = 0; r < 3; r++) {
            double s = 0;
#pragma unroll
            for (int kk = 0; kk < 3; kk++) s += (double)T2[r * 4 + kk] * O1[kk];
            C2[r] = (float)(s + (double)T2[r * 4 + 3]);
        }
        const float invz = 1.0f / C2[2];
        e[0] = a.fx * C2[0] * invz + a.cx;
        e[1] = a.fy * C2[1] * invz + a.cy;
    }
#pragma unroll
    for (int i = 0; i < 9; i++) a.F12[(size_t)p * 9 + i] = F[i];
    a.epipole[(size_t)p * 2] = e[0];
    a.epipole[(size_t)p * 2 + 1] = e[1];
}

struct NmpTriArgs {
    const orbfe_keypoint* kps;
    const int32_t* nk;
    int capacity;
    float* x3Dw;       // the map state: all three or none
    uint8_t* valid;
    uint8_t* free_;
    const float* Tcw;
    const int32_t *pair1, *pair2;
    const int32_t* m12;
    float fx, fy, cx, cy;
    float scale[NMP_MAX_LEVELS], sigma2[NMP_MAX_LEVELS];
    int nlevels;
    float ratio;
    uint8_t* status;
    float *x3D, *normal, *dist, *inspect;
    orbfe_new_points_result* res;
};

struct NmpPoint {
    int status;
    float X[3], normal[3], dmax, dmin;
    float q[NMP_INSPECT_FLOATS];
};

// lines :306-446 for one match, then UpdateNormalAndDepth (MapPoint.cc:359-400)
__device__ __forceinline__ void nmp_point(const float* T1, const float* O1, const float* T2, const float* O2, float fx, float fy, float cx,
                                          float cy, float k1x, float k1y, float k2x, float k2y, float sig1, float sig2, float sf1, float sf2,
                                          float sf_last, float ratio_factor, NmpPoint& r)
{
#pragma unroll
    for (int i = 0; i < NMP_INSPECT_FLOATS; i++) r.q[i] = 0;
    const float invfx = 1.0f / fx, invfy = 1.0f / fy;
    const float xn1[3] = {(k1x - cx) * invfx, (k1y - cy) * invfy, 1.0f}, xn2[3] = {(k2x - cx) * invfx, (k2y - cy) * invfy, 1.0f};
    float ray1[3], ray2[3];
#pragma unroll
    for (int i = 0; i < 3; i++) {   // Rwc * xn
        ray1[i] = (float)((double)T1[i] * xn1[0] + (double)T1[4 + i] * xn1[1] + (double)T1[8 + i] * xn1[2]);
        ray2[i] = (float)((double)T2[i] * xn2[0] + (double)T2[4 + i] * xn2[1] + (double)T2[8 + i] * xn2[2]);
    }
    const double dot = (double)ray1[0] * ray2[0] + (double)ray1[1] * ray2[1] + (double)ray1[2] * ray2[2];
    const double nr1 = sqrt((double)ray1[0] * ray1[0] + (double)ray1[1] * ray1[1] + (double)ray1[2] * ray1[2]);
    const double nr2 = sqrt((double)ray2[0] * ray2[0] + (double)ray2[1] * ray2[1] + (double)ray2[2] * ray2[2]);
    const float cosv = (float)(dot / (nr1 * nr2));
    r.q[0] = cosv;
    if (!(cosv > 0 && (double)cosv < 0.9998)) { r.status = ORBFE_NMP_PARALLAX; return; }
    float At[4][4], W[4], Vt[4][4];
#pragma unroll
    for (int c = 0; c < 4; c++) {   // A rows, stored transposed
        At[c][0] = (float)((double)T1[8 + c] * xn1[0] - (double)T1[c]);
        At[c][1] = (float)((double)T1[8 + c] * xn1[1] - (double)T1[4 + c]);
        At[c][2] = (float)((double)T2[8 + c] * xn2[0] - (double)T2[c]);
        At[c][3] = (float)((double)T2[8 + c] * xn2[1] - (double)T2[4 + c]);
    }
    svd_jacobi<4, 4, 4, false>(At, W, Vt);
    if (Vt[3][3] == 0) { r.status = ORBFE_NMP_W_ZERO; return; }
    const float iw = (float)(1. / (double)Vt[3][3]);
    const float X = Vt[3][0] * iw, Y = Vt[3][1] * iw, Z = Vt[3][2] * iw;
    if (!isfinite(X) || !isfinite(Y) || !isfinite(Z)) { r.status = ORBFE_NMP_NOT_FINITE; return; }
    r.X[0] = X; r.X[1] = Y; r.X[2] = Z;
    float c1[3], c2[3];
#pragma unroll
    for (int i = 0; i < 3; i++) {
        c1[i] = (float)((double)T1[i * 4] * X + (double)T1[i * 4 + 1] * Y + (double)T1[i * 4 + 2] * Z + (double)T1[i * 4 + 3]);
        c2[i] = (float)((double)T2[i * 4] * X + (double)T2[i * 4 + 1] * Y + (double)T2[i * 4 + 2] * Z + (double)T2[i * 4 + 3]);
    }
    if (c1[2] <= 0) { r.status = ORBFE_NMP_Z1; return; }
    if (c2[2] <= 0) { r.status = ORBFE_NMP_Z2; return; }
    const float invz1 = (float)(1.0 / (double)c1[2]);
    const float u1 = fx * c1[0] * invz1 + cx, v1 = fy * c1[1] * invz1 + cy;
    const float ex1 = u1 - k1x, ey1 = v1 - k1y;
    const float e1 = ex1 * ex1 + ey1 * ey1;
    r.q[1] = e1;
    if ((double)e1 > 5.991 * (double)sig1) { r.status = ORBFE_NMP_REPROJECTION1; return; }
    const float invz2 = (float)(1.0 / (double)c2[2]);
    const float u2 = fx * c2[0] * invz2 + cx, v2 = fy * c2[1] * invz2 + cy;
    const float ex2 = u2 - k2x, ey2 = v2 - k2y;
    const float e2 = ex2 * ex2 + ey2 * ey2;
    r.q[2] = e2;
    if ((double)e2 > 5.991 * (double)sig2) { r.status = ORBFE_NMP_REPROJECTION2; return; }
    const float n1[3] = {X - O1[0], Y - O1[1], Z - O1[2]}, n2[3] = {X - O2[0], Y - O2[1], Z - O2[2]};
    const double d1 = sqrt((double)n1[0] * n1[0] + (double)n1[1] * n1[1] + (double)n1[2] * n1[2]);
    const double d2 = sqrt((double)n2[0] * n2[0] + (double)n2[1] * n2[1] + (double)n2[2] * n2[2]);
    const float dist1 = (float)d1, dist2 = (float)d2;
    r.q[3] = dist1; r.q[4] = dist2;
    if (dist1 == 0 || dist2 == 0) { r.status = ORBFE_NMP_ZERO_DISTANCE; return; }
    const float ratioDist = dist2 / dist1, ratioOctave = sf1 / sf2;
    r.q[5] = ratioOctave;
    if (ratioDist * ratio_factor < ratioOctave || ratioDist > ratioOctave * ratio_factor) { r.status = ORBFE_NMP_SCALE; return; }
    // UpdateNormalAndDepth: normal = (n1 / |n1| + n2 / |n2|) / 2, "m / s" = m * (float)(1. / s)
    const float a1 = (float)(1. / d1), a2 = (float)(1. / d2);
#pragma unroll
    for (int i = 0; i < 3; i++) r.normal[i] = ((0.f + n1[i] * a1) + n2[i] * a2) * 0.5f;
    r.dmax = dist1 * sf1;
    r.dmin = r.dmax / sf_last;
    r.status = ORBFE_NMP_CREATED;
}

__global__ __launch_bounds__(NMP_THREADS) void k_nmp_triangulate(NmpTriArgs a)
{
    const int p = blockIdx.y, cap = a.capacity;
    const int f1 = a.pair1 ? a.pair1[p] : p, f2 = a.pair2 ? a.pair2[p] : p + 1;
    const int n1 = clampn(a.nk[f1], cap), n2 = clampn(a.nk[f2], cap);
    if (blockIdx.x != 0 && (int)(blockIdx.x * NMP_THREADS) >= n1) return;
    // a per-lane index into a kernel argument array would go through scratch: the level tables live in LDS
    __shared__ float s_scale[NMP_MAX_LEVELS], s_sigma2[NMP_MAX_LEVELS];
    if (threadIdx.x < NMP_MAX_LEVELS) { s_scale[threadIdx.x] = a.scale[threadIdx.x]; s_sigma2[threadIdx.x] = a.sigma2[threadIdx.x]; }
    const orbfe_keypoint *k1 = a.kps + (size_t)f1 * cap, *k2 = a.kps + (size_t)f2 * cap;
    const int32_t* m12 = a.m12 + (size_t)p * cap;
    // an octave outside the tables anywhere in the pair: every workgroup of the pair finds it and leaves
    int bad = 0;
    for (int i = threadIdx.x; i < n1; i += NMP_THREADS) {
        const int j = m12[i];
        if (j < 0 || j >= n2) continue;
        const int o1 = k1[i].octave, o2 = k2[j].octave;
        if (o1 < 0 || o1 >= a.nlevels || o2 < 0 || o2 >= a.nlevels) bad = 1;
    }
    bad = __syncthreads_or(bad);   // also the barrier behind the LDS tables
    if (bad) {
        if (blockIdx.x == 0 && threadIdx.x == 0) a.res[p].status = ORBFE_ERR_INVALID;
        return;
    }
    const int i1 = blockIdx.x * NMP_THREADS + threadIdx.x;
    int i2 = -1;
    if (i1 < n1) {
        i2 = m12[i1];
        if (i2 < 0 || i2 >= n2) i2 = -1;
    }
    NmpPoint r;
    r.status = ORBFE_NMP_NO_MATCH;
    if (i2 >= 0) {
        float T1[12], T2[12], O1[3], O2[3];
#pragma unroll
        for (int i = 0; i < 12; i++) { T1[i] = a.Tcw[(size_t)f1 * 12 + i]; T2[i] = a.Tcw[(size_t)f2 * 12 + i]; }
        nmp_centre(T1, O1);
        nmp_centre(T2, O2);
        const orbfe_keypoint kp1 = k1[i1], kp2 = k2[i2];
        nmp_point(T1, O1, T2, O2, a.fx, a.fy, a.cx, a.cy, kp1.x, kp1.y, kp2.x, kp2.y, s_sigma2[kp1.octave], s_sigma2[kp2.octave],
                  s_scale[kp1.octave], s_scale[kp2.octave], s_scale[a.nlevels - 1], a.ratio, r);
    }
    const size_t slot = (size_t)p * cap + i1;
    if (i1 < n1) {
        a.status[slot] = (uint8_t)r.status;
        if (a.inspect)
#pragma unroll
            for (int i = 0; i < NMP_INSPECT_FLOATS; i++) a.inspect[slot * NMP_INSPECT_FLOATS + i] = i2 >= 0 ? r.q[i] : 0.f;
    }
    const bool created = r.status == ORBFE_NMP_CREATED;
    if (created) {
#pragma unroll
        for (int i = 0; i < 3; i++) { a.x3D[slot * 3 + i] = r.X[i]; a.normal[slot * 3 + i] = r.normal[i]; }
        a.dist[slot * 2] = r.dmax;
        a.dist[slot * 2 + 1] = r.dmin;
        if (a.x3Dw) {
            const size_t s1 = (size_t)f1 * cap + i1, s2 = (size_t)f2 * cap + i2;
            a.free_[s1] = 0; a.free_[s2] = 0;
            a.valid[s1] = 1; a.valid[s2] = 1;
#pragma unroll
            for (int i = 0; i < 3; i++) { a.x3Dw[s1 * 3 + i] = r.X[i]; a.x3Dw[s2 * 3 + i] = r.X[i]; }
        }
    }
    // the pair's counts: a wave reduction, then one atomic per wave and count
    const int nm = __popcll(__ballot(i2 >= 0)), nn = __popcll(__ballot(created));
    if ((threadIdx.x & 63) == 0) {
        if (nm) atomicAdd(&a.res[p].n_matches, nm);
        if (nn) atomicAdd(&a.res[p].n_new, nn);
    }
}

// ------------------------------------------------------------------------------------------- host --
int report(const NmpCheck& c) { return c.err ? fail(c.err, "%s", c.msg) : ORBFE_OK; }

int launch_prepare(const NmpPrepArgs& a, int npairs, hipStream_t s)
{
    const NmpGrid g = nmp_prepare_grid(npairs);
    hipLaunchKernelGGL(k_nmp_prepare, dim3(g.x, g.y), dim3(g.block), 0, s, a);
    ORBFE_HIP(hipGetLastError());
    return ORBFE_OK;
}

// the pair records are zero before the launch: the counts are summed into them
int launch_triangulate(const NmpTriArgs& a, int npairs, hipStream_t s)
{
    const NmpGrid g = nmp_triangulate_grid(a.capacity, npairs);
    hipLaunchKernelGGL(k_nmp_triangulate, dim3(g.x, g.y), dim3(g.block), 0, s, a);
    ORBFE_HIP(hipGetLastError());
    return ORBFE_OK;
}

NmpTriArgs tri_args(const orbfe_keypoint* d_kps, const int32_t* d_n, int capacity, float* d_x3Dw, uint8_t* d_valid, uint8_t* d_free,
                    const float* d_Tcw, const int32_t* d_pair1, const int32_t* d_pair2, const int32_t* d_match12, const float* K4,
                    const float* scale_factors, const float* level_sigma2, int nlevels, float ratio_factor, uint8_t* d_status, float* d_x3D,
                    float* d_normal, float* d_dist, float* d_inspect, orbfe_new_points_result* d_res)
{
    NmpTriArgs a{};
    a.kps = d_kps; a.nk = d_n; a.capacity = capacity; a.x3Dw = d_x3Dw; a.valid = d_valid; a.free_ = d_free; a.Tcw = d_Tcw;
    a.pair1 = d_pair1; a.pair2 = d_pair2; a.m12 = d_match12;
    a.fx = K4[0]; a.fy = K4[1]; a.cx = K4[2]; a.cy = K4[3];
    for (int l = 0; l < NMP_MAX_LEVELS; l++) { a.scale[l] = scale_factors[std::min(l, nlevels - 1)]; a.sigma2[l] = level_sigma2[std::min(l, nlevels - 1)]; }
    a.nlevels = nlevels; a.ratio = ratio_factor;
    a.status = d_status; a.x3D = d_x3D; a.normal = d_normal; a.dist = d_dist; a.inspect = d_inspect; a.res = d_res;
    return a;
}

int check_triangulate(const char* name, const orbfe_keypoint* d_kps, const int32_t* d_n, int capacity, const float* d_x3Dw, const uint8_t* d_valid,
                      const uint8_t* d_free, const float* d_Tcw, const int32_t* d_pair1, const int32_t* d_pair2, int npairs,
                      const int32_t* d_match12, const float* K4, const float* scale_factors, const float* level_sigma2, int nlevels,
                      float ratio_factor, const uint8_t* d_status, const float* d_x3D, const float* d_normal, const float* d_dist,
                      const orbfe_new_points_result* d_res)
{
    if (!d_kps || !d_n || !d_Tcw || !d_match12 || !d_status || !d_x3D || !d_normal || !d_dist || !d_res)
        return fail(ORBFE_ERR_INVALID, "%s: invalid argument", name);
    const int given = (d_x3Dw != nullptr) + (d_valid != nullptr) + (d_free != nullptr);
    if (given != 0 && given != 3) return fail(ORBFE_ERR_INVALID, "%s: d_x3Dw, d_valid and d_free are all given or all NULL", name);
    int rc = report(nmp_check_common(name, capacity, npairs, d_pair1, d_pair2, K4));
    if (rc) return rc;
    return report(nmp_check_levels(name, scale_factors, level_sigma2, nlevels, ratio_factor));
}

// one pair through the stage: what orbfe_create_new_map_points and orbfe_new_points_inspect share
struct NmpHostSide {
    const orbfe_keypoint* kps; const uint8_t* desc; int n;
    const uint32_t* fv_node; const int32_t* fv_offset; const uint32_t* fv_feature; int nfv;
    float* x3Dw; uint8_t* valid; const float* Tcw;
};

int host_pair(const char* name, const NmpHostSide (&f)[2], bool search, const int32_t* match12_in, const float* K4, const float* scale_factors,
              const float* level_sigma2, int nlevels, float ratio_factor, int check_orientation, float* F12, float* epipole,
              orbfe_new_points_pair* prep, int32_t* match12, uint8_t* status, float* x3D, float* normal, float* dist, float* quantities,
              orbfe_new_points_result* res, int device)
{
    const int n1 = f[0].n, n2 = f[1].n;
    if (n1 < 0 || n2 < 0 || !res || !f[0].Tcw || !f[1].Tcw || (n1 && (!f[0].kps || !status || !x3D || !normal || !dist)) || (n2 && !f[1].kps))
        return fail(ORBFE_ERR_INVALID, "%s: invalid argument", name);
    if (search) {
        if (!F12 || !epipole || !prep || (n1 && !match12)) return fail(ORBFE_ERR_INVALID, "%s: invalid argument", name);
        for (int k = 0; k < 2; k++) {
            if (f[k].nfv < 0 || f[k].nfv > f[k].n || (f[k].n && (!f[k].desc || !f[k].x3Dw || !f[k].valid)) ||
                (f[k].nfv && (!f[k].fv_node || !f[k].fv_offset || !f[k].fv_feature)))
                return fail(ORBFE_ERR_INVALID, "%s: invalid argument", name);
            if (f[k].nfv && (f[k].fv_offset[0] != 0 || f[k].fv_offset[f[k].nfv] > f[k].n))
                return fail(ORBFE_ERR_INVALID, "%s: bad FeatureVector %d", name, k + 1);
        }
    } else if ((n1 && !match12_in) || (n1 && !quantities)) {
        return fail(ORBFE_ERR_INVALID, "%s: invalid argument", name);
    }
    const int cap = std::max(1, std::max(n1, n2));
    int rc = report(nmp_check_common(name, cap, 1, nullptr, nullptr, K4));
    if (rc || (rc = report(nmp_check_levels(name, scale_factors, level_sigma2, nlevels, ratio_factor)))) return rc;
    if ((rc = use_device(device))) return rc;
    HostStage& w = match_host_stage();
    const NmpHostLayout l = nmp_host_layout(cap, search, !search);
    if ((rc = w.begin(l.io))) return rc;
    const size_t C = (size_t)cap, kb = sizeof(orbfe_keypoint);
    memset(w.host<uint8_t>(0), 0, l.io.split);
    const int32_t nn[2] = {n1, n2}, nf[2] = {f[0].nfv, f[1].nfv};
    w.put(l.n, nn, 8);
    if (search) w.put(l.nf, nf, 8);
    for (size_t k = 0; k < 2; k++) {
        const size_t n = (size_t)f[k].n;
        w.put(l.kps + k * C * kb, f[k].kps, n * kb);
        w.put(l.tcw + k * 48, f[k].Tcw, 48);
        if (!search) continue;
        w.put(l.desc + k * C * 32, f[k].desc, n * 32);
        w.put(l.fn + k * C * 4, f[k].fv_node, (size_t)f[k].nfv * 4);
        if (f[k].nfv) {
            w.put(l.fo + k * (C + 1) * 4, f[k].fv_offset, (size_t)(f[k].nfv + 1) * 4);
            w.put(l.ff + k * C * 4, f[k].fv_feature, (size_t)f[k].fv_offset[f[k].nfv] * 4);
        }
        w.put(l.x3Dw + k * C * 12, f[k].x3Dw, n * 12);
        uint8_t *v = w.host<uint8_t>(l.valid) + k * C, *fr = w.host<uint8_t>(l.free_) + k * C;
        for (size_t i = 0; i < n; i++) { v[i] = f[k].valid[i] != 0; fr[i] = !v[i]; }
    }
    // the inspect call: its match list goes up in the (download) block of m12 by a copy of its own
    if (!search) w.put(l.m12, match12_in, (size_t)n1 * 4);
    if ((rc = w.upload())) return rc;
    if (search) {
        rc = orbfe_create_new_map_points_device(
            w.dev<orbfe_keypoint>(l.kps), w.dev<uint8_t>(l.desc), w.dev<int32_t>(l.n), w.dev<uint32_t>(l.fn), w.dev<int32_t>(l.fo),
            w.dev<uint32_t>(l.ff), w.dev<int32_t>(l.nf), cap, w.dev<float>(l.x3Dw), w.dev<uint8_t>(l.valid), w.dev<uint8_t>(l.free_),
            w.dev<float>(l.tcw), nullptr, nullptr, 1, K4, scale_factors, level_sigma2, nlevels, ratio_factor, check_orientation,
            w.dev<float>(l.F12), w.dev<float>(l.epipole), w.dev<orbfe_new_points_pair>(l.prep), w.dev<int32_t>(l.m12), w.dev<int32_t>(l.m21),
            w.dev<int32_t>(l.nm), w.dev<uint8_t>(l.status), w.dev<float>(l.x3D), w.dev<float>(l.normal), w.dev<float>(l.dist),
            w.dev<orbfe_new_points_result>(l.res), w.stream);
    } else {
        ORBFE_HIP(hipMemcpyAsync(w.dev<int32_t>(l.m12), w.host<int32_t>(l.m12), C * 4, hipMemcpyHostToDevice, w.stream));
        ORBFE_HIP(hipMemsetAsync(w.dev<uint8_t>(l.res), 0, sizeof(orbfe_new_points_result), w.stream));
        rc = launch_triangulate(tri_args(w.dev<orbfe_keypoint>(l.kps), w.dev<int32_t>(l.n), cap, nullptr, nullptr, nullptr, w.dev<float>(l.tcw),
                                         nullptr, nullptr, w.dev<int32_t>(l.m12), K4, scale_factors, level_sigma2, nlevels, ratio_factor,
                                         w.dev<uint8_t>(l.status), w.dev<float>(l.x3D), w.dev<float>(l.normal), w.dev<float>(l.dist),
                                         w.dev<float>(l.inspect), w.dev<orbfe_new_points_result>(l.res)),
                                1, w.stream);
    }
    if (rc || (rc = w.download()) || (rc = w.sync())) return rc;
    w.get(res, l.res, sizeof *res);
    if (res->status != ORBFE_OK) return fail(ORBFE_ERR_INVALID, "%s: an octave outside [0, nlevels) on a matched feature", name);
    const size_t N1 = (size_t)n1;
    w.get(status, l.status, N1);
    // slots the kernel leaves alone (codes other than 1) are returned as zeros, not as what an earlier call left in the stage
    const uint8_t* st = w.host<uint8_t>(l.status);
    for (size_t i = 0; i < N1; i++) {
        const bool c = st[i] == ORBFE_NMP_CREATED;
        for (int k = 0; k < 3; k++) {
            x3D[3 * i + k] = c ? w.host<float>(l.x3D)[3 * i + k] : 0.f;
            normal[3 * i + k] = c ? w.host<float>(l.normal)[3 * i + k] : 0.f;
        }
        for (int k = 0; k < 2; k++) dist[2 * i + k] = c ? w.host<float>(l.dist)[2 * i + k] : 0.f;
    }
    if (search) {
        w.get(match12, l.m12, N1 * 4);
        w.get(F12, l.F12, 36); w.get(epipole, l.epipole, 8); w.get(prep, l.prep, sizeof *prep);
        for (size_t k = 0; k < 2; k++) {
            w.get(f[k].x3Dw, l.x3Dw + k * C * 12, (size_t)f[k].n * 12);
            w.get(f[k].valid, l.valid + k * C, (size_t)f[k].n);
        }
    } else {
        w.get(quantities, l.inspect, N1 * NMP_INSPECT_FLOATS * 4);
    }
    return ORBFE_OK;
}

} // namespace
} // namespace orbfe

using namespace orbfe;

extern "C" {

int orbfe_new_points_prepare_batch_device(const int32_t* d_n, int capacity, const float* d_x3Dw, const uint8_t* d_valid, const float* d_Tcw,
                                          const int32_t* d_pair1, const int32_t* d_pair2, int npairs, const float* K4, float* d_F12,
                                          float* d_epipole, orbfe_new_points_pair* d_prep, void* stream)
{
    const char* name = "orbfe_new_points_prepare_batch_device";
    if (!d_n || !d_x3Dw || !d_Tcw || !d_F12 || !d_epipole || !d_prep) return fail(ORBFE_ERR_INVALID, "%s: invalid argument", name);
    int rc = report(nmp_check_common(name, capacity, npairs, d_pair1, d_pair2, K4));
    if (rc || npairs == 0) return rc;
    NmpPrepArgs a{};
    a.nk = d_n; a.capacity = capacity; a.x3Dw = d_x3Dw; a.valid = d_valid; a.Tcw = d_Tcw; a.pair1 = d_pair1; a.pair2 = d_pair2;
    a.fx = K4[0]; a.fy = K4[1]; a.cx = K4[2]; a.cy = K4[3];
    a.F12 = d_F12; a.epipole = d_epipole; a.prep = d_prep;
    return launch_prepare(a, npairs, (hipStream_t)stream);
}

int orbfe_triangulate_matches_batch_device(const orbfe_keypoint* d_kps, const int32_t* d_n, int capacity, float* d_x3Dw, uint8_t* d_valid,
                                           uint8_t* d_free, const float* d_Tcw, const int32_t* d_pair1, const int32_t* d_pair2, int npairs,
                                           const int32_t* d_match12, const float* K4, const float* scale_factors, const float* level_sigma2,
                                           int nlevels, float ratio_factor, uint8_t* d_status, float* d_x3D, float* d_normal, float* d_dist,
                                           orbfe_new_points_result* d_res, void* stream)
{
    int rc = check_triangulate("orbfe_triangulate_matches_batch_device", d_kps, d_n, capacity, d_x3Dw, d_valid, d_free, d_Tcw, d_pair1, d_pair2,
                               npairs, d_match12, K4, scale_factors, level_sigma2, nlevels, ratio_factor, d_status, d_x3D, d_normal, d_dist, d_res);
    if (rc || npairs == 0) return rc;
    const hipStream_t s = (hipStream_t)stream;
    ORBFE_HIP(hipMemsetAsync(d_res, 0, (size_t)npairs * sizeof(orbfe_new_points_result), s));
    return launch_triangulate(tri_args(d_kps, d_n, capacity, d_x3Dw, d_valid, d_free, d_Tcw, d_pair1, d_pair2, d_match12, K4, scale_factors,
                                       level_sigma2, nlevels, ratio_factor, d_status, d_x3D, d_normal, d_dist, nullptr, d_res),
                              npairs, s);
}

int orbfe_create_new_map_points_device(const orbfe_keypoint* d_kps, const uint8_t* d_desc, const int32_t* d_n, const uint32_t* d_fv_node,
                                       const int32_t* d_fv_offset, const uint32_t* d_fv_feature, const int32_t* d_nfv, int capacity,
                                       float* d_x3Dw, uint8_t* d_valid, uint8_t* d_free, const float* d_Tcw, const int32_t* d_pair1,
                                       const int32_t* d_pair2, int npairs, const float* K4, const float* scale_factors,
                                       const float* level_sigma2, int nlevels, float ratio_factor, int check_orientation, float* d_F12,
                                       float* d_epipole, orbfe_new_points_pair* d_prep, int32_t* d_match12, int32_t* d_scratch21,
                                       int32_t* d_nmatches, uint8_t* d_status, float* d_x3D, float* d_normal, float* d_dist,
                                       orbfe_new_points_result* d_res, void* stream)
{
    const char* name = "orbfe_create_new_map_points_device";
    if (!d_desc || !d_fv_node || !d_fv_offset || !d_fv_feature || !d_nfv || !d_x3Dw || !d_valid || !d_free || !d_F12 || !d_epipole || !d_prep ||
        !d_scratch21 || !d_nmatches)
        return fail(ORBFE_ERR_INVALID, "%s: invalid argument", name);
    int rc = check_triangulate(name, d_kps, d_n, capacity, d_x3Dw, d_valid, d_free, d_Tcw, d_pair1, d_pair2, npairs, d_match12, K4, scale_factors,
                               level_sigma2, nlevels, ratio_factor, d_status, d_x3D, d_normal, d_dist, d_res);
    if (rc || npairs == 0) return rc;
    const hipStream_t s = (hipStream_t)stream;
    if ((rc = orbfe_new_points_prepare_batch_device(d_n, capacity, d_x3Dw, d_valid, d_Tcw, d_pair1, d_pair2, npairs, K4, d_F12, d_epipole, d_prep,
                                                    stream)))
        return rc;
    ORBFE_HIP(hipMemsetAsync(d_res, 0, (size_t)npairs * sizeof(orbfe_new_points_result), s));
    const size_t C = (size_t)capacity;
    for (int p = 0; p < npairs; p++) {
        const NmpChainStep st = nmp_chain_step(p, d_pair1 != nullptr);
        const NmpFrameOffsets o = nmp_frame_offsets(st, capacity);
        const int32_t *pr1 = d_pair1 ? d_pair1 + st.index : nullptr, *pr2 = d_pair2 ? d_pair2 + st.index : nullptr;
        if ((rc = orbfe_search_for_triangulation_batch_device(
                 d_kps + o.per_feature, d_desc + o.per_feature * 32, d_free + o.per_feature, d_n + o.per_frame, d_fv_node + o.per_feature,
                 d_fv_offset + o.fv_offset, d_fv_feature + o.per_feature, d_nfv + o.per_frame, capacity, pr1, pr2, 1, d_F12 + st.pair * 9,
                 d_epipole + st.pair * 2, scale_factors, level_sigma2, nlevels, check_orientation, d_match12 + st.pair * C,
                 d_scratch21 + st.pair * C, d_nmatches + st.pair, stream)))
            return rc;
        if ((rc = launch_triangulate(tri_args(d_kps + o.per_feature, d_n + o.per_frame, capacity, d_x3Dw + o.per_feature * 3,
                                              d_valid + o.per_feature, d_free + o.per_feature, d_Tcw + o.tcw, pr1, pr2, d_match12 + st.pair * C,
                                              K4, scale_factors, level_sigma2, nlevels, ratio_factor, d_status + st.pair * C,
                                              d_x3D + st.pair * C * 3, d_normal + st.pair * C * 3, d_dist + st.pair * C * 2, nullptr,
                                              d_res + st.pair),
                                     1, s)))
            return rc;
    }
    return ORBFE_OK;
}

int orbfe_create_new_map_points(const orbfe_keypoint* kps1, const uint8_t* desc1, int n1, const uint32_t* fv_node1, const int32_t* fv_offset1,
                                const uint32_t* fv_feature1, int nfv1, float* x3Dw1, uint8_t* valid1, const float* Tcw1,
                                const orbfe_keypoint* kps2, const uint8_t* desc2, int n2, const uint32_t* fv_node2, const int32_t* fv_offset2,
                                const uint32_t* fv_feature2, int nfv2, float* x3Dw2, uint8_t* valid2, const float* Tcw2, const float* K4,
                                const float* scale_factors, const float* level_sigma2, int nlevels, float ratio_factor, int check_orientation,
                                float* F12, float* epipole, orbfe_new_points_pair* prep, int32_t* match12, uint8_t* status, float* x3D,
                                float* normal, float* dist, orbfe_new_points_result* res, int device)
{
    const NmpHostSide f[2] = {{kps1, desc1, n1, fv_node1, fv_offset1, fv_feature1, nfv1, x3Dw1, valid1, Tcw1},
                              {kps2, desc2, n2, fv_node2, fv_offset2, fv_feature2, nfv2, x3Dw2, valid2, Tcw2}};
    return host_pair("orbfe_create_new_map_points", f, true, nullptr, K4, scale_factors, level_sigma2, nlevels, ratio_factor, check_orientation,
                     F12, epipole, prep, match12, status, x3D, normal, dist, nullptr, res, device);
}

int orbfe_new_points_inspect(const orbfe_keypoint* kps1, int n1, const float* Tcw1, const orbfe_keypoint* kps2, int n2, const float* Tcw2,
                             const int32_t* match12, const float* K4, const float* scale_factors, const float* level_sigma2, int nlevels,
                             float ratio_factor, uint8_t* status, float* x3D, float* normal, float* dist, float* quantities,
                             orbfe_new_points_result* res, int device)
{
    const NmpHostSide f[2] = {{kps1, nullptr, n1, nullptr, nullptr, nullptr, 0, nullptr, nullptr, Tcw1},
                              {kps2, nullptr, n2, nullptr, nullptr, nullptr, 0, nullptr, nullptr, Tcw2}};
    return host_pair("orbfe_new_points_inspect", f, false, match12, K4, scale_factors, level_sigma2, nlevels, ratio_factor, 0, nullptr, nullptr,
                     nullptr, nullptr, status, x3D, normal, dist, quantities, res, device);
}

} // extern "C"
