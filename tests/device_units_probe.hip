// device_units_probe.hip -- test infrastructure only: the device helpers that several kernels share, each behind a small kernel
// that applies it to arrays, and extern "C" calls on HOST pointers (own hipMalloc / hipMemcpy / launch / hipDeviceSynchronize /
// hipFree; the HIP error code is returned).  tests/device_units_build.py compiles this file with the library's flags and loads it
// with ctypes; it is not part of liborbfe.so.  The six headers are included unchanged:
//   include/orbfe_math.h, csrc/wave_dpp.hpp, csrc/lm_dense.hpp, csrc/ransac_sets.hpp, csrc/sim3_points.hpp, csrc/aruco_pose.hpp
// What is tested is these headers as a translation unit of their own, not their instantiations inside the product kernels.
//
// Every kernel is bounds-guarded and every output buffer is sized by the caller's n.  The kernels on wave_dpp.hpp need every lane of
// every wave active: their calls take whole rows of 64 values only (n % 64 == 0, the caller pads with the operation's identity), so
// the guard drops whole waves and never single lanes.  Workgroups are 256 threads, so wave_id() and block_sum see four waves.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "../include/orbfe_math.h"
#include "../orb_slam2_aruco_amd/csrc/aruco_pose.hpp"
#include "../orb_slam2_aruco_amd/csrc/lm_dense.hpp"
#include "../orb_slam2_aruco_amd/csrc/ransac_sets.hpp"
#include "../orb_slam2_aruco_amd/csrc/sim3_points.hpp"
#include "../orb_slam2_aruco_amd/csrc/wave_dpp.hpp"

using namespace orbfe;

namespace {

constexpr int TPB = 256;

// ---- host plumbing: device copies of host arrays, freed on every path
struct Arena {
    std::vector<void*> ptrs;
    hipError_t err = hipSuccess;
    ~Arena()
    {
        for (void* p : ptrs) (void)hipFree(p);
    }
    // a device buffer of `bytes` (at least one element, so that an empty call still has valid pointers), filled from src if given
    template <class T> T* dev(const T* src, size_t count)
    {
        if (err != hipSuccess) return nullptr;
        void* p = nullptr;
        err = hipMalloc(&p, (count ? count : 1) * sizeof(T));
        if (err != hipSuccess) return nullptr;
        ptrs.push_back(p);
        if (src && count) err = hipMemcpy(p, src, count * sizeof(T), hipMemcpyHostToDevice);
        return (T*)p;
    }
    template <class T> void back(T* dst, const T* d, size_t count)
    {
        if (err == hipSuccess && count) err = hipMemcpy(dst, d, count * sizeof(T), hipMemcpyDeviceToHost);
    }
    void ran()
    {
        if (err == hipSuccess) err = hipGetLastError();
        if (err == hipSuccess) err = hipDeviceSynchronize();
    }
};

inline dim3 grid_of(int n) { return dim3((unsigned)((n + TPB - 1) / TPB > 0 ? (n + TPB - 1) / TPB : 1)); }

// ---- include/orbfe_math.h
__global__ __launch_bounds__(TPB) void k_atan2(const float* y, const float* x, float* out, int n)
{
    const int i = blockIdx.x * TPB + threadIdx.x;
    if (i < n) out[i] = orbfe_fast_atan2(y[i], x[i]);
}
__global__ __launch_bounds__(TPB) void k_sincos(const float* a, float* s, float* c, int n)
{
    const int i = blockIdx.x * TPB + threadIdx.x;
    if (i < n) orbfe_sincosf(a[i], &s[i], &c[i]);
}
__global__ __launch_bounds__(TPB) void k_round(const double* v, const float* vf, int* rd, int* rf, int* fl, int* ce, int n)
{
    const int i = blockIdx.x * TPB + threadIdx.x;
    if (i >= n) return;
    rd[i] = orbfe_round_d(v[i]);
    rf[i] = orbfe_round_f(vf[i]);
    fl[i] = orbfe_floor_d(v[i]);
    ce[i] = orbfe_ceil_d(v[i]);
}
__global__ __launch_bounds__(TPB) void k_undistort(const float* uv, int n, const double* cam, const double* k12, float* out)
{
    const int i = blockIdx.x * TPB + threadIdx.x;
    if (i >= n) return;
    double k[12];
    for (int j = 0; j < 12; j++) k[j] = k12[j];
    orbfe_undistort_point(uv[2 * i], uv[2 * i + 1], cam[0], cam[1], cam[2], cam[3], k, &out[2 * i], &out[2 * i + 1]);
}

// ---- csrc/wave_dpp.hpp: one wave per row of 64 values, n % 64 == 0, so the guard is wave-uniform
enum { W_SCAN = 0, W_ROW16 = 1, W_SUM = 2, W_MAX = 3, W_MIN = 4 };
__global__ __launch_bounds__(TPB) void k_wave_i32(int op, const int* in, int* out, int n)
{
    const int row = blockIdx.x * (TPB / 64) + wave_id(), lane = threadIdx.x & 63;
    if (row * 64 >= n) return;
    const int v = in[row * 64 + lane];
    int r;
    switch (op) {
    case W_SCAN: r = wave_incl_scan_add(v); break;
    case W_ROW16: r = row16_incl_scan_add(v); break;
    case W_SUM: r = wave_sum(v); break;
    case W_MAX: r = wave_max(v); break;
    default: r = wave_min(v); break;
    }
    out[row * 64 + lane] = r;
}
enum { U_MAX = 0, U_MIN = 1, U_MIN2 = 2 };
// U_MIN2: the minimum, and the minimum after masking it (k_knn2_csr's best and second best of a chunk)
__global__ __launch_bounds__(TPB) void k_wave_u64(int op, const unsigned long long* in, unsigned long long* out, unsigned long long* out2, int n)
{
    const int row = blockIdx.x * (TPB / 64) + wave_id(), lane = threadIdx.x & 63;
    if (row * 64 >= n) return;
    const unsigned long long key = in[row * 64 + lane];
    if (op == U_MAX) out[row * 64 + lane] = wave_max_u64(key);
    else if (op == U_MIN) out[row * 64 + lane] = wave_min_u64(key);
    else {
        const unsigned long long m1 = wave_min_u64(key);
        const unsigned long long k2 = wave_min_u64(key == m1 ? ~0ull : key);
        out[row * 64 + lane] = m1;
        out2[row * 64 + lane] = k2;
    }
}
__global__ __launch_bounds__(TPB) void k_wave_f64(const double* in, double* out, int n)
{
    const int row = blockIdx.x * (TPB / 64) + wave_id(), lane = threadIdx.x & 63;
    if (row * 64 >= n) return;
    out[row * 64 + lane] = wave_sum_f64(in[row * 64 + lane]);
}

// ---- csrc/lm_dense.hpp
__global__ __launch_bounds__(TPB) void k_quat(const double* R, double* q4, double* rot, int n)
{
    const int i = blockIdx.x * TPB + threadIdx.x;
    if (i >= n) return;
    double m[3][3];
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) m[r][c] = R[9 * i + 3 * r + c];
    const Quat q = quat_from_matrix(m);
    q4[4 * i] = q.x; q4[4 * i + 1] = q.y; q4[4 * i + 2] = q.z; q4[4 * i + 3] = q.w;
    // the matrix of q, column by column: q e_j
    for (int j = 0; j < 3; j++) {
        const double e[3] = {j == 0 ? 1. : 0., j == 1 ? 1. : 0., j == 2 ? 1. : 0.};
        double r[3];
        rotate(q, e, r);
        for (int c = 0; c < 3; c++) rot[9 * i + 3 * c + j] = r[c];
    }
}
__global__ __launch_bounds__(TPB) void k_rotate(const double* q4, const double* v3, double* r3, int n)
{
    const int i = blockIdx.x * TPB + threadIdx.x;
    if (i >= n) return;
    const Quat q = {q4[4 * i], q4[4 * i + 1], q4[4 * i + 2], q4[4 * i + 3]};
    const double v[3] = {v3[3 * i], v3[3 * i + 1], v3[3 * i + 2]};
    double r[3];
    rotate(q, v, r);
    for (int c = 0; c < 3; c++) r3[3 * i + c] = r[c];
}
__global__ __launch_bounds__(TPB) void k_qmul(const double* a4, const double* b4, double* r4, int n)
{
    const int i = blockIdx.x * TPB + threadIdx.x;
    if (i >= n) return;
    const Quat a = {a4[4 * i], a4[4 * i + 1], a4[4 * i + 2], a4[4 * i + 3]}, b = {b4[4 * i], b4[4 * i + 1], b4[4 * i + 2], b4[4 * i + 3]};
    const Quat r = qmul(a, b);
    r4[4 * i] = r.x; r4[4 * i + 1] = r.y; r4[4 * i + 2] = r.z; r4[4 * i + 3] = r.w;
}
__global__ __launch_bounds__(TPB) void k_project(const double* Xc3, const double* obs2, const double* cam, const double* info, double* err2,
                                                 double* chi2, int n)
{
    const int i = blockIdx.x * TPB + threadIdx.x;
    if (i >= n) return;
    const double Xc[3] = {Xc3[3 * i], Xc3[3 * i + 1], Xc3[3 * i + 2]};
    const Cam K = {cam[0], cam[1], cam[2], cam[3]};
    double e[2];
    project_error(Xc, obs2[2 * i], obs2[2 * i + 1], K, e);
    err2[2 * i] = e[0]; err2[2 * i + 1] = e[1];
    chi2[i] = chi2_of(e, info[i]);
}
__global__ __launch_bounds__(TPB) void k_huber(const double* chi2, const double* delta, double* rho2, int n)
{
    const int i = blockIdx.x * TPB + threadIdx.x;
    if (i >= n) return;
    double rho[2];
    huber(chi2[i], delta[i], rho);
    rho2[2 * i] = rho[0]; rho2[2 * i + 1] = rho[1];
}
// x is read first (the caller's sentinel) and written back, so "x untouched" is visible
template <int N> __global__ __launch_bounds__(TPB) void k_ldlt(const double* H, const double* b, double* x, int* ok, int n)
{
    const int i = blockIdx.x * TPB + threadIdx.x;
    if (i >= n) return;
    double m[N][N], bb[N], xx[N];
    for (int r = 0; r < N; r++) {
        for (int c = 0; c < N; c++) m[r][c] = H[(size_t)i * N * N + r * N + c];
        bb[r] = b[i * N + r];
        xx[r] = x[i * N + r];
    }
    ok[i] = ldlt_solve<N>(m, bb, xx) ? 1 : 0;
    for (int r = 0; r < N; r++) x[i * N + r] = xx[r];
}
// one workgroup of LM_THREADS per block of LM_THREADS x N inputs; thread 0 stores the N sums
template <int N> __global__ __launch_bounds__(LM_THREADS) void k_block_sum(const double* in, double* out)
{
    __shared__ double red[LM_WAVES * N];
    double v[N];
    for (int k = 0; k < N; k++) v[k] = in[((size_t)blockIdx.x * LM_THREADS + threadIdx.x) * N + k];
    block_sum<N>(v, red);
    if (threadIdx.x == 0)
        for (int k = 0; k < N; k++) out[blockIdx.x * N + k] = v[k];
}
__global__ __launch_bounds__(LM_THREADS) void k_block_count(const int* in, int* out)
{
    __shared__ double red[LM_WAVES];
    const int c = block_count(in[blockIdx.x * LM_THREADS + threadIdx.x], red);
    if (threadIdx.x == 0) out[blockIdx.x] = c;
}

// ---- csrc/ransac_sets.hpp
template <int K> __global__ __launch_bounds__(TPB) void k_decode(const int32_t* w, int N, int32_t* out, int nsets)
{
    const int i = blockIdx.x * TPB + threadIdx.x;
    if (i >= nsets) return;
    int32_t ww[K], o[K];
    for (int j = 0; j < K; j++) ww[j] = w[(size_t)i * K + j];
    decode_set<K>(ww, N, o);
    for (int j = 0; j < K; j++) out[(size_t)i * K + j] = o[j];
}
__global__ __launch_bounds__(TPB) void k_clampn(const int* v, const int* cap, int* out, int n)
{
    const int i = blockIdx.x * TPB + threadIdx.x;
    if (i < n) out[i] = clampn(v[i], cap[i]);
}

// ---- csrc/sim3_points.hpp
__global__ __launch_bounds__(TPB) void k_rigid(const float* T12, const float* p3, float* d3, int n)
{
    const int i = blockIdx.x * TPB + threadIdx.x;
    if (i >= n) return;
    float d[3];
    rigid(&T12[12 * i], p3[3 * i], p3[3 * i + 1], p3[3 * i + 2], d);
    for (int c = 0; c < 3; c++) d3[3 * i + c] = d[c];
}


// ---- csrc/aruco_pose.hpp: one thread per case; cam17 = fx fy cx cy k[12] has_dist, one camera per call
__device__ inline PoseCamera pose_cam(const double* cam17)
{
    PoseCamera c;
    c.fx = cam17[0]; c.fy = cam17[1]; c.cx = cam17[2]; c.cy = cam17[3];
    for (int j = 0; j < 12; j++) c.k[j] = cam17[4 + j];
    c.has_dist = cam17[16] != 0.0;
    return c;
}
__global__ __launch_bounds__(TPB) void k_pose_normalise(const float* uv, const double* cam17, double* out, int n)
{
    const int i = blockIdx.x * TPB + threadIdx.x;
    if (i >= n) return;
    const pose::V2 p = pose::normalise_point(uv[2 * i], uv[2 * i + 1], pose_cam(cam17));
    out[2 * i] = p.x; out[2 * i + 1] = p.y;
}
__global__ __launch_bounds__(TPB) void k_pose_eig(const double* a6, double* h3, int n)
{
    const int i = blockIdx.x * TPB + threadIdx.x;
    if (i >= n) return;
    double h[3];
    pose::smallest_eigenvector(a6[6 * i], a6[6 * i + 1], a6[6 * i + 2], a6[6 * i + 3], a6[6 * i + 4], a6[6 * i + 5], h);
    for (int c = 0; c < 3; c++) h3[3 * i + c] = h[c];
}
__global__ __launch_bounds__(TPB) void k_pose_homography(const double* src8, const double* dst8, double* H9, int n)
{
    const int i = blockIdx.x * TPB + threadIdx.x;
    if (i >= n) return;
    pose::V2 a[4], b[4];
    for (int c = 0; c < 4; c++) { a[c] = {src8[8 * i + 2 * c], src8[8 * i + 2 * c + 1]}; b[c] = {dst8[8 * i + 2 * c], dst8[8 * i + 2 * c + 1]}; }
    double H[9];
    pose::homography4(a, b, H);
    for (int c = 0; c < 9; c++) H9[9 * i + c] = H[c];
}
__global__ __launch_bounds__(TPB) void k_pose_rotations(const double* j6, double* R1, double* R2, int n)
{
    const int i = blockIdx.x * TPB + threadIdx.x;
    if (i >= n) return;
    double a[9], b[9];
    pose::rotations(j6[6 * i], j6[6 * i + 1], j6[6 * i + 2], j6[6 * i + 3], j6[6 * i + 4], j6[6 * i + 5], a, b);
    for (int c = 0; c < 9; c++) { R1[9 * i + c] = a[c]; R2[9 * i + c] = b[c]; }
}
__global__ __launch_bounds__(TPB) void k_pose_translation(const double* obj8, const double* img8, const double* R9, double* t3, int n)
{
    const int i = blockIdx.x * TPB + threadIdx.x;
    if (i >= n) return;
    pose::V2 a[4], b[4];
    for (int c = 0; c < 4; c++) { a[c] = {obj8[8 * i + 2 * c], obj8[8 * i + 2 * c + 1]}; b[c] = {img8[8 * i + 2 * c], img8[8 * i + 2 * c + 1]}; }
    double R[9], t[3];
    for (int c = 0; c < 9; c++) R[c] = R9[9 * i + c];
    pose::translation(a, b, R, t);
    for (int c = 0; c < 3; c++) t3[3 * i + c] = t[c];
}
__global__ __launch_bounds__(TPB) void k_pose_rot2vec(const double* R9, double* r3, int n)
{
    const int i = blockIdx.x * TPB + threadIdx.x;
    if (i >= n) return;
    double R[9], r[3];
    for (int c = 0; c < 9; c++) R[c] = R9[9 * i + c];
    pose::rot2vec(R, r);
    for (int c = 0; c < 3; c++) r3[3 * i + c] = r[c];
}
__global__ __launch_bounds__(TPB) void k_pose_reproj(const float* obj8, const float* img8, const double* cam17, const double* R9, const double* t3, float* err,
                                                     int n)
{
    const int i = blockIdx.x * TPB + threadIdx.x;
    if (i >= n) return;
    float obj[4][2], img[4][2];
    for (int c = 0; c < 4; c++)
        for (int d = 0; d < 2; d++) { obj[c][d] = obj8[8 * i + 2 * c + d]; img[c][d] = img8[8 * i + 2 * c + d]; }
    double R[9], t[3];
    for (int c = 0; c < 9; c++) R[c] = R9[9 * i + c];
    for (int c = 0; c < 3; c++) t[c] = t3[3 * i + c];
    err[i] = pose::reprojection_error(obj, img, pose_cam(cam17), R, t);
}
// out14 = rvec tvec rvec2 tvec2 err[2], the fields of orbfe_marker_pose in order
__global__ __launch_bounds__(TPB) void k_pose_solve(const float* corners8, float size, const double* cam17, float* out14, int n)
{
    const int i = blockIdx.x * TPB + threadIdx.x;
    if (i >= n) return;
    float c[4][2];
    for (int a = 0; a < 4; a++)
        for (int d = 0; d < 2; d++) c[a][d] = corners8[8 * i + 2 * a + d];
    orbfe_marker_pose p;
    pose::solve_marker(c, size, pose_cam(cam17), &p);
    for (int a = 0; a < 3; a++) { out14[14 * i + a] = p.rvec[a]; out14[14 * i + 3 + a] = p.tvec[a]; out14[14 * i + 6 + a] = p.rvec2[a]; out14[14 * i + 9 + a] = p.tvec2[a]; }
    out14[14 * i + 12] = p.err[0]; out14[14 * i + 13] = p.err[1];
}
// out7 = err rvec tvec of solution `which`
__global__ __launch_bounds__(TPB) void k_pose_solve_half(const float* corners8, float size, const double* cam17, int which, float* out7, int n)
{
    const int i = blockIdx.x * TPB + threadIdx.x;
    if (i >= n) return;
    float c[4][2];
    for (int a = 0; a < 4; a++)
        for (int d = 0; d < 2; d++) c[a][d] = corners8[8 * i + 2 * a + d];
    float e, r[3], t[3];
    pose::solve_marker_half(c, size, pose_cam(cam17), which, &e, r, t);
    out7[7 * i] = e;
    for (int a = 0; a < 3; a++) { out7[7 * i + 1 + a] = r[a]; out7[7 * i + 4 + a] = t[a]; }
}

template <int N> int ldlt_call(const double* H, const double* b, double* x, int* ok, int n)
{
    if (n < 0) return (int)hipErrorInvalidValue;
    Arena A;
    const double *dH = A.dev(H, (size_t)n * N * N), *db = A.dev(b, (size_t)n * N);
    double* dx = A.dev(x, (size_t)n * N);
    int* dok = A.dev<int>(nullptr, n);
    if (A.err == hipSuccess && n) hipLaunchKernelGGL(k_ldlt<N>, grid_of(n), dim3(TPB), 0, 0, dH, db, dx, dok, n);
    A.ran();
    A.back(x, dx, (size_t)n * N);
    A.back(ok, dok, n);
    return (int)A.err;
}
template <int N> int block_sum_call(const double* in, double* out, int nblk)
{
    if (nblk < 0) return (int)hipErrorInvalidValue;
    Arena A;
    const double* din = A.dev(in, (size_t)nblk * LM_THREADS * N);
    double* dout = A.dev<double>(nullptr, (size_t)nblk * N);
    if (A.err == hipSuccess && nblk) hipLaunchKernelGGL(k_block_sum<N>, dim3(nblk), dim3(LM_THREADS), 0, 0, din, dout);
    A.ran();
    A.back(out, dout, (size_t)nblk * N);
    return (int)A.err;
}
template <int K> int decode_call(const int32_t* w, int N, int32_t* out, int nsets)
{
    if (nsets < 0 || N < K) return (int)hipErrorInvalidValue;   // decode_set's contract: N >= K
    Arena A;
    const int32_t* dw = A.dev(w, (size_t)nsets * K);
    int32_t* dout = A.dev<int32_t>(nullptr, (size_t)nsets * K);
    if (A.err == hipSuccess && nsets) hipLaunchKernelGGL(k_decode<K>, grid_of(nsets), dim3(TPB), 0, 0, dw, N, dout, nsets);
    A.ran();
    A.back(out, dout, (size_t)nsets * K);
    return (int)A.err;
}

} // namespace

#define DU_API extern "C" __attribute__((visibility("default")))

DU_API int du_device_count()
{
    int n = 0;
    return hipGetDeviceCount(&n) == hipSuccess ? n : 0;
}

DU_API int du_atan2(const float* y, const float* x, float* out, int n)
{
    if (n < 0) return (int)hipErrorInvalidValue;
    Arena A;
    const float *dy = A.dev(y, n), *dx = A.dev(x, n);
    float* dout = A.dev<float>(nullptr, n);
    if (A.err == hipSuccess && n) hipLaunchKernelGGL(k_atan2, grid_of(n), dim3(TPB), 0, 0, dy, dx, dout, n);
    A.ran();
    A.back(out, dout, n);
    return (int)A.err;
}
DU_API int du_sincos(const float* a, float* s, float* c, int n)
{
    if (n < 0) return (int)hipErrorInvalidValue;
    Arena A;
    const float* da = A.dev(a, n);
    float *ds = A.dev<float>(nullptr, n), *dc = A.dev<float>(nullptr, n);
    if (A.err == hipSuccess && n) hipLaunchKernelGGL(k_sincos, grid_of(n), dim3(TPB), 0, 0, da, ds, dc, n);
    A.ran();
    A.back(s, ds, n);
    A.back(c, dc, n);
    return (int)A.err;
}
DU_API int du_round(const double* v, const float* vf, int* rd, int* rf, int* fl, int* ce, int n)
{
    if (n < 0) return (int)hipErrorInvalidValue;
    Arena A;
    const double* dv = A.dev(v, n);
    const float* dvf = A.dev(vf, n);
    int *drd = A.dev<int>(nullptr, n), *drf = A.dev<int>(nullptr, n), *dfl = A.dev<int>(nullptr, n), *dce = A.dev<int>(nullptr, n);
    if (A.err == hipSuccess && n) hipLaunchKernelGGL(k_round, grid_of(n), dim3(TPB), 0, 0, dv, dvf, drd, drf, dfl, dce, n);
    A.ran();
    A.back(rd, drd, n);
    A.back(rf, drf, n);
    A.back(fl, dfl, n);
    A.back(ce, dce, n);
    return (int)A.err;
}
// uv n x 2, cam = fx fy cx cy, k12 = the 12 coefficients in OpenCV's order, out n x 2
DU_API int du_undistort(const float* uv, int n, const double* cam, const double* k12, float* out)
{
    if (n < 0) return (int)hipErrorInvalidValue;
    Arena A;
    const float* duv = A.dev(uv, (size_t)2 * n);
    const double *dcam = A.dev(cam, 4), *dk = A.dev(k12, 12);
    float* dout = A.dev<float>(nullptr, (size_t)2 * n);
    if (A.err == hipSuccess && n) hipLaunchKernelGGL(k_undistort, grid_of(n), dim3(TPB), 0, 0, duv, n, dcam, dk, dout);
    A.ran();
    A.back(out, dout, (size_t)2 * n);
    return (int)A.err;
}

// op: 0 wave_incl_scan_add, 1 row16_incl_scan_add, 2 wave_sum, 3 wave_max, 4 wave_min; n values = n / 64 whole rows
DU_API int du_wave_i32(int op, const int* in, int* out, int n)
{
    if (n < 0 || n % 64 || op < W_SCAN || op > W_MIN) return (int)hipErrorInvalidValue;
    Arena A;
    const int* din = A.dev(in, n);
    int* dout = A.dev<int>(nullptr, n);
    if (A.err == hipSuccess && n) hipLaunchKernelGGL(k_wave_i32, grid_of(n), dim3(TPB), 0, 0, op, din, dout, n);
    A.ran();
    A.back(out, dout, n);
    return (int)A.err;
}
// op: 0 wave_max_u64, 1 wave_min_u64, 2 minimum and second minimum after masking the first (out, out2)
DU_API int du_wave_u64(int op, const unsigned long long* in, unsigned long long* out, unsigned long long* out2, int n)
{
    if (n < 0 || n % 64 || op < U_MAX || op > U_MIN2 || (op == U_MIN2 && !out2)) return (int)hipErrorInvalidValue;
    Arena A;
    const unsigned long long* din = A.dev(in, n);
    unsigned long long *dout = A.dev<unsigned long long>(nullptr, n), *dout2 = A.dev<unsigned long long>(nullptr, n);
    if (A.err == hipSuccess && n) hipLaunchKernelGGL(k_wave_u64, grid_of(n), dim3(TPB), 0, 0, op, din, dout, dout2, n);
    A.ran();
    A.back(out, dout, n);
    if (op == U_MIN2) A.back(out2, dout2, n);
    return (int)A.err;
}
DU_API int du_wave_f64(const double* in, double* out, int n)
{
    if (n < 0 || n % 64) return (int)hipErrorInvalidValue;
    Arena A;
    const double* din = A.dev(in, n);
    double* dout = A.dev<double>(nullptr, n);
    if (A.err == hipSuccess && n) hipLaunchKernelGGL(k_wave_f64, grid_of(n), dim3(TPB), 0, 0, din, dout, n);
    A.ran();
    A.back(out, dout, n);
    return (int)A.err;
}

// R n x 9 row-major; q4 n x 4 as x y z w; rot n x 9: the matrix rotate() gives for q, row-major
DU_API int du_quat(const double* R, double* q4, double* rot, int n)
{
    if (n < 0) return (int)hipErrorInvalidValue;
    Arena A;
    const double* dR = A.dev(R, (size_t)9 * n);
    double *dq = A.dev<double>(nullptr, (size_t)4 * n), *drot = A.dev<double>(nullptr, (size_t)9 * n);
    if (A.err == hipSuccess && n) hipLaunchKernelGGL(k_quat, grid_of(n), dim3(TPB), 0, 0, dR, dq, drot, n);
    A.ran();
    A.back(q4, dq, (size_t)4 * n);
    A.back(rot, drot, (size_t)9 * n);
    return (int)A.err;
}
DU_API int du_rotate(const double* q4, const double* v3, double* r3, int n)
{
    if (n < 0) return (int)hipErrorInvalidValue;
    Arena A;
    const double *dq = A.dev(q4, (size_t)4 * n), *dv = A.dev(v3, (size_t)3 * n);
    double* dr = A.dev<double>(nullptr, (size_t)3 * n);
    if (A.err == hipSuccess && n) hipLaunchKernelGGL(k_rotate, grid_of(n), dim3(TPB), 0, 0, dq, dv, dr, n);
    A.ran();
    A.back(r3, dr, (size_t)3 * n);
    return (int)A.err;
}
DU_API int du_qmul(const double* a4, const double* b4, double* r4, int n)
{
    if (n < 0) return (int)hipErrorInvalidValue;
    Arena A;
    const double *da = A.dev(a4, (size_t)4 * n), *db = A.dev(b4, (size_t)4 * n);
    double* dr = A.dev<double>(nullptr, (size_t)4 * n);
    if (A.err == hipSuccess && n) hipLaunchKernelGGL(k_qmul, grid_of(n), dim3(TPB), 0, 0, da, db, dr, n);
    A.ran();
    A.back(r4, dr, (size_t)4 * n);
    return (int)A.err;
}
// Xc n x 3, obs n x 2, cam = fx fy cx cy, info n; err n x 2 (project_error), chi2 n (chi2_of on that error)
DU_API int du_project(const double* Xc3, const double* obs2, const double* cam, const double* info, double* err2, double* chi2, int n)
{
    if (n < 0) return (int)hipErrorInvalidValue;
    Arena A;
    const double *dX = A.dev(Xc3, (size_t)3 * n), *dobs = A.dev(obs2, (size_t)2 * n), *dcam = A.dev(cam, 4), *dinfo = A.dev(info, n);
    double *derr = A.dev<double>(nullptr, (size_t)2 * n), *dchi = A.dev<double>(nullptr, n);
    if (A.err == hipSuccess && n) hipLaunchKernelGGL(k_project, grid_of(n), dim3(TPB), 0, 0, dX, dobs, dcam, dinfo, derr, dchi, n);
    A.ran();
    A.back(err2, derr, (size_t)2 * n);
    A.back(chi2, dchi, n);
    return (int)A.err;
}
DU_API int du_huber(const double* chi2, const double* delta, double* rho2, int n)
{
    if (n < 0) return (int)hipErrorInvalidValue;
    Arena A;
    const double *dchi = A.dev(chi2, n), *ddelta = A.dev(delta, n);
    double* drho = A.dev<double>(nullptr, (size_t)2 * n);
    if (A.err == hipSuccess && n) hipLaunchKernelGGL(k_huber, grid_of(n), dim3(TPB), 0, 0, dchi, ddelta, drho, n);
    A.ran();
    A.back(rho2, drho, (size_t)2 * n);
    return (int)A.err;
}
// H n x N x N row-major (the lower triangle is what ldlt_solve reads), b n x N, x n x N in and out, ok n
DU_API int du_ldlt6(const double* H, const double* b, double* x, int* ok, int n) { return ldlt_call<6>(H, b, x, ok, n); }
DU_API int du_ldlt7(const double* H, const double* b, double* x, int* ok, int n) { return ldlt_call<7>(H, b, x, ok, n); }
// in nblk x 256 x N (thread-major), out nblk x N
DU_API int du_block_sum2(const double* in, double* out, int nblk) { return block_sum_call<2>(in, out, nblk); }
DU_API int du_block_sum7(const double* in, double* out, int nblk) { return block_sum_call<7>(in, out, nblk); }
DU_API int du_block_count(const int* in, int* out, int nblk)
{
    if (nblk < 0) return (int)hipErrorInvalidValue;
    Arena A;
    const int* din = A.dev(in, (size_t)nblk * LM_THREADS);
    int* dout = A.dev<int>(nullptr, nblk);
    if (A.err == hipSuccess && nblk) hipLaunchKernelGGL(k_block_count, dim3(nblk), dim3(LM_THREADS), 0, 0, din, dout);
    A.ran();
    A.back(out, dout, nblk);
    return (int)A.err;
}

// w nsets x K rand() words, out nsets x K indices into 0 .. N-1
DU_API int du_decode8(const int32_t* w, int N, int32_t* out, int nsets) { return decode_call<8>(w, N, out, nsets); }
DU_API int du_decode3(const int32_t* w, int N, int32_t* out, int nsets) { return decode_call<3>(w, N, out, nsets); }
DU_API int du_clampn(const int* v, const int* cap, int* out, int n)
{
    if (n < 0) return (int)hipErrorInvalidValue;
    Arena A;
    const int *dv = A.dev(v, n), *dcap = A.dev(cap, n);
    int* dout = A.dev<int>(nullptr, n);
    if (A.err == hipSuccess && n) hipLaunchKernelGGL(k_clampn, grid_of(n), dim3(TPB), 0, 0, dv, dcap, dout, n);
    A.ran();
    A.back(out, dout, n);
    return (int)A.err;
}

// T12 n x 12 (3 x 4 row-major [A | t]), p3 n x 3, d3 n x 3
DU_API int du_rigid(const float* T12, const float* p3, float* d3, int n)
{
    if (n < 0) return (int)hipErrorInvalidValue;
    Arena A;
    const float *dT = A.dev(T12, (size_t)12 * n), *dp = A.dev(p3, (size_t)3 * n);
    float* dd = A.dev<float>(nullptr, (size_t)3 * n);
    if (A.err == hipSuccess && n) hipLaunchKernelGGL(k_rigid, grid_of(n), dim3(TPB), 0, 0, dT, dp, dd, n);
    A.ran();
    A.back(d3, dd, (size_t)3 * n);
    return (int)A.err;
}

// ---- csrc/aruco_pose.hpp.  cam17 = fx fy cx cy k[12] has_dist (doubles), one camera per call
DU_API int du_pose_normalise(const float* uv, const double* cam17, double* out, int n)
{
    if (n < 0) return (int)hipErrorInvalidValue;
    Arena A;
    const float* duv = A.dev(uv, (size_t)2 * n);
    const double* dcam = A.dev(cam17, 17);
    double* dout = A.dev<double>(nullptr, (size_t)2 * n);
    if (A.err == hipSuccess && n) hipLaunchKernelGGL(k_pose_normalise, grid_of(n), dim3(TPB), 0, 0, duv, dcam, dout, n);
    A.ran();
    A.back(out, dout, (size_t)2 * n);
    return (int)A.err;
}
// a6 n x 6 = a00 a01 a02 a11 a12 a22; h3 n x 3
DU_API int du_pose_eig(const double* a6, double* h3, int n)
{
    if (n < 0) return (int)hipErrorInvalidValue;
    Arena A;
    const double* da = A.dev(a6, (size_t)6 * n);
    double* dh = A.dev<double>(nullptr, (size_t)3 * n);
    if (A.err == hipSuccess && n) hipLaunchKernelGGL(k_pose_eig, grid_of(n), dim3(TPB), 0, 0, da, dh, n);
    A.ran();
    A.back(h3, dh, (size_t)3 * n);
    return (int)A.err;
}
// src8, dst8 n x 4 x 2; H9 n x 9 row-major
DU_API int du_pose_homography(const double* src8, const double* dst8, double* H9, int n)
{
    if (n < 0) return (int)hipErrorInvalidValue;
    Arena A;
    const double *ds = A.dev(src8, (size_t)8 * n), *dd = A.dev(dst8, (size_t)8 * n);
    double* dH = A.dev<double>(nullptr, (size_t)9 * n);
    if (A.err == hipSuccess && n) hipLaunchKernelGGL(k_pose_homography, grid_of(n), dim3(TPB), 0, 0, ds, dd, dH, n);
    A.ran();
    A.back(H9, dH, (size_t)9 * n);
    return (int)A.err;
}
// j6 n x 6 = j00 j01 j10 j11 p q; R1, R2 n x 9
DU_API int du_pose_rotations(const double* j6, double* R1, double* R2, int n)
{
    if (n < 0) return (int)hipErrorInvalidValue;
    Arena A;
    const double* dj = A.dev(j6, (size_t)6 * n);
    double *d1 = A.dev<double>(nullptr, (size_t)9 * n), *d2 = A.dev<double>(nullptr, (size_t)9 * n);
    if (A.err == hipSuccess && n) hipLaunchKernelGGL(k_pose_rotations, grid_of(n), dim3(TPB), 0, 0, dj, d1, d2, n);
    A.ran();
    A.back(R1, d1, (size_t)9 * n);
    A.back(R2, d2, (size_t)9 * n);
    return (int)A.err;
}
DU_API int du_pose_translation(const double* obj8, const double* img8, const double* R9, double* t3, int n)
{
    if (n < 0) return (int)hipErrorInvalidValue;
    Arena A;
    const double *dobj = A.dev(obj8, (size_t)8 * n), *dimg = A.dev(img8, (size_t)8 * n), *dR = A.dev(R9, (size_t)9 * n);
    double* dt = A.dev<double>(nullptr, (size_t)3 * n);
    if (A.err == hipSuccess && n) hipLaunchKernelGGL(k_pose_translation, grid_of(n), dim3(TPB), 0, 0, dobj, dimg, dR, dt, n);
    A.ran();
    A.back(t3, dt, (size_t)3 * n);
    return (int)A.err;
}
DU_API int du_pose_rot2vec(const double* R9, double* r3, int n)
{
    if (n < 0) return (int)hipErrorInvalidValue;
    Arena A;
    const double* dR = A.dev(R9, (size_t)9 * n);
    double* dr = A.dev<double>(nullptr, (size_t)3 * n);
    if (A.err == hipSuccess && n) hipLaunchKernelGGL(k_pose_rot2vec, grid_of(n), dim3(TPB), 0, 0, dR, dr, n);
    A.ran();
    A.back(r3, dr, (size_t)3 * n);
    return (int)A.err;
}
// obj8, img8 n x 4 x 2 float (marker plane, pixels); err n
DU_API int du_pose_reproj(const float* obj8, const float* img8, const double* cam17, const double* R9, const double* t3, float* err, int n)
{
    if (n < 0) return (int)hipErrorInvalidValue;
    Arena A;
    const float *dobj = A.dev(obj8, (size_t)8 * n), *dimg = A.dev(img8, (size_t)8 * n);
    const double *dcam = A.dev(cam17, 17), *dR = A.dev(R9, (size_t)9 * n), *dt = A.dev(t3, (size_t)3 * n);
    float* derr = A.dev<float>(nullptr, n);
    if (A.err == hipSuccess && n) hipLaunchKernelGGL(k_pose_reproj, grid_of(n), dim3(TPB), 0, 0, dobj, dimg, dcam, dR, dt, derr, n);
    A.ran();
    A.back(err, derr, n);
    return (int)A.err;
}
DU_API int du_pose_solve(const float* corners8, float size, const double* cam17, float* out14, int n)
{
    if (n < 0) return (int)hipErrorInvalidValue;
    Arena A;
    const float* dc = A.dev(corners8, (size_t)8 * n);
    const double* dcam = A.dev(cam17, 17);
    float* dout = A.dev<float>(nullptr, (size_t)14 * n);
    if (A.err == hipSuccess && n) hipLaunchKernelGGL(k_pose_solve, grid_of(n), dim3(TPB), 0, 0, dc, size, dcam, dout, n);
    A.ran();
    A.back(out14, dout, (size_t)14 * n);
    return (int)A.err;
}
DU_API int du_pose_solve_half(const float* corners8, float size, const double* cam17, int which, float* out7, int n)
{
    if (n < 0 || which < 0 || which > 1) return (int)hipErrorInvalidValue;
    Arena A;
    const float* dc = A.dev(corners8, (size_t)8 * n);
    const double* dcam = A.dev(cam17, 17);
    float* dout = A.dev<float>(nullptr, (size_t)7 * n);
    if (A.err == hipSuccess && n) hipLaunchKernelGGL(k_pose_solve_half, grid_of(n), dim3(TPB), 0, 0, dc, size, dcam, which, dout, n);
    A.ran();
    A.back(out7, dout, (size_t)7 * n);
    return (int)A.err;
}
