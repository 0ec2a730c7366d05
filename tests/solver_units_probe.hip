// solver_units_probe.hip -- test infrastructure only, the second unit probe (the first is device_units_probe.hip): the device helpers
// of the optimizers and solvers, each behind a small kernel that applies it to arrays, and extern "C" calls on HOST pointers (own
// hipMalloc / hipMemcpy / one launch / hipDeviceSynchronize / hipFree; the HIP error code is returned).
// tests/solver_units_build.py compiles this file with the library's flags and loads it with ctypes; it is not part of liborbfe.so.
// The five headers are included unchanged:
//   csrc/se3_quat.hpp, csrc/sim3_group.hpp, csrc/svd_jacobi.hpp, csrc/front_solve.hpp, csrc/ba_edges.hpp
//
// Every kernel is bounds-guarded and every buffer is sized by the caller's n.  The per-lane SVD kernels run under
// __launch_bounds__(64), so that <16, 9, 9> has the registers its product caller has and does not spill (the product's 4 x 4 callers
// run under other bounds: what is tested is the header, not their instantiations); the front kernels are one workgroup of LM_THREADS per system with fail_s in LDS, as
// k_eg_front and k_gba_front call them; the wave kernels take whole rows of 64 values.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "../orb_slam2_aruco_amd/csrc/ba_edges.hpp"
#include "../orb_slam2_aruco_amd/csrc/front_solve.hpp"
#include "../orb_slam2_aruco_amd/csrc/se3_quat.hpp"
#include "../orb_slam2_aruco_amd/csrc/sim3_group.hpp"
#include "../orb_slam2_aruco_amd/csrc/svd_jacobi.hpp"

using namespace orbfe;

namespace {

constexpr int TPB = 256;

struct Arena {
    std::vector<void*> ptrs;
    hipError_t err = hipSuccess;
    ~Arena()
    {
        for (void* p : ptrs) (void)hipFree(p);
    }
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

inline dim3 grid_of(int n, int tpb = TPB) { return dim3((unsigned)((n + tpb - 1) / tpb > 0 ? (n + tpb - 1) / tpb : 1)); }

// an SE3 as 7 doubles: q (x y z w), t
__device__ inline SE3 se3_of(const double* a)
{
    SE3 T;
    T.q = Quat{a[0], a[1], a[2], a[3]};
    for (int i = 0; i < 3; i++) T.t[i] = a[4 + i];
    T.pad = 0;
    return T;
}
__device__ inline void se3_to(const SE3& T, double* a)
{
    a[0] = T.q.x; a[1] = T.q.y; a[2] = T.q.z; a[3] = T.q.w;
    for (int i = 0; i < 3; i++) a[4 + i] = T.t[i];
}
// a Sim3 as 8 doubles: q (x y z w), t, s
__device__ inline Sim3 sim_of(const double* a)
{
    Sim3 S;
    S.q = Quat{a[0], a[1], a[2], a[3]};
    for (int i = 0; i < 3; i++) S.t[i] = a[4 + i];
    S.s = a[7];
    return S;
}
__device__ inline void sim_to(const Sim3& S, double* a)
{
    a[0] = S.q.x; a[1] = S.q.y; a[2] = S.q.z; a[3] = S.q.w;
    for (int i = 0; i < 3; i++) a[4 + i] = S.t[i];
    a[7] = S.s;
}

// ---- csrc/se3_quat.hpp
__global__ __launch_bounds__(TPB) void k_se3_exp(const double* u6, double* out7, int n)
{
    const int i = blockIdx.x * TPB + threadIdx.x;
    if (i >= n) return;
    double u[6];
    for (int c = 0; c < 6; c++) u[c] = u6[6 * i + c];
    se3_to(se3_exp(u), out7 + 7 * i);
}
__global__ __launch_bounds__(TPB) void k_se3_mul(const double* a7, const double* b7, double* out7, int n)
{
    const int i = blockIdx.x * TPB + threadIdx.x;
    if (i >= n) return;
    se3_to(mul(se3_of(a7 + 7 * i), se3_of(b7 + 7 * i)), out7 + 7 * i);
}
__global__ __launch_bounds__(TPB) void k_se3_map(const double* a7, const double* p3, double* out3, int n)
{
    const int i = blockIdx.x * TPB + threadIdx.x;
    if (i >= n) return;
    const double p[3] = {p3[3 * i], p3[3 * i + 1], p3[3 * i + 2]};
    double r[3];
    map(se3_of(a7 + 7 * i), p, r);
    for (int c = 0; c < 3; c++) out3[3 * i + c] = r[c];
}
__global__ __launch_bounds__(TPB) void k_normalize(const double* q4, double* out4, int n)
{
    const int i = blockIdx.x * TPB + threadIdx.x;
    if (i >= n) return;
    Quat q = {q4[4 * i], q4[4 * i + 1], q4[4 * i + 2], q4[4 * i + 3]};
    normalize_rotation(q);
    out4[4 * i] = q.x; out4[4 * i + 1] = q.y; out4[4 * i + 2] = q.z; out4[4 * i + 3] = q.w;
}
__global__ __launch_bounds__(TPB) void k_se3_from_float(const float* Rt12, double* out7, int n)
{
    const int i = blockIdx.x * TPB + threadIdx.x;
    if (i >= n) return;
    se3_to(se3_from_float(Rt12 + 12 * i), out7 + 7 * i);
}
__global__ __launch_bounds__(TPB) void k_to_float(const double* a7, float* Rt12, int n)
{
    const int i = blockIdx.x * TPB + threadIdx.x;
    if (i >= n) return;
    to_float(se3_of(a7 + 7 * i), Rt12 + 12 * i);
}

// ---- csrc/sim3_group.hpp
__global__ __launch_bounds__(TPB) void k_sim3_exp(const double* u7, double* out8, int n)
{
    const int i = blockIdx.x * TPB + threadIdx.x;
    if (i >= n) return;
    double u[7];
    for (int c = 0; c < 7; c++) u[c] = u7[7 * i + c];
    sim_to(sim3_exp(u), out8 + 8 * i);
}
__global__ __launch_bounds__(TPB) void k_sim3_log(const double* s8, double* out7, int n)
{
    const int i = blockIdx.x * TPB + threadIdx.x;
    if (i >= n) return;
    double r[7];
    sim3_log(sim_of(s8 + 8 * i), r);
    for (int c = 0; c < 7; c++) out7[7 * i + c] = r[c];
}
__global__ __launch_bounds__(TPB) void k_sim3_mul(const double* a8, const double* b8, double* out8, int n)
{
    const int i = blockIdx.x * TPB + threadIdx.x;
    if (i >= n) return;
    sim_to(mul(sim_of(a8 + 8 * i), sim_of(b8 + 8 * i)), out8 + 8 * i);
}
__global__ __launch_bounds__(TPB) void k_sim3_map(const double* a8, const double* p3, double* out3, int n)
{
    const int i = blockIdx.x * TPB + threadIdx.x;
    if (i >= n) return;
    const double p[3] = {p3[3 * i], p3[3 * i + 1], p3[3 * i + 2]};
    double r[3];
    map(sim_of(a8 + 8 * i), p, r);
    for (int c = 0; c < 3; c++) out3[3 * i + c] = r[c];
}
__global__ __launch_bounds__(TPB) void k_sim3_inverse(const double* a8, double* out8, int n)
{
    const int i = blockIdx.x * TPB + threadIdx.x;
    if (i >= n) return;
    sim_to(inverse(sim_of(a8 + 8 * i)), out8 + 8 * i);
}
__global__ __launch_bounds__(TPB) void k_lu3(const double* m9, const double* b3, double* x3, int n)
{
    const int i = blockIdx.x * TPB + threadIdx.x;
    if (i >= n) return;
    double m[3][3], b[3], x[3];
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) m[r][c] = m9[9 * i + 3 * r + c];
        b[r] = b3[3 * i + r];
    }
    lu3_solve(m, b, x);
    for (int c = 0; c < 3; c++) x3[3 * i + c] = x[c];
}

// ---- csrc/svd_jacobi.hpp: one matrix a lane.  at: n x N1 x M (rows N.. are storage, as the callers leave it); out: w n x N,
// vt n x N x N, at_out n x N1 x M
template <int M, int N, int N1, bool WANT_U> __global__ __launch_bounds__(64) void k_svd(const float* at, float* w, float* vt, float* at_out, int n)
{
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    float At[N1][M], W[N], Vt[N][N];
    for (int r = 0; r < N1; r++)
        for (int c = 0; c < M; c++) At[r][c] = at[((size_t)i * N1 + r) * M + c];
    svd_jacobi<M, N, N1, WANT_U>(At, W, Vt);
    for (int r = 0; r < N; r++) {
        w[(size_t)i * N + r] = W[r];
        for (int c = 0; c < N; c++) vt[((size_t)i * N + r) * N + c] = Vt[r][c];
    }
    for (int r = 0; r < N1; r++)
        for (int c = 0; c < M; c++) at_out[((size_t)i * N1 + r) * M + c] = At[r][c];
}
template <int M, int N, int N1, bool WANT_U> int svd_call(const float* at, float* w, float* vt, float* at_out, int n)
{
    Arena a;
    const float* d_at = a.dev(at, (size_t)n * N1 * M);
    float* d_w = a.dev<float>(nullptr, (size_t)n * N);
    float* d_vt = a.dev<float>(nullptr, (size_t)n * N * N);
    float* d_out = a.dev<float>(nullptr, (size_t)n * N1 * M);
    if (a.err == hipSuccess) {
        k_svd<M, N, N1, WANT_U><<<grid_of(n, 64), 64>>>(d_at, d_w, d_vt, d_out, n);
        a.ran();
    }
    a.back(w, d_w, (size_t)n * N);
    a.back(vt, d_vt, (size_t)n * N * N);
    a.back(at_out, d_out, (size_t)n * N1 * M);
    return (int)a.err;
}

// ---- csrc/front_solve.hpp: a workgroup a system.  m: nsys x (n * n) rows of n (lower triangle in use), r: nsys x n.  packed: the
// lower triangle goes through dynamic LDS as in k_gba_front and comes back only when the factorisation succeeded.  ret: nsys x
// LM_THREADS, what each thread was returned; fail: nsys, fail_s behind the call.
__global__ __launch_bounds__(LM_THREADS) void k_front_llt(int packed, double* m, int n, int k, double* r, int* ret, int* fail)
{
    extern __shared__ __align__(16) double su_tri[];
    __shared__ int fail_s;
    const int tid = threadIdx.x;
    double* F = m + (size_t)blockIdx.x * n * n;
    double* rr = r + (size_t)blockIdx.x * n;
    if (tid == 0) fail_s = 0;
    __syncthreads();
    bool ok;
    if (packed) {
        for (int i = 0; i < n; i++)
            for (int j = tid; j <= i; j += LM_THREADS) su_tri[(size_t)i * (i + 1) / 2 + j] = F[(size_t)i * n + j];
        __syncthreads();
        ok = front_partial_llt<true>(su_tri, n, k, rr, &fail_s);
        if (ok)
            for (int i = 0; i < n; i++)
                for (int j = tid; j <= i; j += LM_THREADS) F[(size_t)i * n + j] = su_tri[(size_t)i * (i + 1) / 2 + j];
        __syncthreads();
    } else {
        ok = front_partial_llt<false>(F, n, k, rr, &fail_s);
    }
    ret[(size_t)blockIdx.x * LM_THREADS + tid] = ok ? 1 : 0;
    if (tid == 0) fail[blockIdx.x] = fail_s;
}

// a workgroup a system, all of one shape: vtx nsys x (nown + nb), xt nsys x (nvert * R), f nsys x (n * n), r nsys x n, w nsys x n
template <int R> __global__ __launch_bounds__(LM_THREADS) void k_front_back(int nown, int nb, int nvert, const int32_t* vtx, double* xt, const double* f,
                                                                             const double* r, double* w)
{
    FrontNode nd = {};
    nd.nown = nown;
    nd.nb = nb;
    const int n = R * (nown + nb);
    const size_t s = blockIdx.x;
    front_substitute_back<R>(nd, vtx + s * (nown + nb), xt + s * nvert * R, f + s * n * n, r + s * n, w + s * n);
}
template <int R> int front_back_call(int nsys, int nown, int nb, int nvert, const int32_t* vtx, double* xt, const double* f, const double* r)
{
    Arena a;
    const size_t n = (size_t)R * (nown + nb);
    const int32_t* d_v = a.dev(vtx, (size_t)nsys * (nown + nb));
    double* d_x = a.dev(xt, (size_t)nsys * nvert * R);
    const double* d_f = a.dev(f, nsys * n * n);
    const double* d_r = a.dev(r, nsys * n);
    double* d_w = a.dev<double>(nullptr, nsys * n);
    if (a.err == hipSuccess && nsys > 0) {
        k_front_back<R><<<dim3((unsigned)nsys), LM_THREADS>>>(nown, nb, nvert, d_v, d_x, d_f, d_r, d_w);
        a.ran();
    }
    a.back(xt, d_x, (size_t)nsys * nvert * R);
    return (int)a.err;
}

// ---- csrc/ba_edges.hpp
// out20 = err[2] Jp[2][6] Jx[2][3]
__global__ __launch_bounds__(TPB) void k_mono(const double* t7, const double* x3, const double* obs2, const double* cam, double* out20, int n)
{
    const int i = blockIdx.x * TPB + threadIdx.x;
    if (i >= n) return;
    const Cam K = {cam[0], cam[1], cam[2], cam[3]};
    const double X[3] = {x3[3 * i], x3[3 * i + 1], x3[3 * i + 2]};
    MonoLin o;
    lba_mono_linearize(se3_of(t7 + 7 * i), X, obs2[2 * i], obs2[2 * i + 1], K, o);
    double* out = out20 + 20 * i;
    out[0] = o.err[0]; out[1] = o.err[1];
    for (int a = 0; a < 2; a++) {
        for (int c = 0; c < 6; c++) out[2 + 6 * a + c] = o.Jp[a][c];
        for (int c = 0; c < 3; c++) out[14 + 3 * a + c] = o.Jx[a][c];
    }
}
// the poses come as 3 x 4 floats, as the restatement's entry takes them; out26 = err[2] Jc[2][6] Jm[2][6]
__global__ __launch_bounds__(TPB) void k_marker(const float* tcw12, const float* twm12, const double* p3, const double* obs2, const double* cam,
                                                double* out26, int n)
{
    const int i = blockIdx.x * TPB + threadIdx.x;
    if (i >= n) return;
    const Cam K = {cam[0], cam[1], cam[2], cam[3]};
    const SE3 Tc = se3_from_float(tcw12 + 12 * i), Tm = se3_from_float(twm12 + 12 * i);
    const double p[3] = {p3[3 * i], p3[3 * i + 1], p3[3 * i + 2]};
    double e[2], Jc[2][6], Jm[2][6];
    lba_marker_error(Tc, Tm, p, obs2[2 * i], obs2[2 * i + 1], K, e);
    lba_marker_jacobian(Tc, Tm, true, p, obs2[2 * i], obs2[2 * i + 1], K, Jc);
    lba_marker_jacobian(Tc, Tm, false, p, obs2[2 * i], obs2[2 * i + 1], K, Jm);
    double* out = out26 + 26 * i;
    out[0] = e[0]; out[1] = e[1];
    for (int a = 0; a < 2; a++)
        for (int c = 0; c < 6; c++) {
            out[2 + 6 * a + c] = Jc[a][c];
            out[14 + 6 * a + c] = Jm[a][c];
        }
}
// in15 = J[2][6] w r0 r1
__global__ __launch_bounds__(TPB) void k_diag(const double* in15, double* out27, int n)
{
    const int i = blockIdx.x * TPB + threadIdx.x;
    if (i >= n) return;
    double J[2][6], out[27];
    for (int a = 0; a < 2; a++)
        for (int c = 0; c < 6; c++) J[a][c] = in15[15 * i + 6 * a + c];
    lba_diag_block(J, in15[15 * i + 12], in15[15 * i + 13], in15[15 * i + 14], out);
    for (int c = 0; c < 27; c++) out27[27 * i + c] = out[c];
}
__global__ __launch_bounds__(TPB) void k_rot_of(const double* q4, double* r9, int n)
{
    const int i = blockIdx.x * TPB + threadIdx.x;
    if (i >= n) return;
    double R[3][3];
    rot_of(Quat{q4[4 * i], q4[4 * i + 1], q4[4 * i + 2], q4[4 * i + 3]}, R);
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) r9[9 * i + 3 * r + c] = R[r][c];
}
// one wave per row of 64 values, n % 64 == 0, so the guard is wave-uniform; op 0: wave_sum, 1: wave_max
__global__ __launch_bounds__(TPB) void k_wave(int op, const double* in, double* out, int n)
{
    const int row = blockIdx.x * (TPB / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row * 64 >= n) return;
    const double v = in[row * 64 + lane];
    out[row * 64 + lane] = op == 0 ? wave_sum(v) : wave_max(v);
}

// in7 = Hll[6] lambda
__global__ __launch_bounds__(TPB) void k_dinv3(const double* in7, double* d9, int n)
{
    const int i = blockIdx.x * TPB + threadIdx.x;
    if (i >= n) return;
    damped_inverse3(in7 + 7 * i, in7[7 * i + 6], d9 + 9 * i);
}
// a thread a system of nitems items, the accumulators in / out: w nsys x nitems x 2 x 18 (Wi, Wj), d nsys x nitems x 9, bl nsys x nitems x 3
__global__ __launch_bounds__(TPB) void k_pair_items(const double* w, const double* d, const double* bl, int nitems, int diag, double* acc36, double* accb6,
                                                    int nsys)
{
    const int i = blockIdx.x * TPB + threadIdx.x;
    if (i >= nsys) return;
    double acc[36], accb[6];
    for (int k = 0; k < 36; k++) acc[k] = acc36[36 * i + k];
    for (int k = 0; k < 6; k++) accb[k] = accb6[6 * i + k];
    for (int it = 0; it < nitems; it++) {
        const size_t q = (size_t)i * nitems + it;
        pair_item_add(w + q * 36, w + q * 36 + 18, d + q * 9, bl + q * 3, diag != 0, acc, accb);
    }
    for (int k = 0; k < 36; k++) acc36[36 * i + k] = acc[k];
    for (int k = 0; k < 6; k++) accb6[6 * i + k] = accb[k];
}
// one workgroup: the children of nodes[node] into its front
template <int R> __global__ __launch_bounds__(LM_THREADS) void k_merge(const FrontNode* nodes, int node, const int32_t* cmap, double* fronts)
{
    const FrontNode nd = nodes[node];
    const int n = R * (nd.nown + nd.nb);
    double* F = fronts + nd.front;
    front_merge_children<R>(nd, nodes, cmap, fronts, F, F + (size_t)n * n);
}
// one workgroup: run_sum, then block_sum
__global__ __launch_bounds__(LM_THREADS) void k_run_sum(const double* v, int n, double* out)
{
    __shared__ double red[LM_WAVES];
    double s[1] = {run_sum(v, n)};
    block_sum<1>(s, red);
    if (threadIdx.x == 0) out[0] = s[0];
}

// out = f(in...) over n items of the given widths, all doubles
template <class K> int call1(K kernel, const double* in, int win, double* out, int wout, int n)
{
    Arena a;
    const double* d_in = a.dev(in, (size_t)n * win);
    double* d_out = a.dev<double>(nullptr, (size_t)n * wout);
    if (a.err == hipSuccess) {
        kernel<<<grid_of(n), TPB>>>(d_in, d_out, n);
        a.ran();
    }
    a.back(out, d_out, (size_t)n * wout);
    return (int)a.err;
}
template <class K> int call2(K kernel, const double* x, int wx, const double* y, int wy, double* out, int wout, int n)
{
    Arena a;
    const double* d_x = a.dev(x, (size_t)n * wx);
    const double* d_y = a.dev(y, (size_t)n * wy);
    double* d_out = a.dev<double>(nullptr, (size_t)n * wout);
    if (a.err == hipSuccess) {
        kernel<<<grid_of(n), TPB>>>(d_x, d_y, d_out, n);
        a.ran();
    }
    a.back(out, d_out, (size_t)n * wout);
    return (int)a.err;
}

} // namespace

// the library's flags hide every symbol; these calls are the probe's interface
#pragma GCC visibility push(default)
extern "C" {

int su_device_count()
{
    int n = 0;
    return hipGetDeviceCount(&n) == hipSuccess ? n : 0;
}
// the workgroup size of the front kernels, for the sizes of `ret` on the caller's side
int su_lm_threads() { return LM_THREADS; }

int su_se3_exp(const double* u6, double* out7, int n) { return call1(k_se3_exp, u6, 6, out7, 7, n); }
int su_se3_mul(const double* a7, const double* b7, double* out7, int n) { return call2(k_se3_mul, a7, 7, b7, 7, out7, 7, n); }
int su_se3_map(const double* a7, const double* p3, double* out3, int n) { return call2(k_se3_map, a7, 7, p3, 3, out3, 3, n); }
int su_normalize(const double* q4, double* out4, int n) { return call1(k_normalize, q4, 4, out4, 4, n); }
int su_se3_from_float(const float* Rt12, double* out7, int n)
{
    Arena a;
    const float* d_in = a.dev(Rt12, (size_t)n * 12);
    double* d_out = a.dev<double>(nullptr, (size_t)n * 7);
    if (a.err == hipSuccess) {
        k_se3_from_float<<<grid_of(n), TPB>>>(d_in, d_out, n);
        a.ran();
    }
    a.back(out7, d_out, (size_t)n * 7);
    return (int)a.err;
}
int su_to_float(const double* a7, float* Rt12, int n)
{
    Arena a;
    const double* d_in = a.dev(a7, (size_t)n * 7);
    float* d_out = a.dev<float>(nullptr, (size_t)n * 12);
    if (a.err == hipSuccess) {
        k_to_float<<<grid_of(n), TPB>>>(d_in, d_out, n);
        a.ran();
    }
    a.back(Rt12, d_out, (size_t)n * 12);
    return (int)a.err;
}

int su_sim3_exp(const double* u7, double* out8, int n) { return call1(k_sim3_exp, u7, 7, out8, 8, n); }
int su_sim3_log(const double* s8, double* out7, int n) { return call1(k_sim3_log, s8, 8, out7, 7, n); }
int su_sim3_mul(const double* a8, const double* b8, double* out8, int n) { return call2(k_sim3_mul, a8, 8, b8, 8, out8, 8, n); }
int su_sim3_map(const double* a8, const double* p3, double* out3, int n) { return call2(k_sim3_map, a8, 8, p3, 3, out3, 3, n); }
int su_sim3_inverse(const double* a8, double* out8, int n) { return call1(k_sim3_inverse, a8, 8, out8, 8, n); }
int su_lu3(const double* m9, const double* b3, double* x3, int n) { return call2(k_lu3, m9, 9, b3, 3, x3, 3, n); }

int su_svd_3x3(const float* at, float* w, float* vt, float* at_out, int n) { return svd_call<3, 3, 3, true>(at, w, vt, at_out, n); }
int su_svd_4x4(const float* at, float* w, float* vt, float* at_out, int n) { return svd_call<4, 4, 4, false>(at, w, vt, at_out, n); }
int su_svd_16x9(const float* at, float* w, float* vt, float* at_out, int n) { return svd_call<16, 9, 9, false>(at, w, vt, at_out, n); }
int su_svd_9x8(const float* at, float* w, float* vt, float* at_out, int n) { return svd_call<9, 8, 9, true>(at, w, vt, at_out, n); }

// m and r are in / out: nsys x (n * n) and nsys x n, each with `guard` doubles in front and behind that the caller fills and checks
// (solver_units_build.front_llt); the kernel is handed the inner parts.
int su_front_llt(int packed, double* m, int n, int k, double* r, int nsys, int guard, int* ret, int* fail)
{
    Arena a;
    const size_t nm = (size_t)nsys * n * n + 2 * (size_t)guard, nr = (size_t)nsys * n + 2 * (size_t)guard;
    double* d_m = a.dev(m, nm);
    double* d_r = a.dev(r, nr);
    int* d_ret = a.dev<int>(nullptr, (size_t)nsys * LM_THREADS);
    int* d_fail = a.dev<int>(nullptr, (size_t)nsys);
    const size_t lds = packed ? (size_t)n * (n + 1) / 2 * sizeof(double) : 0;
    if (a.err == hipSuccess && lds > 48 * 1024)
        a.err = hipFuncSetAttribute(reinterpret_cast<const void*>(k_front_llt), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (a.err == hipSuccess && nsys > 0) {
        k_front_llt<<<dim3((unsigned)nsys), LM_THREADS, lds>>>(packed, d_m + guard, n, k, d_r + guard, d_ret, d_fail);
        a.ran();
    }
    a.back(m, d_m, nm);
    a.back(r, d_r, nr);
    a.back(ret, d_ret, (size_t)nsys * LM_THREADS);
    a.back(fail, d_fail, (size_t)nsys);
    return (int)a.err;
}
int su_front_back6(int nsys, int nown, int nb, int nvert, const int32_t* vtx, double* xt, const double* f, const double* r)
{
    return front_back_call<6>(nsys, nown, nb, nvert, vtx, xt, f, r);
}
int su_front_back7(int nsys, int nown, int nb, int nvert, const int32_t* vtx, double* xt, const double* f, const double* r)
{
    return front_back_call<7>(nsys, nown, nb, nvert, vtx, xt, f, r);
}

int su_mono(const double* t7, const double* x3, const double* obs2, const double* cam4, double* out20, int n)
{
    Arena a;
    const double* d_t = a.dev(t7, (size_t)n * 7);
    const double* d_x = a.dev(x3, (size_t)n * 3);
    const double* d_o = a.dev(obs2, (size_t)n * 2);
    const double* d_c = a.dev(cam4, 4);
    double* d_out = a.dev<double>(nullptr, (size_t)n * 20);
    if (a.err == hipSuccess) {
        k_mono<<<grid_of(n), TPB>>>(d_t, d_x, d_o, d_c, d_out, n);
        a.ran();
    }
    a.back(out20, d_out, (size_t)n * 20);
    return (int)a.err;
}
int su_marker(const float* tcw12, const float* twm12, const double* p3, const double* obs2, const double* cam4, double* out26, int n)
{
    Arena a;
    const float* d_c = a.dev(tcw12, (size_t)n * 12);
    const float* d_m = a.dev(twm12, (size_t)n * 12);
    const double* d_p = a.dev(p3, (size_t)n * 3);
    const double* d_o = a.dev(obs2, (size_t)n * 2);
    const double* d_k = a.dev(cam4, 4);
    double* d_out = a.dev<double>(nullptr, (size_t)n * 26);
    if (a.err == hipSuccess) {
        k_marker<<<grid_of(n), TPB>>>(d_c, d_m, d_p, d_o, d_k, d_out, n);
        a.ran();
    }
    a.back(out26, d_out, (size_t)n * 26);
    return (int)a.err;
}
int su_diag(const double* in15, double* out27, int n) { return call1(k_diag, in15, 15, out27, 27, n); }
int su_rot_of(const double* q4, double* r9, int n) { return call1(k_rot_of, q4, 4, r9, 9, n); }
int su_dinv3(const double* in7, double* d9, int n) { return call1(k_dinv3, in7, 7, d9, 9, n); }
int su_pair_items(const double* w, const double* d, const double* bl, int nitems, int diag, double* acc36, double* accb6, int nsys)
{
    Arena a;
    const double* d_w = a.dev(w, (size_t)nsys * nitems * 36);
    const double* d_d = a.dev(d, (size_t)nsys * nitems * 9);
    const double* d_b = a.dev(bl, (size_t)nsys * nitems * 3);
    double* d_acc = a.dev(acc36, (size_t)nsys * 36);
    double* d_accb = a.dev(accb6, (size_t)nsys * 6);
    if (a.err == hipSuccess && nsys > 0) {
        k_pair_items<<<grid_of(nsys), TPB>>>(d_w, d_d, d_b, nitems, diag, d_acc, d_accb, nsys);
        a.ran();
    }
    a.back(acc36, d_acc, (size_t)nsys * 36);
    a.back(accb6, d_accb, (size_t)nsys * 6);
    return (int)a.err;
}
// desc: nn x 7 = front (in doubles), nown, nb, child[2], cmap[2]; fronts (nfronts doubles) in / out.  The caller has checked that every
// front and every map entry lies inside (solver_units_build.merge).
int su_merge(int R, const int32_t* desc, int nn, const int32_t* cmap, int ncmap, double* fronts, int nfronts, int node)
{
    if ((R != 6 && R != 7) || node < 0 || node >= nn) return (int)hipErrorInvalidValue;
    std::vector<FrontNode> nodes((size_t)nn);
    for (int i = 0; i < nn; i++) {
        const int32_t* d = desc + 7 * i;
        FrontNode nd = {};
        nd.front = d[0]; nd.nown = d[1]; nd.nb = d[2];
        nd.child[0] = d[3]; nd.child[1] = d[4]; nd.cmap[0] = d[5]; nd.cmap[1] = d[6];
        nodes[(size_t)i] = nd;
    }
    Arena a;
    const FrontNode* d_nodes = a.dev(nodes.data(), (size_t)nn);
    const int32_t* d_cmap = a.dev(cmap, (size_t)ncmap);
    double* d_f = a.dev(fronts, (size_t)nfronts);
    if (a.err == hipSuccess) {
        if (R == 6) k_merge<6><<<1, LM_THREADS>>>(d_nodes, node, d_cmap, d_f);
        else k_merge<7><<<1, LM_THREADS>>>(d_nodes, node, d_cmap, d_f);
        a.ran();
    }
    a.back(fronts, d_f, (size_t)nfronts);
    return (int)a.err;
}
int su_run_sum(const double* v, int n, double* out)
{
    Arena a;
    const double* d_v = a.dev(v, (size_t)n);
    double* d_out = a.dev<double>(nullptr, 1);
    if (a.err == hipSuccess) {
        k_run_sum<<<1, LM_THREADS>>>(d_v, n, d_out);
        a.ran();
    }
    a.back(out, d_out, 1);
    return (int)a.err;
}
int su_wave(int op, const double* in, double* out, int n)
{
    if (n % 64) return (int)hipErrorInvalidValue;
    Arena a;
    const double* d_in = a.dev(in, (size_t)n);
    double* d_out = a.dev<double>(nullptr, (size_t)n);
    if (a.err == hipSuccess) {
        k_wave<<<grid_of(n), TPB>>>(op, d_in, d_out, n);
        a.ran();
    }
    a.back(out, d_out, (size_t)n);
    return (int)a.err;
}

} // extern "C"
#pragma GCC visibility pop
