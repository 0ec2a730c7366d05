// TEST INFRASTRUCTURE ONLY -- a CPU restatement of ORB_SLAM2::Sim3Solver (the algorithm of src/Sim3Solver.cc: constructor,
// SetRansacParameters, iterate, ComputeSim3, CheckInliers, Project) on flat arrays, with OpenCV 3.4's CV_32F arithmetic written out:
// the parity oracle of csrc/sim3_solver.hip (tests/test_sim3_gpu.py) and the subject of tests/test_sim3_cpu.py.  Written on its own:
// it shares no code with the device file, and its eigen solver keeps OpenCV's pivot caches (indR / indC), which the device's does not.
// Build: g++ -O2 -ffp-contract=off (tests/sim3_build.py).
//
// Arithmetic: a Mat product sums float products in double in index order, scales by alpha, adds beta * C, rounds once; a Mat
// scaled by a scalar multiplies in float by the scalar rounded to float; cv::reduce sums floats left to right; cv::norm and Mat::dot
// sum in double; cv::Rodrigues works in double; cv::eigen is the float Jacobi method of modules/core/src/lapack.cpp.
// The chi-square gates are stored as size_t by the reference (include/Sim3Solver.h:78-79): 9.210 * sigma2 truncated.
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <utility>
#include <vector>

namespace {

struct Kp { float x, y, size, angle, response; int32_t octave, class_id; };

struct Result {
    int32_t n, max_iterations, no_more, found, n_inliers, best, best_inliers;
    float s12, R12[9], t12[3], T12[16];
    int32_t status;
};

struct Vec3 { float v[3]; };
struct Pix { float u, v; };

// ---- OpenCV pieces ----
// y = alpha * (A x) + beta * c, A rows x 3 with row stride lda
float prod_row(const float* a, const float* x, double alpha, float c, double beta)
{
    double s = 0;
    for (int k = 0; k < 3; k++) s += (double)a[k] * (double)x[k];
    return (float)(s * alpha + (double)c * beta);
}

float hyp(float a, float b)
{
    a = std::fabs(a); b = std::fabs(b);
    if (a > b) { b /= a; return a * std::sqrt(1 + b * b); }
    if (b > 0) { a /= b; return b * std::sqrt(1 + a * a); }
    return 0;
}

// Jacobi eigenvalue method for a symmetric n x n float matrix (row-major A, destroyed); W: eigenvalues descending, V: eigenvectors
// in rows.  The pivot is looked up through per-row (indR) and per-column (indC) caches of the largest off-diagonal element that
// are refreshed for the two rotated indices only.
void jacobi_eigen(float* A, int n, float* W, float* V)
{
    const float eps = FLT_EPSILON;
    std::vector<int> indR(n), indC(n);
    for (int i = 0; i < n; i++)
        for (int j = 0; j < n; j++) V[i * n + j] = i == j ? 1.f : 0.f;
    auto refresh = [&](int k) {
        if (k < n - 1) {
            int m = k + 1;
            float mv = std::fabs(A[n * k + m]);
            for (int i = k + 2; i < n; i++) {
                const float val = std::fabs(A[n * k + i]);
                if (mv < val) { mv = val; m = i; }
            }
            indR[k] = m;
        }
        if (k > 0) {
            int m = 0;
            float mv = std::fabs(A[k]);
            for (int i = 1; i < k; i++) {
                const float val = std::fabs(A[n * i + k]);
                if (mv < val) { mv = val; m = i; }
            }
            indC[k] = m;
        }
    };
    for (int k = 0; k < n; k++) {
        W[k] = A[(n + 1) * k];
        refresh(k);
    }
    const int maxIters = n * n * 30;
    if (n > 1)
        for (int iters = 0; iters < maxIters; iters++) {
            int k = 0;
            float mv = std::fabs(A[indR[0]]);
            for (int i = 1; i < n - 1; i++) {
                const float val = std::fabs(A[n * i + indR[i]]);
                if (mv < val) { mv = val; k = i; }
            }
            int l = indR[k];
            for (int i = 1; i < n; i++) {
                const float val = std::fabs(A[n * indC[i] + i]);
                if (mv < val) { mv = val; k = indC[i]; l = i; }
            }
            const float p = A[n * k + l];
            if (std::fabs(p) <= eps) break;
            const float y = (float)((W[l] - W[k]) * 0.5);
            float t = std::fabs(y) + hyp(p, y);
            float s = hyp(p, t);
            const float c = t / s;
            s = p / s;
            t = (p / t) * p;
            if (y < 0) { s = -s; t = -t; }
            A[n * k + l] = 0;
            W[k] -= t;
            W[l] += t;
            auto rot = [&](float& v0, float& v1) {
                const float a0 = v0, b0 = v1;
                v0 = a0 * c - b0 * s;
                v1 = a0 * s + b0 * c;
            };
            for (int i = 0; i < k; i++) rot(A[n * i + k], A[n * i + l]);
            for (int i = k + 1; i < l; i++) rot(A[n * k + i], A[n * i + l]);
            for (int i = l + 1; i < n; i++) rot(A[n * k + i], A[n * l + i]);
            for (int i = 0; i < n; i++) rot(V[n * k + i], V[n * l + i]);
            refresh(k);
            refresh(l);
        }
    for (int k = 0; k < n - 1; k++) {
        int m = k;
        for (int i = k + 1; i < n; i++)
            if (W[m] < W[i]) m = i;
        if (k != m) {
            std::swap(W[m], W[k]);
            for (int i = 0; i < n; i++) std::swap(V[n * m + i], V[n * k + i]);
        }
    }
}

void rodrigues(const float* rv, float* R)
{
    double r[3] = {rv[0], rv[1], rv[2]};
    const double theta = std::sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]);
    if (theta < DBL_EPSILON) {
        for (int i = 0; i < 9; i++) R[i] = i % 4 == 0 ? 1.f : 0.f;
        return;
    }
    const double c = std::cos(theta), s = std::sin(theta), c1 = 1. - c, it = 1. / theta;
    for (double& x : r) x *= it;
    const double rrt[9] = {r[0] * r[0], r[0] * r[1], r[0] * r[2], r[0] * r[1], r[1] * r[1], r[1] * r[2], r[0] * r[2], r[1] * r[2], r[2] * r[2]};
    const double rx[9] = {0, -r[2], r[1], r[2], 0, -r[0], -r[1], r[0], 0};
    for (int i = 0; i < 9; i++) R[i] = (float)((c * (i % 4 == 0 ? 1. : 0.) + c1 * rrt[i]) + s * rx[i]);
}

// ---- the solver ----
struct Model {
    bool degenerate;
    float s, R[9], t[3], T12[12], T21[12];
    float l1, l2;   // the two largest eigenvalues of N
};

struct Solver {
    int n1 = 0, N = 0;
    std::vector<Vec3> X1, X2;
    std::vector<Pix> P1, P2;
    std::vector<float> e1, e2;
    std::vector<int> idx1;
    float K1[4], K2[4];
    bool fix_scale = true;
    int min_inliers = 6, max_its = 300;

    static Vec3 transform(const float* T, const float* x)
    {
        Vec3 o;
        for (int r = 0; r < 3; r++) o.v[r] = prod_row(T + 4 * r, x, 1.0, T[4 * r + 3], 1.0);
        return o;
    }
    static Pix image(const Vec3& X, const float* K)
    {
        const float invz = 1 / X.v[2];
        const float x = X.v[0] * invz, y = X.v[1] * invz;
        return Pix{K[0] * x + K[2], K[1] * y + K[3]};
    }

    // returns false on an octave outside the level table
    bool construct(const Kp* k1, int n1_, const float* x1, const uint8_t* v1, const float* Tcw1, const Kp* k2, int n2, const float* x2,
                   const uint8_t* v2, const float* Tcw2, const int32_t* m12, const float* ls2, int nlevels)
    {
        n1 = n1_;
        for (int i1 = 0; i1 < n1; i1++) {
            const int i2 = m12[i1];
            if (i2 < 0 || i2 >= n2) continue;
            if (v1 && (!v1[i1] || !v2[i2])) continue;
            const int o1 = k1[i1].octave, o2 = k2[i2].octave;
            if (o1 < 0 || o1 >= nlevels || o2 < 0 || o2 >= nlevels) return false;
            e1.push_back((float)(size_t)(9.210 * ls2[o1]));
            e2.push_back((float)(size_t)(9.210 * ls2[o2]));
            idx1.push_back(i1);
            X1.push_back(transform(Tcw1, x1 + 3 * i1));
            X2.push_back(transform(Tcw2, x2 + 3 * i2));
        }
        N = (int)idx1.size();
        for (int i = 0; i < N; i++) {
            P1.push_back(image(X1[i], K1));
            P2.push_back(image(X2[i], K2));
        }
        return true;
    }

    void set_ransac(double probability, int minInliers, int maxIterations)
    {
        min_inliers = minInliers;
        int its = 1;
        if (N > 0 && minInliers != N) {
            const float epsilon = (float)minInliers / N;
            const double nit = std::ceil(std::log(1 - probability) / std::log(1 - std::pow((double)epsilon, 3)));
            // not finite or below 1 (undefined in the reference): 1
            its = nit >= (double)maxIterations ? maxIterations : nit >= 1 ? (int)nit : 1;
        }
        max_its = its < 1 ? 1 : its;
    }

    Model horn(const int* set) const
    {
        Model m{};
        float A[3][3], B[3][3], Oa[3], Ob[3];   // A: set 1, B: set 2; [coordinate][point]
        for (int i = 0; i < 3; i++)
            for (int r = 0; r < 3; r++) { A[r][i] = X1[set[i]].v[r]; B[r][i] = X2[set[i]].v[r]; }
        const float third = (float)(1.0 / 3);
        for (int r = 0; r < 3; r++) {
            float sa = A[r][0]; sa += A[r][1]; sa += A[r][2];
            float sb = B[r][0]; sb += B[r][1]; sb += B[r][2];
            Oa[r] = sa * third; Ob[r] = sb * third;
            for (int i = 0; i < 3; i++) { A[r][i] = A[r][i] - Oa[r]; B[r][i] = B[r][i] - Ob[r]; }
        }
        float M[3][3];
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++) {
                double s = 0;
                for (int k = 0; k < 3; k++) s += (double)B[i][k] * (double)A[j][k];
                M[i][j] = (float)s;
            }
        double n11 = M[0][0] + (double)M[1][1] + M[2][2], n12 = (double)M[1][2] - M[2][1], n13 = (double)M[2][0] - M[0][2];
        double n14 = (double)M[0][1] - M[1][0], n22 = (double)M[0][0] - M[1][1] - M[2][2], n23 = (double)M[0][1] + M[1][0];
        double n24 = (double)M[2][0] + M[0][2], n33 = -(double)M[0][0] + M[1][1] - M[2][2], n34 = (double)M[1][2] + M[2][1];
        double n44 = -(double)M[0][0] - M[1][1] + M[2][2];
        float Nm[16] = {(float)n11, (float)n12, (float)n13, (float)n14, (float)n12, (float)n22, (float)n23, (float)n24,
                        (float)n13, (float)n23, (float)n33, (float)n34, (float)n14, (float)n24, (float)n34, (float)n44};
        float W[4], V[16];
        jacobi_eigen(Nm, 4, W, V);
        m.l1 = W[0]; m.l2 = W[1];
        float vec[3] = {V[1], V[2], V[3]};
        double nn = 0;
        for (float x : vec) nn += (double)x * (double)x;
        const double nrm = std::sqrt(nn);
        if (!(nrm > 0) || !std::isfinite(nrm)) { m.degenerate = true; return m; }
        const double ang = std::atan2(nrm, (double)V[0]);
        const float k = (float)((2 * ang) * (1. / nrm));
        for (float& x : vec) x = x * k;
        rodrigues(vec, m.R);
        m.s = 1.0f;
        if (!fix_scale) {
            float P3[3][3];
            for (int r = 0; r < 3; r++)
                for (int i = 0; i < 3; i++) {
                    double s = 0;
                    for (int q = 0; q < 3; q++) s += (double)m.R[3 * r + q] * (double)B[q][i];
                    P3[r][i] = (float)s;
                }
            double nom = 0, den = 0;
            for (int r = 0; r < 3; r++)
                for (int i = 0; i < 3; i++) nom += (double)A[r][i] * (double)P3[r][i];
            for (int r = 0; r < 3; r++)
                for (int i = 0; i < 3; i++) { const float sq = P3[r][i] * P3[r][i]; den += sq; }
            m.s = (float)(nom / den);
        }
        for (int r = 0; r < 3; r++) m.t[r] = prod_row(m.R + 3 * r, Ob, -(double)m.s, Oa[r], 1.0);
        const float inv = (float)(1.0 / m.s);
        float sRi[9];
        for (int r = 0; r < 3; r++)
            for (int c = 0; c < 3; c++) sRi[3 * r + c] = m.R[3 * c + r] * inv;
        for (int r = 0; r < 3; r++) {
            for (int c = 0; c < 3; c++) { m.T12[4 * r + c] = m.R[3 * r + c] * m.s; m.T21[4 * r + c] = sRi[3 * r + c]; }
            m.T12[4 * r + 3] = m.t[r];
            m.T21[4 * r + 3] = prod_row(sRi + 3 * r, m.t, -1.0, 0.f, 0.0);
        }
        return m;
    }

    int check(const Model& m, std::vector<bool>& flags) const
    {
        int n = 0;
        flags.assign(N, false);
        if (m.degenerate) return 0;
        for (int i = 0; i < N; i++) {
            const Pix a = image(transform(m.T12, X2[i].v), K1);   // point of 2 in image 1
            const Pix b = image(transform(m.T21, X1[i].v), K2);   // point of 1 in image 2
            const float d1[2] = {P1[i].u - a.u, P1[i].v - a.v}, d2[2] = {b.u - P2[i].u, b.v - P2[i].v};
            const float err1 = (float)((double)d1[0] * d1[0] + (double)d1[1] * d1[1]);
            const float err2 = (float)((double)d2[0] * d2[0] + (double)d2[1] * d2[1]);
            if (err1 < e1[i] && err2 < e2[i]) { flags[i] = true; n++; }
        }
        return n;
    }
};

void decode(const int32_t* w, int N, int K, int* out)
{
    std::vector<int> avail(N);
    for (int i = 0; i < N; i++) avail[i] = i;
    for (int j = 0; j < K; j++) {
        const int d = (int)avail.size();
        const int randi = (int)(((double)w[j] / ((double)2147483647 + 1.0)) * d);
        out[j] = avail[randi];
        avail[randi] = avail.back();
        avail.pop_back();
    }
}

} // namespace

extern "C" {

__attribute__((visibility("default"))) void ref_sim3_decode_sets(int N, int iterations, const int32_t* words, int32_t* out)
{
    for (int it = 0; it < iterations; it++) decode(words + 3 * it, N, 3, out + 3 * it);
}

// One iterate() window.  Every hypothesis of the window is evaluated (models: x 13 = s12, R12, t12; counts; eig: x 2), the decision
// is the sequential one.  Returns N, or -1 for an octave outside the level table.
__attribute__((visibility("default"))) int ref_sim3(const Kp* k1, int n1, const float* x1, const uint8_t* v1, const float* Tcw1,
                                                    const float* K1, const Kp* k2, int n2, const float* x2, const uint8_t* v2,
                                                    const float* Tcw2, const float* K2, const int32_t* m12, const float* ls2, int nlevels,
                                                    int fix_scale, double probability, int min_inliers, int max_iterations, int first,
                                                    int n_iterations, int best_in, const int32_t* words, Result* res, uint8_t* inl12,
                                                    int32_t* idx1, float* X1, float* X2, float* P1, float* P2, float* e1, float* e2,
                                                    int32_t* sets, float* models, int32_t* counts, float* eig)
{
    Solver S;
    memcpy(S.K1, K1, 16);
    memcpy(S.K2, K2, 16);
    S.fix_scale = fix_scale != 0;
    if (!S.construct(k1, n1, x1, v1, Tcw1, k2, n2, x2, v2, Tcw2, m12, ls2, nlevels)) return -1;
    S.set_ransac(probability, min_inliers, max_iterations);
    const int N = S.N;
    for (int i = 0; i < N; i++) {
        idx1[i] = S.idx1[i]; e1[i] = S.e1[i]; e2[i] = S.e2[i];
        memcpy(X1 + 3 * i, S.X1[i].v, 12); memcpy(X2 + 3 * i, S.X2[i].v, 12);
        P1[2 * i] = S.P1[i].u; P1[2 * i + 1] = S.P1[i].v; P2[2 * i] = S.P2[i].u; P2[2 * i + 1] = S.P2[i].v;
    }
    Result r{};
    r.n = N;
    r.max_iterations = S.max_its;
    r.found = r.best = -1;
    r.best_inliers = best_in;
    memset(inl12, 0, (size_t)n1);
    if (N < min_inliers || N < 3) {
        r.no_more = 1;
        *res = r;
        return N;
    }
    int it = first, done = 0, best = best_in;
    bool decided = false;
    std::vector<bool> flags;
    while (it < S.max_its && done < n_iterations) {
        int* set = sets + 3 * done;
        decode(words + 3 * done, N, 3, set);
        const Model m = S.horn(set);
        const int c = S.check(m, flags);
        float* mo = models + 13 * done;
        if (!m.degenerate) { mo[0] = m.s; memcpy(mo + 1, m.R, 36); memcpy(mo + 10, m.t, 12); }
        counts[done] = c;
        eig[2 * done] = m.l1; eig[2 * done + 1] = m.l2;
        if (!decided && !m.degenerate && c >= best) {
            best = c;
            r.best = it; r.best_inliers = c;
            r.s12 = m.s; memcpy(r.R12, m.R, 36); memcpy(r.t12, m.t, 12);
            memcpy(r.T12, m.T12, 48); r.T12[12] = r.T12[13] = r.T12[14] = 0; r.T12[15] = 1;
            if (c > min_inliers) {
                r.found = it; r.n_inliers = c;
                for (int i = 0; i < N; i++)
                    if (flags[i]) inl12[S.idx1[i]] = 1;
                decided = true;
            }
        }
        it++; done++;
    }
    if (!decided && it >= S.max_its) r.no_more = 1;
    *res = r;
    return N;
}

}
