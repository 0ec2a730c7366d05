// solver_units_host.cpp -- test infrastructure: the SE3Quat pieces of tests/g2o_ref.hpp (the CPU restatement, glibc's libm) behind the
// array calls tests/solver_units_probe.hip gives the device's, for tests/solver_units_build.py.  An SE3 is 7 doubles: q (x y z w), t.
// Behind them, sequential restatements of the steps the bundle adjustments and the front solvers share (csrc/ba_edges.hpp,
// front_solve.hpp, lm_dense.hpp's run_sum), in the device's order of operations, under the probe's names and argument lists.
#include "g2o_ref.hpp"

#include <stdint.h>

#include <vector>

namespace {

SE3 se3_of(const double* a)
{
    SE3 T;
    T.q = Quat{a[0], a[1], a[2], a[3]};
    for (int i = 0; i < 3; i++) T.t[i] = a[4 + i];
    return T;
}
void se3_to(const SE3& T, double* a)
{
    a[0] = T.q.x; a[1] = T.q.y; a[2] = T.q.z; a[3] = T.q.w;
    for (int i = 0; i < 3; i++) a[4 + i] = T.t[i];
}

} // namespace

extern "C" {

int su_se3_exp(const double* u6, double* out7, int n)
{
    for (int i = 0; i < n; i++) se3_to(se3_exp(u6 + 6 * i), out7 + 7 * i);
    return 0;
}
int su_se3_mul(const double* a7, const double* b7, double* out7, int n)
{
    for (int i = 0; i < n; i++) se3_to(mul(se3_of(a7 + 7 * i), se3_of(b7 + 7 * i)), out7 + 7 * i);
    return 0;
}
int su_se3_map(const double* a7, const double* p3, double* out3, int n)
{
    for (int i = 0; i < n; i++) map(se3_of(a7 + 7 * i), p3 + 3 * i, out3 + 3 * i);
    return 0;
}
int su_normalize(const double* q4, double* out4, int n)
{
    for (int i = 0; i < n; i++) {
        Quat q = {q4[4 * i], q4[4 * i + 1], q4[4 * i + 2], q4[4 * i + 3]};
        normalize_rotation(q);
        out4[4 * i] = q.x; out4[4 * i + 1] = q.y; out4[4 * i + 2] = q.z; out4[4 * i + 3] = q.w;
    }
    return 0;
}
int su_se3_from_float(const float* Rt12, double* out7, int n)
{
    for (int i = 0; i < n; i++) se3_to(se3_from_float(Rt12 + 12 * i), out7 + 7 * i);
    return 0;
}
int su_to_float(const double* a7, float* Rt12, int n)
{
    for (int i = 0; i < n; i++) to_float(se3_of(a7 + 7 * i), Rt12 + 12 * i);
    return 0;
}

// the workgroup the device's sums are laid out for (csrc/lm_dense.hpp's LM_THREADS; the GPU test compares it with the probe's)
int su_lm_threads() { return 256; }

// (H + lambda I)^-1 of the packed upper triangle 00 01 02 11 12 22 by cofactors, row 0 of the adjugate giving the determinant
int su_dinv3(const double* in7, double* d9, int n)
{
    for (int i = 0; i < n; i++) {
        const double* H = in7 + 7 * i;
        const double l = H[6];
        const double a = H[0] + l, b = H[1], c = H[2], d = H[3] + l, e = H[4], f = H[5] + l;
        const double c00 = d * f - e * e, c10 = e * c - b * f, c20 = b * e - d * c;
        const double id = 1. / (c00 * a + c10 * b + c20 * c);
        double* D = d9 + 9 * i;
        D[0] = c00 * id; D[1] = c10 * id; D[2] = c20 * id;
        D[4] = (a * f - c * c) * id; D[5] = (c * b - a * e) * id; D[8] = (a * d - b * b) * id;
        D[3] = D[1]; D[6] = D[2]; D[7] = D[5];
    }
    return 0;
}

// acc += Wi D Wj^T (6 x 3, 3 x 3, 3 x 6), and on the diagonal accb += Wi D bl, item after item: Y = Wi D first, each entry a sum
// from the left
int su_pair_items(const double* w, const double* d, const double* bl, int nitems, int diag, double* acc36, double* accb6, int nsys)
{
    for (int i = 0; i < nsys; i++)
        for (int it = 0; it < nitems; it++) {
            const size_t q = (size_t)i * nitems + it;
            const double *Wi = w + q * 36, *Wj = Wi + 18, *D = d + q * 9, *b = bl + q * 3;
            for (int r = 0; r < 6; r++) {
                double Y[3];
                for (int c = 0; c < 3; c++) Y[c] = Wi[3 * r] * D[c] + Wi[3 * r + 1] * D[3 + c] + Wi[3 * r + 2] * D[6 + c];
                for (int c = 0; c < 6; c++) acc36[36 * i + 6 * r + c] += Y[0] * Wj[3 * c] + Y[1] * Wj[3 * c + 1] + Y[2] * Wj[3 * c + 2];
                if (diag) accb6[6 * i + r] += Y[0] * b[0] + Y[1] * b[1] + Y[2] * b[2];
            }
        }
    return 0;
}

// the Schur complements of the children of `node` added to its front, the left child and then the right: entry (i, j), i >= j, of a
// child's boundary block goes to (map i, map j) of the front, or to the transposed place when that lies above the diagonal
int su_merge(int R, const int32_t* desc, int nn, const int32_t* cmap, int ncmap, double* fronts, int nfronts, int node)
{
    (void)nn; (void)ncmap; (void)nfronts;
    const int32_t* nd = desc + 7 * node;
    const int n = R * (nd[1] + nd[2]);
    double* F = fronts + nd[0];
    double* r = F + (size_t)n * n;
    for (int ch = 0; ch < 2; ch++) {
        if (nd[3 + ch] < 0) continue;
        const int32_t* cn = desc + 7 * nd[3 + ch];
        const int m = R * (cn[1] + cn[2]), ck = R * cn[1], cb = R * cn[2];
        const double* G = fronts + cn[0];
        const int32_t* map = cmap + nd[5 + ch];
        for (int i = 0; i < cb; i++) {
            const int row = R * map[i / R] + i % R;
            for (int j = 0; j <= i; j++) {
                const int col = R * map[j / R] + j % R;
                const int hi = row > col ? row : col, lo = row > col ? col : row;
                F[(size_t)hi * n + lo] += G[(size_t)(ck + i) * m + ck + j];
            }
            r[row] += G[(size_t)m * m + ck + i];
        }
    }
    return 0;
}

// the sum of n doubles as a workgroup adds them: thread t the contiguous run [t per, (t + 1) per) from the left, per = ceil(n /
// threads); the 64 lanes of a wave by the butterfly lane ^= 32, 16, .. 1 (lane 0's value); the waves from the left
int su_run_sum(const double* v, int n, double* out)
{
    const int T = su_lm_threads(), per = (n + T - 1) / T;
    std::vector<double> part((size_t)T, 0.);
    for (int t = 0; t < T; t++)
        for (int i = t * per; i < n && i < (t + 1) * per; i++) part[(size_t)t] += v[i];
    double total = 0;
    for (int w = 0; w < T / 64; w++) {
        double lane[64], next[64];
        for (int l = 0; l < 64; l++) lane[l] = part[(size_t)w * 64 + l];
        for (int off = 32; off >= 1; off >>= 1) {
            for (int l = 0; l < 64; l++) next[l] = lane[l] + lane[l ^ off];
            for (int l = 0; l < 64; l++) lane[l] = next[l];
        }
        total = w == 0 ? lane[0] : total + lane[0];
    }
    out[0] = total;
    return 0;
}

} // extern "C"
