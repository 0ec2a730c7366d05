// new_points_ref.cpp -- CPU restatement of the geometry of LocalMapping::CreateNewMapPoints (monocular) for the parity tests of
// orbfe_new_points_* / orbfe_triangulate_matches_* / orbfe_create_new_map_points*.  No OpenCV here: the pieces the reference runs
// through are restated from their algorithms and OpenCV 3.4's numeric conventions for CV_32F -- Mat products and dot products
// accumulate in double and round once, cv::norm is a double sum of float squares and a double square root, 3 x 3 inverses are
// cofactor formulas in double, "m / s" multiplies by (float)(1. / s), cv::SVD is the one-sided Jacobi (double sums of float
// products, float rotations, FLT_EPSILON * 2).  One pair at a time: the tests walk a keyframe's neighbours in order and run the
// oracle's SearchForTriangulation between the calls, as the reference does.
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

namespace {

struct KeyPoint {
    float x, y, size, angle, response;
    int32_t octave, class_id;
};

// singular value decomposition of a 4 x 4 float matrix given transposed (At = A^T): Vt rows = right singular vectors, by descending
// singular value.  One-sided Jacobi on the rows of At.
void svd4(float At[4][4], float Vt[4][4])
{
    const int N = 4, M = 4;
    const float eps = FLT_EPSILON * 2;
    double W[4];
    for (int i = 0; i < N; i++) {
        double sd = 0;
        for (int k = 0; k < M; k++) sd += (double)At[i][k] * At[i][k];
        W[i] = sd;
        for (int k = 0; k < N; k++) Vt[i][k] = 0;
        Vt[i][i] = 1;
    }
    for (int iter = 0; iter < 30; iter++) {
        bool changed = false;
        for (int i = 0; i < N - 1; i++)
            for (int j = i + 1; j < N; j++) {
                double a = W[i], p = 0, b = W[j];
                for (int k = 0; k < M; k++) p += (double)At[i][k] * At[j][k];
                if (std::fabs(p) <= eps * std::sqrt(a * b)) continue;
                p *= 2;
                const double beta = a - b, gamma = hypot(p, beta);
                float c, s;
                if (beta < 0) {
                    const double delta = (gamma - beta) * 0.5;
                    s = (float)std::sqrt(delta / gamma);
                    c = (float)(p / (gamma * s * 2));
                } else {
                    c = (float)std::sqrt((gamma + beta) / (gamma * 2));
                    s = (float)(p / (gamma * c * 2));
                }
                a = b = 0;
                for (int k = 0; k < M; k++) {
                    const float t0 = c * At[i][k] + s * At[j][k];
                    const float t1 = -s * At[i][k] + c * At[j][k];
                    At[i][k] = t0; At[j][k] = t1;
                    a += (double)t0 * t0; b += (double)t1 * t1;
                }
                W[i] = a; W[j] = b;
                changed = true;
                for (int k = 0; k < N; k++) {
                    const float t0 = c * Vt[i][k] + s * Vt[j][k];
                    const float t1 = -s * Vt[i][k] + c * Vt[j][k];
                    Vt[i][k] = t0; Vt[j][k] = t1;
                }
            }
        if (!changed) break;
    }
    for (int i = 0; i < N; i++) {
        double sd = 0;
        for (int k = 0; k < M; k++) sd += (double)At[i][k] * At[i][k];
        W[i] = std::sqrt(sd);
    }
    for (int i = 0; i < N - 1; i++) {
        int j = i;
        for (int k = i + 1; k < N; k++)
            if (W[j] < W[k]) j = k;
        if (i != j) {
            std::swap(W[i], W[j]);
            for (int k = 0; k < M; k++) std::swap(At[i][k], At[j][k]);
            for (int k = 0; k < N; k++) std::swap(Vt[i][k], Vt[j][k]);
        }
    }
}

void mm3(const float* A, const float* B, float* C)
{
    float R[9];
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) {
            double s = 0;
            for (int k = 0; k < 3; k++) s += (double)A[r * 3 + k] * B[k * 3 + c];
            R[r * 3 + c] = (float)s;
        }
    memcpy(C, R, sizeof R);
}

void inv3(const float* S, float* D)
{
    double d = S[0] * ((double)S[4] * S[8] - (double)S[5] * S[7]) - S[1] * ((double)S[3] * S[8] - (double)S[5] * S[6]) +
               S[2] * ((double)S[3] * S[7] - (double)S[4] * S[6]);
    if (d == 0.) {
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
    for (int i = 0; i < 9; i++) D[i] = (float)t[i];
}

// Ow = -Rwc * tcw, T = [R | t] 3 x 4 row-major
void centre(const float* T, float* O)
{
    for (int r = 0; r < 3; r++) {
        double s = 0;
        for (int k = 0; k < 3; k++) s += (double)T[k * 4 + r] * T[k * 4 + 3];
        O[r] = (float)(s * -1.0);
    }
}

} // namespace

extern "C" {

// the gate and the search's inputs of one pair.  recf: baseline, median_depth; reci: n_depths, skipped
void nmp_ref_prepare(int n2, const float* x3Dw2, const uint8_t* valid2, const float* T1, const float* T2, const float* K4, float* F12,
                     float* epipole, float* recf, int32_t* reci)
{
    const float fx = K4[0], fy = K4[1], cx = K4[2], cy = K4[3];
    float O1[3], O2[3];
    centre(T1, O1);
    centre(T2, O2);
    const float b[3] = {O2[0] - O1[0], O2[1] - O1[1], O2[2] - O1[2]};
    const float baseline = (float)std::sqrt((double)b[0] * b[0] + (double)b[1] * b[1] + (double)b[2] * b[2]);
    std::vector<float> z;
    for (int i = 0; i < n2; i++) {
        if (valid2 && !valid2[i]) continue;
        const double d = (double)T2[8] * x3Dw2[3 * i] + (double)T2[9] * x3Dw2[3 * i + 1] + (double)T2[10] * x3Dw2[3 * i + 2];
        z.push_back((float)(d + (double)T2[11]));
    }
    std::sort(z.begin(), z.end());
    const float median = z.empty() ? 0.f : z[(z.size() - 1) / 2];
    const float ratio = baseline / median;
    const int skipped = z.empty() || (double)ratio < 0.01;
    recf[0] = baseline; recf[1] = median;
    reci[0] = (int32_t)z.size(); reci[1] = skipped;
    for (int i = 0; i < 9; i++) F12[i] = 0;
    epipole[0] = epipole[1] = 0;
    if (skipped) return;
    float R1[9], R2t[9], R12[9], M[9], t12[3];
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) { R1[r * 3 + c] = T1[r * 4 + c]; R2t[r * 3 + c] = T2[c * 4 + r]; }
    mm3(R1, R2t, R12);
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) {
            double s = 0;
            for (int k = 0; k < 3; k++) s += (double)R1[r * 3 + k] * R2t[k * 3 + c];
            M[r * 3 + c] = (float)(s * -1.0);
        }
    for (int r = 0; r < 3; r++) {
        double s = 0;
        for (int k = 0; k < 3; k++) s += (double)M[r * 3 + k] * T2[k * 4 + 3];
        t12[r] = (float)(s + (double)T1[r * 4 + 3]);
    }
    const float t12x[9] = {0, -t12[2], t12[1], t12[2], 0, -t12[0], -t12[1], t12[0], 0};
    const float Kt[9] = {fx, 0, 0, 0, fy, 0, cx, cy, 1}, K[9] = {fx, 0, cx, 0, fy, cy, 0, 0, 1};
    float Kti[9], Ki[9], A[9];
    inv3(Kt, Kti);
    inv3(K, Ki);
    mm3(Kti, t12x, A);
    mm3(A, R12, A);
    mm3(A, Ki, F12);
    float C2[3];
    for (int r = 0; r < 3; r++) {
        double s = 0;
        for (int k = 0; k < 3; k++) s += (double)T2[r * 4 + k] * O1[k];
        C2[r] = (float)(s + (double)T2[r * 4 + 3]);
    }
    const float invz = 1.0f / C2[2];
    epipole[0] = fx * C2[0] * invz + cx;
    epipole[1] = fy * C2[1] * invz + cy;
}

// the triangulation of one pair's match list, in ascending i1.  status (n1), x3D / normal (n1 x 3), dist (n1 x 2), q (n1 x 6: cos,
// err1, err2, dist1, dist2, ratioOctave; 0 behind the rejecting gate) -- all written, zeros where nothing applies.  res3: n_matches,
// n_new, status.  The map state (x3Dw*, valid*: may be NULL together) is updated where a point is created.  An octave outside
// [0, nlevels) on a matched feature: returns -1 with res3 = {0, 0, -1} and nothing else written.
int nmp_ref_triangulate(const KeyPoint* k1, int n1, float* x3Dw1, uint8_t* valid1, const float* T1, const KeyPoint* k2, int n2, float* x3Dw2,
                        uint8_t* valid2, const float* T2, const int32_t* m12, const float* K4, const float* sf, const float* sg, int nlevels,
                        float ratio_factor, uint8_t* status, float* x3D, float* normal, float* dist, float* q, int32_t* res3)
{
    res3[0] = res3[1] = res3[2] = 0;
    for (int i = 0; i < n1; i++) {
        const int j = m12[i];
        if (j < 0 || j >= n2) continue;
        if (k1[i].octave < 0 || k1[i].octave >= nlevels || k2[j].octave < 0 || k2[j].octave >= nlevels) { res3[2] = -1; return -1; }
    }
    const float fx = K4[0], fy = K4[1], cx = K4[2], cy = K4[3];
    const float invfx = 1.0f / fx, invfy = 1.0f / fy;
    float O1[3], O2[3];
    centre(T1, O1);
    centre(T2, O2);
    for (int i1 = 0; i1 < n1; i1++) {
        status[i1] = 0;
        for (int k = 0; k < 3; k++) x3D[3 * i1 + k] = normal[3 * i1 + k] = 0;
        dist[2 * i1] = dist[2 * i1 + 1] = 0;
        float* Q = q + 6 * i1;
        for (int k = 0; k < 6; k++) Q[k] = 0;
        const int i2 = m12[i1];
        if (i2 < 0 || i2 >= n2) continue;
        res3[0]++;
        const float k1x = k1[i1].x, k1y = k1[i1].y, k2x = k2[i2].x, k2y = k2[i2].y;
        const float xn1[3] = {(k1x - cx) * invfx, (k1y - cy) * invfy, 1.0f}, xn2[3] = {(k2x - cx) * invfx, (k2y - cy) * invfy, 1.0f};
        float ray1[3], ray2[3];
        for (int i = 0; i < 3; i++) {
            ray1[i] = (float)((double)T1[i] * xn1[0] + (double)T1[4 + i] * xn1[1] + (double)T1[8 + i] * xn1[2]);
            ray2[i] = (float)((double)T2[i] * xn2[0] + (double)T2[4 + i] * xn2[1] + (double)T2[8 + i] * xn2[2]);
        }
        const double dot = (double)ray1[0] * ray2[0] + (double)ray1[1] * ray2[1] + (double)ray1[2] * ray2[2];
        const double nr1 = std::sqrt((double)ray1[0] * ray1[0] + (double)ray1[1] * ray1[1] + (double)ray1[2] * ray1[2]);
        const double nr2 = std::sqrt((double)ray2[0] * ray2[0] + (double)ray2[1] * ray2[1] + (double)ray2[2] * ray2[2]);
        const float cosv = (float)(dot / (nr1 * nr2));
        Q[0] = cosv;
        if (!(cosv > 0 && (double)cosv < 0.9998)) { status[i1] = 2; continue; }
        float At[4][4], Vt[4][4];
        for (int c = 0; c < 4; c++) {
            At[c][0] = (float)((double)T1[8 + c] * xn1[0] - (double)T1[c]);
            At[c][1] = (float)((double)T1[8 + c] * xn1[1] - (double)T1[4 + c]);
            At[c][2] = (float)((double)T2[8 + c] * xn2[0] - (double)T2[c]);
            At[c][3] = (float)((double)T2[8 + c] * xn2[1] - (double)T2[4 + c]);
        }
        svd4(At, Vt);
        if (Vt[3][3] == 0) { status[i1] = 3; continue; }
        const float iw = (float)(1. / (double)Vt[3][3]);
        const float X[3] = {Vt[3][0] * iw, Vt[3][1] * iw, Vt[3][2] * iw};
        if (!std::isfinite(X[0]) || !std::isfinite(X[1]) || !std::isfinite(X[2])) { status[i1] = 4; continue; }
        float c1[3], c2[3];
        for (int i = 0; i < 3; i++) {
            c1[i] = (float)((double)T1[i * 4] * X[0] + (double)T1[i * 4 + 1] * X[1] + (double)T1[i * 4 + 2] * X[2] + (double)T1[i * 4 + 3]);
            c2[i] = (float)((double)T2[i * 4] * X[0] + (double)T2[i * 4 + 1] * X[1] + (double)T2[i * 4 + 2] * X[2] + (double)T2[i * 4 + 3]);
        }
        if (c1[2] <= 0) { status[i1] = 5; continue; }
        if (c2[2] <= 0) { status[i1] = 6; continue; }
        const float invz1 = (float)(1.0 / (double)c1[2]);
        const float u1 = fx * c1[0] * invz1 + cx, v1 = fy * c1[1] * invz1 + cy;
        const float ex1 = u1 - k1x, ey1 = v1 - k1y;
        const float e1 = ex1 * ex1 + ey1 * ey1;
        Q[1] = e1;
        if ((double)e1 > 5.991 * (double)sg[k1[i1].octave]) { status[i1] = 7; continue; }
        const float invz2 = (float)(1.0 / (double)c2[2]);
        const float u2 = fx * c2[0] * invz2 + cx, v2 = fy * c2[1] * invz2 + cy;
        const float ex2 = u2 - k2x, ey2 = v2 - k2y;
        const float e2 = ex2 * ex2 + ey2 * ey2;
        Q[2] = e2;
        if ((double)e2 > 5.991 * (double)sg[k2[i2].octave]) { status[i1] = 8; continue; }
        const float na[3] = {X[0] - O1[0], X[1] - O1[1], X[2] - O1[2]}, nb[3] = {X[0] - O2[0], X[1] - O2[1], X[2] - O2[2]};
        const double d1 = std::sqrt((double)na[0] * na[0] + (double)na[1] * na[1] + (double)na[2] * na[2]);
        const double d2 = std::sqrt((double)nb[0] * nb[0] + (double)nb[1] * nb[1] + (double)nb[2] * nb[2]);
        const float dist1 = (float)d1, dist2 = (float)d2;
        Q[3] = dist1; Q[4] = dist2;
        if (dist1 == 0 || dist2 == 0) { status[i1] = 9; continue; }
        const float sf1 = sf[k1[i1].octave], sf2 = sf[k2[i2].octave];
        const float ratioDist = dist2 / dist1, ratioOctave = sf1 / sf2;
        Q[5] = ratioOctave;
        if (ratioDist * ratio_factor < ratioOctave || ratioDist > ratioOctave * ratio_factor) { status[i1] = 10; continue; }
        const float a1 = (float)(1. / d1), a2 = (float)(1. / d2);
        for (int i = 0; i < 3; i++) {
            normal[3 * i1 + i] = ((0.f + na[i] * a1) + nb[i] * a2) * 0.5f;
            x3D[3 * i1 + i] = X[i];
        }
        dist[2 * i1] = dist1 * sf1;
        dist[2 * i1 + 1] = dist[2 * i1] / sf[nlevels - 1];
        status[i1] = 1;
        res3[1]++;
        if (x3Dw1) {
            valid1[i1] = 1; valid2[i2] = 1;
            for (int i = 0; i < 3; i++) x3Dw1[3 * i1 + i] = x3Dw2[3 * i2 + i] = X[i];
        }
    }
    return 0;
}

} // extern "C"
