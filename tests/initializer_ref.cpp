// initializer_ref.cpp -- CPU restatement of ORB_SLAM2::Initializer (src/Initializer.cc of the reference) for the parity tests of
// orbfe_initialize*.  It follows Initializer.cc function by function, in float as the reference is, with the pieces of OpenCV 3.4
// it calls restated from their algorithms (no OpenCV here):
//   cv::SVDecomp / cv::SVD::compute, CV_32F   -> JacobiSVDImpl_ (one-sided Jacobi on the transposed matrix; double sums of float
//                                               products, float rotations, eps = FLT_EPSILON*2; rows sorted by descending
//                                               singular value; for FULL_UV the missing left vectors are completed from
//                                               RNG(0x12345678) vectors by Gram-Schmidt); m < n is solved transposed
//   Mat * Mat, CV_32F                         -> GEMMSingleMul<float, double>: double sums, one rounding (alpha before it)
//   Mat::inv() 3x3, cv::determinant 3x3       -> the cofactor formulas in double
//   cv::norm, Mat::dot                        -> double sums;  "m / s" -> convertTo with the float factor (float)(1. / s)
// Built by tests/initializer_build.py (g++ -O2 -ffp-contract=off) and loaded with ctypes.  Single-threaded: the reference's two
// threads (H, F) share no state.
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <utility>
#include <vector>

namespace {

struct KeyPoint {   // cv::KeyPoint layout
    float x, y, size, angle, response;
    int32_t octave, class_id;
};

struct Result {     // the layout of the library's result record
    int32_t initialized, model;
    float SH, SF, RH;
    int32_t best_h, best_f;
    float H21[9], F21[9], R21[9], t21[3];
    int32_t n_good;
    float parallax;
};

typedef std::pair<int, int> Match;

// ------------------------------------------------------------------------------------- OpenCV pieces --
struct Rng {
    uint64_t state;
    explicit Rng(uint64_t s) : state(s ? s : 0xffffffffull) {}
    unsigned next()
    {
        state = (uint64_t)(unsigned)state * 4164903690u + (unsigned)(state >> 32);
        return (unsigned)state;
    }
};

// JacobiSVDImpl_<float>: At is n rows of m (the transposed input) with n1 >= n rows of storage; W n; Vt n x n (may be null)
void jacobi_svd(float* At, int m, int n, int n1, float* Wout, float* Vt)
{
    const double minval = FLT_MIN;
    const float eps = FLT_EPSILON * 2;
    std::vector<double> W(n);
    for (int i = 0; i < n; i++) {
        double sd = 0;
        for (int k = 0; k < m; k++) { const float t = At[i * m + k]; sd += (double)t * t; }
        W[i] = sd;
        if (Vt) {
            for (int k = 0; k < n; k++) Vt[i * n + k] = 0;
            Vt[i * n + i] = 1;
        }
    }
    const int max_iter = std::max(m, 30);
    for (int iter = 0; iter < max_iter; iter++) {
        bool changed = false;
        for (int i = 0; i < n - 1; i++)
            for (int j = i + 1; j < n; j++) {
                float *Ai = At + i * m, *Aj = At + j * m;
                double a = W[i], p = 0, b = W[j];
                for (int k = 0; k < m; k++) p += (double)Ai[k] * Aj[k];
                if (std::abs(p) <= eps * std::sqrt((double)a * b)) continue;
                p *= 2;
                double beta = a - b, gamma = std::hypot(p, beta);
                float c, s;
                if (beta < 0) {
                    double delta = (gamma - beta) * 0.5;
                    s = (float)std::sqrt(delta / gamma);
                    c = (float)(p / (gamma * s * 2));
                } else {
                    c = (float)std::sqrt((gamma + beta) / (gamma * 2));
                    s = (float)(p / (gamma * c * 2));
                }
                a = b = 0;
                for (int k = 0; k < m; k++) {
                    float t0 = c * Ai[k] + s * Aj[k];
                    float t1 = -s * Ai[k] + c * Aj[k];
                    Ai[k] = t0; Aj[k] = t1;
                    a += (double)t0 * t0; b += (double)t1 * t1;
                }
                W[i] = a; W[j] = b;
                changed = true;
                if (Vt) {
                    float *Vi = Vt + i * n, *Vj = Vt + j * n;
                    for (int k = 0; k < n; k++) {
                        float t0 = c * Vi[k] + s * Vj[k];
                        float t1 = -s * Vi[k] + c * Vj[k];
                        Vi[k] = t0; Vj[k] = t1;
                    }
                }
            }
        if (!changed) break;
    }
    for (int i = 0; i < n; i++) {
        double sd = 0;
        for (int k = 0; k < m; k++) { const float t = At[i * m + k]; sd += (double)t * t; }
        W[i] = std::sqrt(sd);
    }
    for (int i = 0; i < n - 1; i++) {
        int j = i;
        for (int k = i + 1; k < n; k++)
            if (W[j] < W[k]) j = k;
        if (i != j) {
            std::swap(W[i], W[j]);
            if (Vt) {
                for (int k = 0; k < m; k++) std::swap(At[i * m + k], At[j * m + k]);
                for (int k = 0; k < n; k++) std::swap(Vt[i * n + k], Vt[j * n + k]);
            }
        }
    }
    for (int i = 0; i < n; i++) Wout[i] = (float)W[i];
    if (!Vt) return;
    Rng rng(0x12345678);
    for (int i = 0; i < n1; i++) {
        double sd = i < n ? W[i] : 0;
        for (int ii = 0; ii < 100 && sd <= minval; ii++) {
            const float val0 = (float)(1. / m);
            for (int k = 0; k < m; k++) At[i * m + k] = (rng.next() & 256) != 0 ? val0 : -val0;
            for (int iter = 0; iter < 2; iter++)
                for (int j = 0; j < i; j++) {
                    sd = 0;
                    for (int k = 0; k < m; k++) sd += At[i * m + k] * At[j * m + k];
                    float asum = 0;
                    for (int k = 0; k < m; k++) {
                        float t = (float)(At[i * m + k] - sd * At[j * m + k]);
                        At[i * m + k] = t;
                        asum += std::abs(t);
                    }
                    asum = asum > eps * 100 ? 1 / asum : 0;
                    for (int k = 0; k < m; k++) At[i * m + k] *= asum;
                }
            sd = 0;
            for (int k = 0; k < m; k++) { const float t = At[i * m + k]; sd += (double)t * t; }
            sd = std::sqrt(sd);
        }
        const float s = (float)(sd > minval ? 1 / sd : 0.);
        for (int k = 0; k < m; k++) At[i * m + k] *= s;
    }
}

// SVDecomp(A (rows x cols), w, u, vt, FULL_UV): u rows x rows, vt cols x cols, w min(rows, cols)
void svdecomp(const float* A, int rows, int cols, float* w, float* u, float* vt)
{
    int m = rows, n = cols;
    const bool at = m < n;
    if (at) std::swap(m, n);
    const int urows = m;   // FULL_UV
    std::vector<float> buf((size_t)urows * m, 0.f), V((size_t)n * n);
    for (int r = 0; r < rows; r++)
        for (int c = 0; c < cols; c++) {
            if (!at) buf[(size_t)c * m + r] = A[r * cols + c];   // transpose(src, temp_a)
            else buf[(size_t)r * m + c] = A[r * cols + c];
        }
    jacobi_svd(buf.data(), m, n, urows, w, V.data());
    // temp_u = buf (urows x m), temp_v = V (n x n)
    if (!at) {
        if (u) for (int r = 0; r < m; r++) for (int c = 0; c < urows; c++) u[r * urows + c] = buf[(size_t)c * m + r];
        if (vt) std::memcpy(vt, V.data(), sizeof(float) * n * n);
    } else {
        if (u) for (int r = 0; r < n; r++) for (int c = 0; c < n; c++) u[r * n + c] = V[(size_t)c * n + r];
        if (vt) std::memcpy(vt, buf.data(), sizeof(float) * urows * m);
    }
}

// C (r x c) = alpha * A (r x k) * B (k x c)
void gemm(const float* A, const float* B, float* C, int r, int k, int c, double alpha = 1.0)
{
    std::vector<float> R((size_t)r * c);
    for (int i = 0; i < r; i++)
        for (int j = 0; j < c; j++) {
            double s = 0;
            for (int q = 0; q < k; q++) s += (double)A[i * k + q] * B[q * c + j];
            R[(size_t)i * c + j] = (float)(s * alpha);
        }
    std::memcpy(C, R.data(), sizeof(float) * r * c);
}
void mm3(const float* A, const float* B, float* C, double alpha = 1.0) { gemm(A, B, C, 3, 3, 3, alpha); }

double det3(const float* m)
{
    return m[0] * ((double)m[4] * m[8] - (double)m[5] * m[7]) - m[1] * ((double)m[3] * m[8] - (double)m[5] * m[6]) +
           m[2] * ((double)m[3] * m[7] - (double)m[4] * m[6]);
}

void inv3(const float* S, float* D)
{
    double d = det3(S);
    if (d == 0.) { for (int i = 0; i < 9; i++) D[i] = 0; return; }
    d = 1. / d;
    const double t[9] = {((double)S[4] * S[8] - (double)S[5] * S[7]) * d, ((double)S[2] * S[7] - (double)S[1] * S[8]) * d,
                         ((double)S[1] * S[5] - (double)S[2] * S[4]) * d, ((double)S[5] * S[6] - (double)S[3] * S[8]) * d,
                         ((double)S[0] * S[8] - (double)S[2] * S[6]) * d, ((double)S[2] * S[3] - (double)S[0] * S[5]) * d,
                         ((double)S[3] * S[7] - (double)S[4] * S[6]) * d, ((double)S[1] * S[6] - (double)S[0] * S[7]) * d,
                         ((double)S[0] * S[4] - (double)S[1] * S[3]) * d};
    for (int i = 0; i < 9; i++) D[i] = (float)t[i];
}

void transpose3(const float* A, float* B) { for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) B[r * 3 + c] = A[c * 3 + r]; }

double norm3(const float* t) { return std::sqrt((double)t[0] * t[0] + (double)t[1] * t[1] + (double)t[2] * t[2]); }

void div_by(float* v, int n, double s)
{
    const float a = (float)(1. / s);
    for (int i = 0; i < n; i++) v[i] = v[i] * a;
}

// --------------------------------------------------------------------------------- Initializer --
struct Initializer {
    float K[9];
    std::vector<KeyPoint> mvKeys1, mvKeys2;
    std::vector<Match> mvMatches12;
    std::vector<bool> mvbMatched1;
    float mSigma, mSigma2;
    int mMaxIterations;
    std::vector<std::vector<size_t>> mvSets;
    // the intermediate results the tests compare
    float T12[18];
    std::vector<float> pn1, pn2, models, scores, sv;
    int32_t margins[10] = {0};   // inliers of the chosen model (Reconstruct*'s N), motions checked, nGood of each motion

    void Normalize(const std::vector<KeyPoint>& vKeys, std::vector<float>& vNormalizedPoints, float* T)
    {
        float meanX = 0, meanY = 0;
        const int N = vKeys.size();
        vNormalizedPoints.resize(2 * N);
        for (int i = 0; i < N; i++) { meanX += vKeys[i].x; meanY += vKeys[i].y; }
        meanX = meanX / N;
        meanY = meanY / N;
        float meanDevX = 0, meanDevY = 0;
        for (int i = 0; i < N; i++) {
            vNormalizedPoints[2 * i] = vKeys[i].x - meanX;
            vNormalizedPoints[2 * i + 1] = vKeys[i].y - meanY;
            meanDevX += std::fabs(vNormalizedPoints[2 * i]);
            meanDevY += std::fabs(vNormalizedPoints[2 * i + 1]);
        }
        meanDevX = meanDevX / N;
        meanDevY = meanDevY / N;
        float sX = 1.0 / meanDevX, sY = 1.0 / meanDevY;
        for (int i = 0; i < N; i++) {
            vNormalizedPoints[2 * i] = vNormalizedPoints[2 * i] * sX;
            vNormalizedPoints[2 * i + 1] = vNormalizedPoints[2 * i + 1] * sY;
        }
        const float Tm[9] = {sX, 0, -meanX * sX, 0, sY, -meanY * sY, 0, 0, 1};
        std::memcpy(T, Tm, sizeof(Tm));
    }

    // ComputeH21 -> Hn (row-major 3x3); sv: the two smallest singular values
    void ComputeH21(const float* p1, const float* p2, float* Hn, float* svo)
    {
        float A[16 * 9];
        for (int i = 0; i < 8; i++) {
            const float u1 = p1[2 * i], v1 = p1[2 * i + 1], u2 = p2[2 * i], v2 = p2[2 * i + 1];
            const float r0[9] = {0.0, 0.0, 0.0, -u1, -v1, -1, v2 * u1, v2 * v1, v2};
            const float r1[9] = {u1, v1, 1, 0.0, 0.0, 0.0, -u2 * u1, -u2 * v1, -u2};
            std::memcpy(A + (2 * i) * 9, r0, sizeof(r0));
            std::memcpy(A + (2 * i + 1) * 9, r1, sizeof(r1));
        }
        float w[9], vt[81];
        svdecomp(A, 16, 9, w, nullptr, vt);
        std::memcpy(Hn, vt + 8 * 9, 9 * sizeof(float));
        svo[0] = w[7]; svo[1] = w[8];
    }

    void ComputeF21(const float* p1, const float* p2, float* F, float* svo)
    {
        float A[8 * 9];
        for (int i = 0; i < 8; i++) {
            const float u1 = p1[2 * i], v1 = p1[2 * i + 1], u2 = p2[2 * i], v2 = p2[2 * i + 1];
            const float r[9] = {u2 * u1, u2 * v1, u2, v2 * u1, v2 * v1, v2, u1, v1, 1};
            std::memcpy(A + i * 9, r, sizeof(r));
        }
        float w[8], u[64], vt[81];
        svdecomp(A, 8, 9, w, u, vt);
        float Fpre[9], w3[3], u3[9], vt3[9];
        std::memcpy(Fpre, vt + 8 * 9, sizeof(Fpre));
        // the two smallest singular values of the system: w[7], and the ninth -- 0 in exact arithmetic, here the residual |A f|
        // the null vector actually reaches
        double r2 = 0;
        for (int i = 0; i < 8; i++) {
            double d = 0;
            for (int k = 0; k < 9; k++) d += (double)A[i * 9 + k] * Fpre[k];
            r2 += d * d;
        }
        svo[0] = w[7]; svo[1] = (float)std::sqrt(r2);
        svdecomp(Fpre, 3, 3, w3, u3, vt3);
        w3[2] = 0;
        const float dg[9] = {w3[0], 0, 0, 0, w3[1], 0, 0, 0, w3[2]};
        float ud[9];
        mm3(u3, dg, ud);
        mm3(ud, vt3, F);
    }

    float CheckHomography(const float* H21, const float* H12, std::vector<bool>& vbMatchesInliers, float sigma)
    {
        const int N = mvMatches12.size();
        vbMatchesInliers.resize(N);
        float score = 0;
        const float th = 5.991;
        const float invSigmaSquare = 1.0 / (sigma * sigma);
        for (int i = 0; i < N; i++) {
            bool bIn = true;
            const KeyPoint& kp1 = mvKeys1[mvMatches12[i].first];
            const KeyPoint& kp2 = mvKeys2[mvMatches12[i].second];
            const float u1 = kp1.x, v1 = kp1.y, u2 = kp2.x, v2 = kp2.y;
            const float w2in1inv = 1.0 / (H12[6] * u2 + H12[7] * v2 + H12[8]);
            const float u2in1 = (H12[0] * u2 + H12[1] * v2 + H12[2]) * w2in1inv;
            const float v2in1 = (H12[3] * u2 + H12[4] * v2 + H12[5]) * w2in1inv;
            const float squareDist1 = (u1 - u2in1) * (u1 - u2in1) + (v1 - v2in1) * (v1 - v2in1);
            const float chiSquare1 = squareDist1 * invSigmaSquare;
            if (chiSquare1 > th) bIn = false;
            else score += th - chiSquare1;
            const float w1in2inv = 1.0 / (H21[6] * u1 + H21[7] * v1 + H21[8]);
            const float u1in2 = (H21[0] * u1 + H21[1] * v1 + H21[2]) * w1in2inv;
            const float v1in2 = (H21[3] * u1 + H21[4] * v1 + H21[5]) * w1in2inv;
            const float squareDist2 = (u2 - u1in2) * (u2 - u1in2) + (v2 - v1in2) * (v2 - v1in2);
            const float chiSquare2 = squareDist2 * invSigmaSquare;
            if (chiSquare2 > th) bIn = false;
            else score += th - chiSquare2;
            vbMatchesInliers[i] = bIn;
        }
        return score;
    }

    float CheckFundamental(const float* F, std::vector<bool>& vbMatchesInliers, float sigma)
    {
        const int N = mvMatches12.size();
        vbMatchesInliers.resize(N);
        float score = 0;
        const float th = 3.841, thScore = 5.991;
        const float invSigmaSquare = 1.0 / (sigma * sigma);
        for (int i = 0; i < N; i++) {
            bool bIn = true;
            const KeyPoint& kp1 = mvKeys1[mvMatches12[i].first];
            const KeyPoint& kp2 = mvKeys2[mvMatches12[i].second];
            const float u1 = kp1.x, v1 = kp1.y, u2 = kp2.x, v2 = kp2.y;
            const float a2 = F[0] * u1 + F[1] * v1 + F[2];
            const float b2 = F[3] * u1 + F[4] * v1 + F[5];
            const float c2 = F[6] * u1 + F[7] * v1 + F[8];
            const float num2 = a2 * u2 + b2 * v2 + c2;
            const float squareDist1 = num2 * num2 / (a2 * a2 + b2 * b2);
            const float chiSquare1 = squareDist1 * invSigmaSquare;
            if (chiSquare1 > th) bIn = false;
            else score += thScore - chiSquare1;
            const float a1 = F[0] * u2 + F[3] * v2 + F[6];
            const float b1 = F[1] * u2 + F[4] * v2 + F[7];
            const float c1 = F[2] * u2 + F[5] * v2 + F[8];
            const float num1 = a1 * u1 + b1 * v1 + c1;
            const float squareDist2 = num1 * num1 / (a1 * a1 + b1 * b1);
            const float chiSquare2 = squareDist2 * invSigmaSquare;
            if (chiSquare2 > th) bIn = false;
            else score += thScore - chiSquare2;
            vbMatchesInliers[i] = bIn;
        }
        return score;
    }

    void FindHomography(std::vector<bool>& vbMatchesInliers, float& score, float* H21, int& best)
    {
        const int N = mvMatches12.size();
        std::vector<float> vPn1, vPn2;
        float T1[9], T2[9], T2inv[9];
        Normalize(mvKeys1, vPn1, T1);
        Normalize(mvKeys2, vPn2, T2);
        std::memcpy(T12, T1, sizeof(T1)); std::memcpy(T12 + 9, T2, sizeof(T2));
        pn1 = vPn1; pn2 = vPn2;
        inv3(T2, T2inv);
        score = 0.0;
        best = -1;
        vbMatchesInliers = std::vector<bool>(N, false);
        std::vector<bool> vbCurrentInliers(N, false);
        for (int it = 0; it < mMaxIterations; it++) {
            float p1[16], p2[16];
            for (size_t j = 0; j < 8; j++) {
                const int idx = mvSets[it][j];
                p1[2 * j] = vPn1[2 * mvMatches12[idx].first]; p1[2 * j + 1] = vPn1[2 * mvMatches12[idx].first + 1];
                p2[2 * j] = vPn2[2 * mvMatches12[idx].second]; p2[2 * j + 1] = vPn2[2 * mvMatches12[idx].second + 1];
            }
            float Hn[9], H21i[9], H12i[9];
            ComputeH21(p1, p2, Hn, &sv[(size_t)it * 2]);
            mm3(T2inv, Hn, H21i);
            mm3(H21i, T1, H21i);
            inv3(H21i, H12i);
            std::memcpy(&models[(size_t)it * 27], H21i, 36);
            std::memcpy(&models[(size_t)it * 27 + 9], H12i, 36);
            const float currentScore = CheckHomography(H21i, H12i, vbCurrentInliers, mSigma);
            scores[it] = currentScore;
            if (currentScore > score) {
                std::memcpy(H21, H21i, 36);
                vbMatchesInliers = vbCurrentInliers;
                score = currentScore;
                best = it;
            }
        }
    }

    void FindFundamental(std::vector<bool>& vbMatchesInliers, float& score, float* F21, int& best)
    {
        const int N = vbMatchesInliers.size();   // (as the reference: the caller's vector is empty here)
        std::vector<float> vPn1, vPn2;
        float T1[9], T2[9], T2t[9];
        Normalize(mvKeys1, vPn1, T1);
        Normalize(mvKeys2, vPn2, T2);
        transpose3(T2, T2t);
        score = 0.0;
        best = -1;
        vbMatchesInliers = std::vector<bool>(N, false);
        std::vector<bool> vbCurrentInliers(N, false);
        for (int it = 0; it < mMaxIterations; it++) {
            float p1[16], p2[16];
            for (int j = 0; j < 8; j++) {
                const int idx = mvSets[it][j];
                p1[2 * j] = vPn1[2 * mvMatches12[idx].first]; p1[2 * j + 1] = vPn1[2 * mvMatches12[idx].first + 1];
                p2[2 * j] = vPn2[2 * mvMatches12[idx].second]; p2[2 * j + 1] = vPn2[2 * mvMatches12[idx].second + 1];
            }
            float Fn[9], F21i[9];
            ComputeF21(p1, p2, Fn, &sv[(size_t)(mMaxIterations + it) * 2]);
            mm3(T2t, Fn, F21i);
            mm3(F21i, T1, F21i);
            std::memcpy(&models[(size_t)it * 27 + 18], F21i, 36);
            const float currentScore = CheckFundamental(F21i, vbCurrentInliers, mSigma);
            scores[mMaxIterations + it] = currentScore;
            if (currentScore > score) {
                std::memcpy(F21, F21i, 36);
                vbMatchesInliers = vbCurrentInliers;
                score = currentScore;
                best = it;
            }
        }
    }

    void Triangulate(const KeyPoint& kp1, const KeyPoint& kp2, const float* P1, const float* P2, float* x3D)
    {
        float A[16];
        for (int c = 0; c < 4; c++) {
            A[0 * 4 + c] = (float)((double)P1[8 + c] * kp1.x - (double)P1[c]);
            A[1 * 4 + c] = (float)((double)P1[8 + c] * kp1.y - (double)P1[4 + c]);
            A[2 * 4 + c] = (float)((double)P2[8 + c] * kp2.x - (double)P2[c]);
            A[3 * 4 + c] = (float)((double)P2[8 + c] * kp2.y - (double)P2[4 + c]);
        }
        float w[4], vt[16];
        svdecomp(A, 4, 4, w, nullptr, vt);
        x3D[0] = vt[12]; x3D[1] = vt[13]; x3D[2] = vt[14];
        div_by(x3D, 3, vt[15]);
    }

    int CheckRT(const float* R, const float* t, const std::vector<bool>& vbMatchesInliers, float th2, std::vector<float>& vP3D,
                std::vector<bool>& vbGood, float& parallax)
    {
        const float fx = K[0], fy = K[4], cx = K[2], cy = K[5];
        vbGood = std::vector<bool>(mvKeys1.size(), false);
        vP3D.assign(mvKeys1.size() * 3, 0.f);
        std::vector<float> vCosParallax;
        vCosParallax.reserve(mvKeys1.size());
        const float P1[12] = {K[0], K[1], K[2], 0, K[3], K[4], K[5], 0, K[6], K[7], K[8], 0};
        const float Rt[12] = {R[0], R[1], R[2], t[0], R[3], R[4], R[5], t[1], R[6], R[7], R[8], t[2]};
        float P2[12], Rtr[9], O2[3];
        gemm(K, Rt, P2, 3, 3, 4);
        transpose3(R, Rtr);
        gemm(Rtr, t, O2, 3, 3, 1, -1.0);
        int nGood = 0;
        for (size_t i = 0, iend = mvMatches12.size(); i < iend; i++) {
            if (!vbMatchesInliers[i]) continue;
            const KeyPoint& kp1 = mvKeys1[mvMatches12[i].first];
            const KeyPoint& kp2 = mvKeys2[mvMatches12[i].second];
            float p3dC1[3];
            Triangulate(kp1, kp2, P1, P2, p3dC1);
            if (!std::isfinite(p3dC1[0]) || !std::isfinite(p3dC1[1]) || !std::isfinite(p3dC1[2])) {
                vbGood[mvMatches12[i].first] = false;
                continue;
            }
            const float normal2[3] = {p3dC1[0] - O2[0], p3dC1[1] - O2[1], p3dC1[2] - O2[2]};
            const float dist1 = norm3(p3dC1), dist2 = norm3(normal2);
            const double dot = (double)p3dC1[0] * normal2[0] + (double)p3dC1[1] * normal2[1] + (double)p3dC1[2] * normal2[2];
            const float cosParallax = dot / (dist1 * dist2);
            if (p3dC1[2] <= 0 && cosParallax < 0.99998) continue;
            float p3dC2[3];
            for (int r = 0; r < 3; r++)
                p3dC2[r] = (float)((double)R[r * 3] * p3dC1[0] + (double)R[r * 3 + 1] * p3dC1[1] + (double)R[r * 3 + 2] * p3dC1[2] + (double)t[r]);
            if (p3dC2[2] <= 0 && cosParallax < 0.99998) continue;
            float invZ1 = 1.0 / p3dC1[2];
            float im1x = fx * p3dC1[0] * invZ1 + cx, im1y = fy * p3dC1[1] * invZ1 + cy;
            float squareError1 = (im1x - kp1.x) * (im1x - kp1.x) + (im1y - kp1.y) * (im1y - kp1.y);
            if (squareError1 > th2) continue;
            float invZ2 = 1.0 / p3dC2[2];
            float im2x = fx * p3dC2[0] * invZ2 + cx, im2y = fy * p3dC2[1] * invZ2 + cy;
            float squareError2 = (im2x - kp2.x) * (im2x - kp2.x) + (im2y - kp2.y) * (im2y - kp2.y);
            if (squareError2 > th2) continue;
            vCosParallax.push_back(cosParallax);
            const int i1 = mvMatches12[i].first;
            vP3D[3 * i1] = p3dC1[0]; vP3D[3 * i1 + 1] = p3dC1[1]; vP3D[3 * i1 + 2] = p3dC1[2];
            nGood++;
            if (cosParallax < 0.99998) vbGood[i1] = true;
        }
        if (nGood > 0) {
            std::sort(vCosParallax.begin(), vCosParallax.end());
            size_t idx = std::min(50, int(vCosParallax.size() - 1));
            parallax = std::acos(vCosParallax[idx]) * 180 / M_PI;
        } else
            parallax = 0;
        return nGood;
    }

    void DecomposeE(const float* E, float* R1, float* R2, float* t)
    {
        float w[3], u[9], vt[9];
        svdecomp(E, 3, 3, w, u, vt);
        t[0] = u[2]; t[1] = u[5]; t[2] = u[8];
        div_by(t, 3, norm3(t));
        const float W[9] = {0, -1, 0, 1, 0, 0, 0, 0, 1};
        float Wt[9];
        transpose3(W, Wt);
        mm3(u, W, R1); mm3(R1, vt, R1);
        if (det3(R1) < 0) for (int i = 0; i < 9; i++) R1[i] = -R1[i];
        mm3(u, Wt, R2); mm3(R2, vt, R2);
        if (det3(R2) < 0) for (int i = 0; i < 9; i++) R2[i] = -R2[i];
    }

    bool ReconstructF(std::vector<bool>& vbMatchesInliers, const float* F21, Result& res, std::vector<float>& vP3D,
                      std::vector<bool>& vbTriangulated, float minParallax, int minTriangulated)
    {
        int N = 0;
        for (size_t i = 0; i < vbMatchesInliers.size(); i++) N += vbMatchesInliers[i];
        float Kt[9], E21[9], R1[9], R2[9], t[3];
        transpose3(K, Kt);
        mm3(Kt, F21, E21);
        mm3(E21, K, E21);
        DecomposeE(E21, R1, R2, t);
        float t1[3] = {t[0], t[1], t[2]}, t2[3] = {-t[0], -t[1], -t[2]};
        std::vector<float> P[4];
        std::vector<bool> G[4];
        float par[4];
        const float* Rs[4] = {R1, R2, R1, R2};
        const float* ts[4] = {t1, t1, t2, t2};
        int nGood[4];
        for (int k = 0; k < 4; k++) nGood[k] = CheckRT(Rs[k], ts[k], vbMatchesInliers, 4.0 * mSigma2, P[k], G[k], par[k]);
        margins[0] = N; margins[1] = 4;
        for (int k = 0; k < 4; k++) margins[2 + k] = nGood[k];
        const int maxGood = std::max(nGood[0], std::max(nGood[1], std::max(nGood[2], nGood[3])));
        const int nMinGood = std::max(static_cast<int>(0.9 * N), minTriangulated);
        int nsimilar = 0;
        for (int k = 0; k < 4; k++) nsimilar += nGood[k] > 0.7 * maxGood;
        int first = 0;
        while (nGood[first] != maxGood) first++;
        res.n_good = maxGood;
        res.parallax = par[first];
        if (maxGood < nMinGood || nsimilar > 1) return false;
        if (par[first] > minParallax) {
            vP3D = P[first];
            vbTriangulated = G[first];
            std::memcpy(res.R21, Rs[first], 36);
            std::memcpy(res.t21, ts[first], 12);
            return true;
        }
        return false;
    }

    bool ReconstructH(std::vector<bool>& vbMatchesInliers, const float* H21, Result& res, std::vector<float>& vP3D,
                      std::vector<bool>& vbTriangulated, float minParallax, int minTriangulated)
    {
        int N = 0;
        for (size_t i = 0; i < vbMatchesInliers.size(); i++) N += vbMatchesInliers[i];
        float invK[9], A[9], U[9], w[3], Vt[9];
        inv3(K, invK);
        mm3(invK, H21, A);
        mm3(A, K, A);
        svdecomp(A, 3, 3, w, U, Vt);
        float s = det3(U) * det3(Vt);
        float d1 = w[0], d2 = w[1], d3 = w[2];
        if (d1 / d2 < 1.00001 || d2 / d3 < 1.00001) return false;
        std::vector<float> vR(8 * 9), vt(8 * 3);
        float aux1 = std::sqrt((d1 * d1 - d2 * d2) / (d1 * d1 - d3 * d3));
        float aux3 = std::sqrt((d2 * d2 - d3 * d3) / (d1 * d1 - d3 * d3));
        float x1[] = {aux1, aux1, -aux1, -aux1};
        float x3[] = {aux3, -aux3, aux3, -aux3};
        float aux_stheta = std::sqrt((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 + d3) * d2);
        float ctheta = (d2 * d2 + d1 * d3) / ((d1 + d3) * d2);
        float stheta[] = {aux_stheta, -aux_stheta, -aux_stheta, aux_stheta};
        for (int i = 0; i < 4; i++) {
            float Rp[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
            Rp[0] = ctheta; Rp[2] = -stheta[i]; Rp[6] = stheta[i]; Rp[8] = ctheta;
            float UR[9];
            mm3(U, Rp, UR, s);
            mm3(UR, Vt, &vR[i * 9]);
            float tp[3] = {x1[i], 0, -x3[i]};
            for (int k = 0; k < 3; k++) tp[k] = tp[k] * (d1 - d3);
            float t[3];
            gemm(U, tp, t, 3, 3, 1);
            div_by(t, 3, norm3(t));
            std::memcpy(&vt[i * 3], t, 12);
        }
        float aux_sphi = std::sqrt((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 - d3) * d2);
        float cphi = (d1 * d3 - d2 * d2) / ((d1 - d3) * d2);
        float sphi[] = {aux_sphi, -aux_sphi, -aux_sphi, aux_sphi};
        for (int i = 0; i < 4; i++) {
            float Rp[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
            Rp[0] = cphi; Rp[2] = sphi[i]; Rp[4] = -1; Rp[6] = sphi[i]; Rp[8] = -cphi;
            float UR[9];
            mm3(U, Rp, UR, s);
            mm3(UR, Vt, &vR[(4 + i) * 9]);
            float tp[3] = {x1[i], 0, x3[i]};
            for (int k = 0; k < 3; k++) tp[k] = tp[k] * (d1 + d3);
            float t[3];
            gemm(U, tp, t, 3, 3, 1);
            div_by(t, 3, norm3(t));
            std::memcpy(&vt[(4 + i) * 3], t, 12);
        }
        int bestGood = 0, secondBestGood = 0, bestSolutionIdx = -1;
        float bestParallax = -1;
        std::vector<float> bestP3D;
        std::vector<bool> bestTriangulated;
        for (size_t i = 0; i < 8; i++) {
            float parallaxi;
            std::vector<float> vP3Di;
            std::vector<bool> vbTriangulatedi;
            int nGood = CheckRT(&vR[i * 9], &vt[i * 3], vbMatchesInliers, 4.0 * mSigma2, vP3Di, vbTriangulatedi, parallaxi);
            margins[0] = N; margins[1] = 8; margins[2 + i] = nGood;
            if (nGood > bestGood) {
                secondBestGood = bestGood;
                bestGood = nGood;
                bestSolutionIdx = i;
                bestParallax = parallaxi;
                bestP3D = vP3Di;
                bestTriangulated = vbTriangulatedi;
            } else if (nGood > secondBestGood) {
                secondBestGood = nGood;
            }
        }
        res.n_good = bestGood;
        res.parallax = bestSolutionIdx >= 0 ? bestParallax : 0.f;
        if (secondBestGood < 0.75 * bestGood && bestParallax >= minParallax && bestGood > minTriangulated && bestGood > 0.9 * N) {
            std::memcpy(res.R21, &vR[bestSolutionIdx * 9], 36);
            std::memcpy(res.t21, &vt[bestSolutionIdx * 3], 12);
            vP3D = bestP3D;
            vbTriangulated = bestTriangulated;
            return true;
        }
        return false;
    }

    void set_matches(const int32_t* m12, int n1)
    {
        mvMatches12.clear();
        mvbMatched1.resize(mvKeys1.size());
        for (int i = 0; i < n1; i++) {
            if (m12[i] >= 0) { mvMatches12.push_back(Match(i, m12[i])); mvbMatched1[i] = true; }
            else mvbMatched1[i] = false;
        }
    }
};

void decode_sets(int N, int iters, const int32_t* words, std::vector<std::vector<size_t>>& sets)
{
    std::vector<size_t> vAllIndices, vAvailableIndices;
    for (int i = 0; i < N; i++) vAllIndices.push_back(i);
    sets = std::vector<std::vector<size_t>>(iters, std::vector<size_t>(8, 0));
    for (int it = 0; it < iters; it++) {
        vAvailableIndices = vAllIndices;
        for (size_t j = 0; j < 8; j++) {
            const int d = (int)vAvailableIndices.size() - 1 - 0 + 1;   // RandomInt(0, size - 1)
            const int randi = int(((double)words[it * 8 + j] / ((double)2147483647 + 1.0)) * d) + 0;
            const int idx = vAvailableIndices[randi];
            sets[it][j] = idx;
            vAvailableIndices[randi] = vAvailableIndices.back();
            vAvailableIndices.pop_back();
        }
    }
}

} // namespace

extern "C" {

// jacobi_svd on its own (tests/solver_units_build.py): At n1 x m in / out, W n, Vt n x n
void ref_jacobi_svd(float* At, int m, int n, int n1, float* W, float* Vt) { jacobi_svd(At, m, n, n1, W, Vt); }

// Initializer(frame1, sigma, iterations).Initialize(frame2, matches12, ...) with the sets drawn from `words`.  Outputs as
// orbfe_initialize; debug outputs (any may be NULL): sets iters x 8, T12 18, pn1 n1 x 2, pn2 n2 x 2, models iters x 27, scores
// 2 x iters, sv 2 x iters x 2 (the two smallest singular values of each eight-point system), margins 10 (inliers of the chosen model,
// motions checked, nGood of each).  Returns N (the match count).
int ref_initialize(const KeyPoint* kps1, int n1, const KeyPoint* kps2, int n2, const int32_t* m12, const float* K4, float sigma, int iters,
                   const int32_t* words, Result* res, float* p3d, uint8_t* tri, int32_t* sets_out, float* T12, float* pn1, float* pn2,
                   float* models, float* scores, float* sv, int32_t* margins)
{
    Initializer I;
    const float K[9] = {K4[0], 0, K4[2], 0, K4[1], K4[3], 0, 0, 1};
    std::memcpy(I.K, K, sizeof(K));
    I.mvKeys1.assign(kps1, kps1 + n1);
    I.mvKeys2.assign(kps2, kps2 + n2);
    I.mSigma = sigma;
    I.mSigma2 = sigma * sigma;
    I.mMaxIterations = iters;
    I.set_matches(m12, n1);
    const int N = I.mvMatches12.size();
    std::memset(res, 0, sizeof(*res));
    res->best_h = res->best_f = -1;
    if (N < 8) return N;   // (the library's documented deviation: RandomInt(0, -1) in the reference)
    decode_sets(N, iters, words, I.mvSets);
    I.models.assign((size_t)iters * 27, 0.f);
    I.scores.assign((size_t)iters * 2, 0.f);
    I.sv.assign((size_t)iters * 4, 0.f);
    std::vector<bool> vbMatchesInliersH, vbMatchesInliersF;
    float SH, SF, H[9] = {0}, F[9] = {0};
    int bh, bf;
    I.FindHomography(vbMatchesInliersH, SH, H, bh);
    I.FindFundamental(vbMatchesInliersF, SF, F, bf);
    const float RH = SH / (SH + SF);
    res->SH = SH; res->SF = SF; res->RH = RH;
    res->best_h = bh; res->best_f = bf;
    std::memcpy(res->H21, H, 36);
    std::memcpy(res->F21, F, 36);
    res->model = RH > 0.40 ? 0 : 1;
    std::vector<float> vP3D;
    std::vector<bool> vbTri;
    bool ok = false;
    if (RH > 0.40) ok = I.ReconstructH(vbMatchesInliersH, H, *res, vP3D, vbTri, 1.0, 50);
    else if (bf >= 0) ok = I.ReconstructF(vbMatchesInliersF, F, *res, vP3D, vbTri, 1.0, 50);
    res->initialized = ok;
    if (ok) {
        for (int i = 0; i < n1; i++) {
            if (p3d) for (int k = 0; k < 3; k++) p3d[3 * i + k] = vP3D[3 * i + k];
            if (tri) tri[i] = vbTri[i];
        }
    }
    if (sets_out) for (int it = 0; it < iters; it++) for (int j = 0; j < 8; j++) sets_out[it * 8 + j] = (int32_t)I.mvSets[it][j];
    if (T12) std::memcpy(T12, I.T12, sizeof(I.T12));
    if (pn1) std::memcpy(pn1, I.pn1.data(), sizeof(float) * 2 * n1);
    if (pn2) std::memcpy(pn2, I.pn2.data(), sizeof(float) * 2 * n2);
    if (models) std::memcpy(models, I.models.data(), sizeof(float) * I.models.size());
    if (scores) std::memcpy(scores, I.scores.data(), sizeof(float) * I.scores.size());
    if (sv) std::memcpy(sv, I.sv.data(), sizeof(float) * I.sv.size());
    if (margins) std::memcpy(margins, I.margins, sizeof(I.margins));
    return N;
}

// InitializeUseAruco: poses npose x 12 (R row-major, t).  res->best_h = bestIdA (-1 = none); returns the bool
int ref_initialize_use_aruco(const KeyPoint* kps1, int n1, const KeyPoint* kps2, int n2, const int32_t* m12, const float* K4, float sigma,
                             const float* poses, int npose, Result* res, float* p3d, uint8_t* tri, int32_t* ngood_out, float* parallax_out)
{
    std::memset(res, 0, sizeof(*res));
    res->model = 2;
    res->best_h = res->best_f = -1;
    if (npose == 0) return 0;
    Initializer I;
    const float K[9] = {K4[0], 0, K4[2], 0, K4[1], K4[3], 0, 0, 1};
    std::memcpy(I.K, K, sizeof(K));
    I.mvKeys1.assign(kps1, kps1 + n1);
    I.mvKeys2.assign(kps2, kps2 + n2);
    I.mSigma = sigma;
    I.mSigma2 = sigma * sigma;
    I.set_matches(m12, n1);
    const int N = I.mvMatches12.size();
    int bestGood = 0;
    std::vector<bool> vbMatchesInliers(N, true);
    for (int i = 0; i < npose; i++) {
        float parallaxi;
        std::vector<float> vP3Di;
        std::vector<bool> vbTriangulatedi;
        int nGood = I.CheckRT(poses + i * 12, poses + i * 12 + 9, vbMatchesInliers, 4.0 * I.mSigma2, vP3Di, vbTriangulatedi, parallaxi);
        if (ngood_out) ngood_out[i] = nGood;
        if (parallax_out) parallax_out[i] = parallaxi;
        if (nGood > bestGood) {
            bestGood = nGood;
            res->best_h = i;
            res->n_good = nGood;
            res->parallax = parallaxi;
            for (int k = 0; k < n1; k++) {
                if (p3d) for (int q = 0; q < 3; q++) p3d[3 * k + q] = vP3Di[3 * k + q];
                if (tri) tri[k] = vbTriangulatedi[k];
            }
        }
    }
    res->initialized = !(bestGood < 0.7 * N);
    if (res->initialized && res->best_h >= 0) {
        std::memcpy(res->R21, poses + res->best_h * 12, 36);
        std::memcpy(res->t21, poses + res->best_h * 12 + 9, 12);
    }
    return res->initialized;
}

void ref_decode_sets(int N, int iters, const int32_t* words, int32_t* out)
{
    std::vector<std::vector<size_t>> sets;
    decode_sets(N, iters, words, sets);
    for (int it = 0; it < iters; it++) for (int j = 0; j < 8; j++) out[it * 8 + j] = (int32_t)sets[it][j];
}

}
