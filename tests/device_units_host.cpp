// device_units_host.cpp -- test infrastructure only: include/orbfe_math.h as g++ compiles it (-ffp-contract=off), behind the array
// calls that tests/device_units_probe.hip offers for the same header on the device.  tests/device_units_build.py loads it with
// ctypes; with -DDEVICE_UNITS_MAIN it is a program of its own that runs every call over a small input, for the sanitizers.
#include <cmath>
#include <cstdio>
#include <vector>

#include "../include/orbfe_math.h"

extern "C" {

int du_atan2(const float* y, const float* x, float* out, int n)
{
    for (int i = 0; i < n; i++) out[i] = orbfe_fast_atan2(y[i], x[i]);
    return 0;
}

int du_sincos(const float* a, float* s, float* c, int n)
{
    for (int i = 0; i < n; i++) orbfe_sincosf(a[i], &s[i], &c[i]);
    return 0;
}

int du_round(const double* v, const float* vf, int* rd, int* rf, int* fl, int* ce, int n)
{
    for (int i = 0; i < n; i++) {
        rd[i] = orbfe_round_d(v[i]);
        rf[i] = orbfe_round_f(vf[i]);
        fl[i] = orbfe_floor_d(v[i]);
        ce[i] = orbfe_ceil_d(v[i]);
    }
    return 0;
}

int du_undistort(const float* uv, int n, const double* cam, const double* k12, float* out)
{
    for (int i = 0; i < n; i++) {
        double k[12];
        for (int j = 0; j < 12; j++) k[j] = k12[j];
        orbfe_undistort_point(uv[2 * i], uv[2 * i + 1], cam[0], cam[1], cam[2], cam[3], k, &out[2 * i], &out[2 * i + 1]);
    }
    return 0;
}

} // extern "C"

#ifdef DEVICE_UNITS_MAIN
int main()
{
    // every quadrant, both axes, the origin, a half-way case of every rounding helper, a point outside the frame
    const int n = 41 * 41;
    std::vector<float> y(n), x(n), a(n), s(n), c(n), o(n), uv(2 * n), und(2 * n);
    std::vector<double> v(n);
    std::vector<int> rd(n), rf(n), fl(n), ce(n);
    for (int i = 0; i < n; i++) {
        y[i] = (float)(i / 41 - 20);
        x[i] = (float)(i % 41 - 20);
        a[i] = (float)(i - n / 2) * 5.9f;
        v[i] = (i - n / 2) * 0.5;
        uv[2 * i] = -40.f + 17.5f * (float)(i % 41);
        uv[2 * i + 1] = -40.f + 14.f * (float)(i / 41);
    }
    std::vector<float> vf(v.begin(), v.end());
    const double cam[4] = {517.306408, 516.469215, 318.643040, 255.313989};
    const double k12[12] = {0.262383, -0.953104, -0.005358, 0.002628, 1.163314, 0.01, -0.02, 0.005, 1e-3, -5e-4, 2e-4, -1e-4};
    du_atan2(y.data(), x.data(), o.data(), n);
    du_sincos(a.data(), s.data(), c.data(), n);
    du_round(v.data(), vf.data(), rd.data(), rf.data(), fl.data(), ce.data(), n);
    du_undistort(uv.data(), n, cam, k12, und.data());
    int bad = 0;
    for (int i = 0; i < n; i++) {
        bad += !(o[i] >= 0.f && o[i] <= 360.f);
        bad += !(std::fabs(s[i] * s[i] + c[i] * c[i] - 1.f) < 1e-6f);
        bad += !(fl[i] <= rd[i] && rd[i] <= ce[i] && ce[i] - fl[i] <= 1 && rf[i] == rd[i]);
        bad += !(std::isfinite(und[2 * i]) && std::isfinite(und[2 * i + 1]));
    }
    std::printf("device_units_host: %d values per call, %d violations\n", n, bad);
    return bad != 0;
}
#endif
