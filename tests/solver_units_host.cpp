// solver_units_host.cpp -- test infrastructure: the SE3Quat pieces of tests/g2o_ref.hpp (the CPU restatement, glibc's libm) behind the
// array calls tests/solver_units_probe.hip gives the device's, for tests/solver_units_build.py.  An SE3 is 7 doubles: q (x y z w), t.
#include "g2o_ref.hpp"

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

} // extern "C"
