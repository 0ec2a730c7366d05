// TEST INFRASTRUCTURE ONLY -- what include/shims/Optimizer_sim3_orbfe.cc touches of g2o::Sim3 (Thirdparty/g2o/g2o/types/sim3.h) and of
// the Eigen types it is made of: construction from (Quaterniond | Matrix3d, Vector3d, double), rotation(), translation(), scale(),
// Quaterniond's coefficients, its construction from a rotation matrix and toRotationMatrix().  Nothing is normalised, as in g2o.
#ifndef MOCK_G2O_SEVEN_DOF_H
#define MOCK_G2O_SEVEN_DOF_H
#include <cmath>
namespace Eigen {
struct Vector3d {
    double v[3];
    Vector3d() : v{0, 0, 0} {}
    Vector3d(double x, double y, double z) : v{x, y, z} {}
    double& operator[](int i) { return v[i]; }
    const double& operator[](int i) const { return v[i]; }
};
struct Matrix3d {
    double m[3][3];
    double& operator()(int r, int c) { return m[r][c]; }
    const double& operator()(int r, int c) const { return m[r][c]; }
};
class Quaterniond {
    double x_, y_, z_, w_;
public:
    Quaterniond() : x_(0), y_(0), z_(0), w_(1) {}
    Quaterniond(double w, double x, double y, double z) : x_(x), y_(y), z_(z), w_(w) {}
    explicit Quaterniond(const Matrix3d& R)
    {
        double* q[3] = {&x_, &y_, &z_};
        double t = R(0, 0) + R(1, 1) + R(2, 2);
        if (t > 0) {
            t = std::sqrt(t + 1.0);
            w_ = 0.5 * t;
            t = 0.5 / t;
            x_ = (R(2, 1) - R(1, 2)) * t;
            y_ = (R(0, 2) - R(2, 0)) * t;
            z_ = (R(1, 0) - R(0, 1)) * t;
        } else {
            int i = 0;
            if (R(1, 1) > R(0, 0)) i = 1;
            if (R(2, 2) > R(i, i)) i = 2;
            const int j = (i + 1) % 3, k = (j + 1) % 3;
            t = std::sqrt(R(i, i) - R(j, j) - R(k, k) + 1.0);
            *q[i] = 0.5 * t;
            t = 0.5 / t;
            w_ = (R(k, j) - R(j, k)) * t;
            *q[j] = (R(j, i) + R(i, j)) * t;
            *q[k] = (R(k, i) + R(i, k)) * t;
        }
    }
    double x() const { return x_; }
    double y() const { return y_; }
    double z() const { return z_; }
    double w() const { return w_; }
    Matrix3d toRotationMatrix() const
    {
        const double tx = 2 * x_, ty = 2 * y_, tz = 2 * z_;
        const double twx = tx * w_, twy = ty * w_, twz = tz * w_;
        const double txx = tx * x_, txy = ty * x_, txz = tz * x_;
        const double tyy = ty * y_, tyz = tz * y_, tzz = tz * z_;
        Matrix3d R;
        R(0, 0) = 1 - (tyy + tzz); R(0, 1) = txy - twz; R(0, 2) = txz + twy;
        R(1, 0) = txy + twz; R(1, 1) = 1 - (txx + tzz); R(1, 2) = tyz - twx;
        R(2, 0) = txz - twy; R(2, 1) = tyz + twx; R(2, 2) = 1 - (txx + tyy);
        return R;
    }
};
}
namespace g2o {
class Sim3 {
    Eigen::Quaterniond r;
    Eigen::Vector3d t;
    double s;
public:
    Sim3() : s(1.) {}
    Sim3(const Eigen::Quaterniond& r_, const Eigen::Vector3d& t_, double s_) : r(r_), t(t_), s(s_) {}
    Sim3(const Eigen::Matrix3d& R, const Eigen::Vector3d& t_, double s_) : r(Eigen::Quaterniond(R)), t(t_), s(s_) {}
    const Eigen::Quaterniond& rotation() const { return r; }
    const Eigen::Vector3d& translation() const { return t; }
    const double& scale() const { return s; }
};
}
#endif
