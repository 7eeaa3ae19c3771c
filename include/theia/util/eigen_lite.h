// Tiny fixed-size vectors with the handful of Eigen accessors the BA boundary
// uses (x(), y(), operator[], data(), head<3>() is not needed).  The reference's
// data model stores Eigen::Vector2d / Vector4d (feature.h, track.h:84-88); this
// Eigen-free shim keeps the same spelling so host code ports verbatim.
#ifndef THEIA_MI355_EIGEN_LITE_H_
#define THEIA_MI355_EIGEN_LITE_H_
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>
namespace Eigen {
template <typename T, int N>
struct LiteVector {
  T v[N];
  LiteVector() { for (int i = 0; i < N; ++i) v[i] = T(0); }
  LiteVector(T a, T b) { static_assert(N == 2, "size"); v[0] = a; v[1] = b; }
  LiteVector(T a, T b, T c) { static_assert(N == 3, "size"); v[0] = a; v[1] = b; v[2] = c; }
  LiteVector(T a, T b, T c, T d) { static_assert(N == 4, "size"); v[0] = a; v[1] = b; v[2] = c; v[3] = d; }
  T& operator[](int i) { return v[i]; }
  const T& operator[](int i) const { return v[i]; }
  T& operator()(int i) { return v[i]; }
  const T& operator()(int i) const { return v[i]; }
  T& x() { return v[0]; }
  T& y() { return v[1]; }
  const T& x() const { return v[0]; }
  const T& y() const { return v[1]; }
  T* data() { return v; }
  const T* data() const { return v; }
  static constexpr int size() { return N; }
  static LiteVector Zero() { return LiteVector(); }
};
// The smallest dynamic float vector the descriptor interface needs (keypoints_and_descriptors.h stores
// std::vector<Eigen::VectorXf>): size, element access, data, Constant / Zero, squaredNorm / norm and normalize.
class LiteVectorXf {
 public:
  LiteVectorXf() {}
  explicit LiteVectorXf(int n) : v_(static_cast<size_t>(n), 0.f) {}
  static LiteVectorXf Constant(int n, float value) {
    LiteVectorXf r(n);
    for (float& x : r.v_) x = value;
    return r;
  }
  static LiteVectorXf Zero(int n) { return LiteVectorXf(n); }
  int size() const { return static_cast<int>(v_.size()); }
  void resize(int n) { v_.resize(static_cast<size_t>(n)); }
  float& operator[](int i) { return v_[static_cast<size_t>(i)]; }
  const float& operator[](int i) const { return v_[static_cast<size_t>(i)]; }
  float& operator()(int i) { return v_[static_cast<size_t>(i)]; }
  const float& operator()(int i) const { return v_[static_cast<size_t>(i)]; }
  float* data() { return v_.data(); }
  const float* data() const { return v_.data(); }
  float squaredNorm() const {
    float s = 0.f;
    for (const float x : v_) s += x * x;
    return s;
  }
  float norm() const { return std::sqrt(squaredNorm()); }
  void normalize() {
    const float n = norm();
    if (n > 0.f)
      for (float& x : v_) x /= n;
  }
  LiteVectorXf normalized() const {
    LiteVectorXf r(*this);
    r.normalize();
    return r;
  }

 private:
  std::vector<float> v_;
};
// A 3x3 double matrix, column-major as Eigen's default, with element access and data().
struct LiteMatrix3d {
  double m[9];
  LiteMatrix3d() { for (int i = 0; i < 9; ++i) m[i] = 0.0; }
  double& operator()(int r, int c) { return m[r + 3 * c]; }
  const double& operator()(int r, int c) const { return m[r + 3 * c]; }
  double* data() { return m; }
  const double* data() const { return m; }
  static LiteMatrix3d Zero() { return LiteMatrix3d(); }
};
typedef LiteMatrix3d Matrix3d;
typedef LiteVectorXf VectorXf;
typedef LiteVector<double, 2> Vector2d;
typedef LiteVector<double, 3> Vector3d;
typedef LiteVector<double, 4> Vector4d;
}  // namespace Eigen
#endif
