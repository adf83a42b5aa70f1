// The per-point arithmetic of the normal estimation (cloud_normals.hip), in fp64 and in named scalars
// only (no locally indexed array: nothing here may end up in scratch memory): the neighbourhood test,
// the covariance from the moments about the query point, the cyclic Jacobi eigen-solve of the symmetric
// 3 x 3 matrix and the choice of the smallest eigenvalue's vector.  Host and device: tests/cpp/
// normals_solver.cpp runs the same text on the CPU against LAPACK.
#pragma once

#include <cmath>

#if defined(__HIPCC__)
#define MOPT_NORMALS_HD __host__ __device__ __forceinline__
#else
#define MOPT_NORMALS_HD inline
#endif

namespace mopt {
namespace normals {

constexpr int kJacobiSweeps = 6;  // cyclic sweeps over (0,1), (0,2), (1,2): see symmetricEigen3

// d2 as the header defines it: every operation rounded on its own, so that membership is the same on
// the device and in a restatement on the host
MOPT_NORMALS_HD double distance2(double dx, double dy, double dz) {
#pragma clang fp contract(off)
  const double xx = dx * dx, yy = dy * dy, zz = dz * dz;
  const double xy = xx + yy;
  return xy + zz;
}

// Sum over a neighbourhood of d and d d^T, and its size
struct Moments {
  double sx = 0.0, sy = 0.0, sz = 0.0;
  double xx = 0.0, xy = 0.0, xz = 0.0, yy = 0.0, yz = 0.0, zz = 0.0;
  int k = 0;
};

MOPT_NORMALS_HD void accumulate(Moments &m, double dx, double dy, double dz) {
  m.sx += dx, m.sy += dy, m.sz += dz;
  m.xx += dx * dx, m.xy += dx * dy, m.xz += dx * dz;
  m.yy += dy * dy, m.yz += dy * dz, m.zz += dz * dz;
  m.k += 1;
}

// One Jacobi rotation in the (p, q) plane of a symmetric 3 x 3 matrix: app, aqq, apq its entries there,
// arp, arq the entries that couple the third index r to p and q; v?p, v?q the two columns of the
// accumulated eigenvector matrix.  An off-diagonal entry that is exactly 0 needs no rotation (and must
// not get one: with app == aqq too the angle would be 0 / 0).
MOPT_NORMALS_HD void jacobiRotate(double &app, double &aqq, double &apq, double &arp, double &arq,
                                  double &v0p, double &v0q, double &v1p, double &v1q, double &v2p,
                                  double &v2q) {
  if (apq == 0.0) return;
  // t = tan of the rotation angle, the smaller root of t^2 + 2 t theta - 1 = 0; a theta so large that
  // its square overflows gives t = 0 through 1 / inf
  const double theta = (aqq - app) / (2.0 * apq);
  const double root = std::fabs(theta) + std::sqrt(theta * theta + 1.0);
  const double t = (theta < 0.0 ? -1.0 : 1.0) / root;
  const double c = 1.0 / std::sqrt(t * t + 1.0), s = t * c;
  app -= t * apq;
  aqq += t * apq;
  apq = 0.0;
  const double rp = arp, rq = arq;
  arp = c * rp - s * rq;
  arq = s * rp + c * rq;
  const double a0 = v0p, b0 = v0q, a1 = v1p, b1 = v1q, a2 = v2p, b2 = v2q;
  v0p = c * a0 - s * b0, v0q = s * a0 + c * b0;
  v1p = c * a1 - s * b1, v1q = s * a1 + c * b1;
  v2p = c * a2 - s * b2, v2q = s * a2 + c * b2;
}

// Unit normal (unoriented) and curvature l0 / (l0 + l1 + l2) of the neighbourhood with these moments
// (k >= 1).  Cyclic Jacobi, a fixed number of sweeps: the off-diagonal norm falls quadratically once
// it is small, and a 3 x 3 matrix is at fp64's rounding level after four sweeps in every case tried
// (tests/cpp/normals_solver.cpp: graded, clustered and rank-deficient spectra); six leaves a margin.
// Preferred over the closed trigonometric form, which loses the eigenvector where l0 ~ l1.
MOPT_NORMALS_HD void normalFromMoments(const Moments &m, double &nx, double &ny, double &nz,
                                       double &curvature) {
  const double k = double(m.k);
  const double mx = m.sx / k, my = m.sy / k, mz = m.sz / k;
  double a00 = m.xx / k - mx * mx, a01 = m.xy / k - mx * my, a02 = m.xz / k - mx * mz;
  double a11 = m.yy / k - my * my, a12 = m.yz / k - my * mz, a22 = m.zz / k - mz * mz;
  double v00 = 1.0, v01 = 0.0, v02 = 0.0;  // v<row><column>: column j is the vector of a<j><j>
  double v10 = 0.0, v11 = 1.0, v12 = 0.0;
  double v20 = 0.0, v21 = 0.0, v22 = 1.0;
#pragma unroll
  for (int sweep = 0; sweep < kJacobiSweeps; ++sweep) {
    jacobiRotate(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21);
    jacobiRotate(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22);
    jacobiRotate(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22);
  }
  // the smallest eigenvalue's column, by compares (the first of equal ones)
  const bool first = a00 <= a11 && a00 <= a22;
  const bool second = !first && a11 <= a22;
  const double l0 = first ? a00 : second ? a11 : a22;
  double x = first ? v00 : second ? v01 : v02;
  double y = first ? v10 : second ? v11 : v12;
  double z = first ? v20 : second ? v21 : v22;
  const double norm = std::sqrt(x * x + y * y + z * z);  // (1 up to the rotations' rounding)
  nx = x / norm, ny = y / norm, nz = z / norm;
  const double trace = a00 + a11 + a22;
  curvature = trace == 0.0 ? 0.0 : l0 / trace;
}

}  // namespace normals
}  // namespace mopt
