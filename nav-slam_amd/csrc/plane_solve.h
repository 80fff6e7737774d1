// plane_solve.h — the two solvers of the point-to-plane registration: the
// eigen-decomposition of a symmetric 3x3 matrix (sym3_eig, surface normals
// from a neighbourhood's covariance) and the linearised point-to-plane step
// (plane_solve). Plain C++ for host and device alike, in the manner of
// align_solve.h: no HIP headers, only + - * / sqrt in f64, no contraction and
// nothing but fixed-size local storage, so that the device (k_normals in
// plane.hip, k_reg_solve in reg_step.h) and a host build
// (tests/plane_solve_driver.cpp) give the same bits. Not part of the
// reference. DESIGN.md §11.
#pragma once

#include "align_solve.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace nv {

constexpr int kEig3Sweeps = 30;
// A pivot of the unit-diagonal system at or below this refuses the step: a
// well-posed scene's pivots are of order 1 (the room scene: all >= 0.97), a
// set of parallel normals gives exact zeros or rounding-level ones.
constexpr double kPlanePivotMin = 1e-10;
// lambda1 <= kPlaneLineTol * lambda2: the neighbours are coincident or
// collinear and define no plane (three orders above Jacobi's eigenvalue
// noise of about eps * lambda2)
constexpr double kPlaneLineTol = 1e-12;

// One Jacobi rotation of the symmetric 3x3 matrix in the plane (p,q), r the
// third axis: app, aqq, apq the pivot block, arp, arq the other two entries;
// (v0p, v0q), ... the matching columns of the eigenvector matrix.
NV_HD inline void eig3_rotate(double &app, double &aqq, double &apq, double &arp, double &arq,
                              double &v0p, double &v0q, double &v1p, double &v1q, double &v2p,
                              double &v2q) {
  if (apq == 0.0) return;
  double t, c, s;
  jacobi_angle(app, aqq, apq, t, c, s);
  app = app - t * apq;
  aqq = aqq + t * apq;
  apq = 0.0;
  const double rp = arp, rq = arq;
  arp = c * rp - s * rq;
  arq = s * rp + c * rq;
  const double a0 = v0p, b0 = v0q, a1 = v1p, b1 = v1q, a2 = v2p, b2 = v2q;
  v0p = c * a0 - s * b0;
  v0q = s * a0 + c * b0;
  v1p = c * a1 - s * b1;
  v1q = s * a1 + c * b1;
  v2p = c * a2 - s * b2;
  v2q = s * a2 + c * b2;
}

// order (la, column a) before (lb, column b) when la > lb
NV_HD inline void eig3_order(double &la, double &lb, double &a0, double &a1, double &a2,
                             double &b0, double &b1, double &b2) {
  if (la > lb) {
    double t = la; la = lb; lb = t;
    t = a0; a0 = b0; b0 = t;
    t = a1; a1 = b1; b1 = t;
    t = a2; a2 = b2; b2 = t;
  }
}

// Eigen-decomposition of the symmetric matrix
//   [ c[0] c[1] c[2] ]
//   [ c[1] c[3] c[4] ]
//   [ c[2] c[4] c[5] ]
// by cyclic Jacobi, rotations (0,1), (0,2), (1,2) per sweep until the
// off-diagonal norm is <= eps * |C|_F (or kEig3Sweeps sweeps). lam: the
// eigenvalues ascending; vec[3 k .. 3 k + 2]: the unit eigenvector of lam[k].
// A diagonal input takes no rotation: its entries come back as they are.
// Every value lives in a named scalar, so a device build keeps them in
// registers.
NV_HD inline void sym3_eig(const double c[6], double lam[3], double vec[9]) {
  double a00 = c[0], a01 = c[1], a02 = c[2], a11 = c[3], a12 = c[4], a22 = c[5];
  double v00 = 1.0, v01 = 0.0, v02 = 0.0;  // vrk: component r of column k
  double v10 = 0.0, v11 = 1.0, v12 = 0.0;
  double v20 = 0.0, v21 = 0.0, v22 = 1.0;
  for (int sweep = 0; sweep < kEig3Sweeps; ++sweep) {
    const double off = 2.0 * ((a01 * a01 + a02 * a02) + a12 * a12);
    const double all = ((a00 * a00 + a11 * a11) + a22 * a22) + off;
    if (nv_sqrt(off) <= kAlignEps * nv_sqrt(all)) break;
    eig3_rotate(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21);
    eig3_rotate(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22);
    eig3_rotate(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22);
  }
  eig3_order(a00, a11, v00, v10, v20, v01, v11, v21);
  eig3_order(a11, a22, v01, v11, v21, v02, v12, v22);
  eig3_order(a00, a11, v00, v10, v20, v01, v11, v21);
  lam[0] = a00;
  lam[1] = a11;
  lam[2] = a22;
  vec[0] = v00; vec[1] = v10; vec[2] = v20;
  vec[3] = v01; vec[4] = v11; vec[5] = v21;
  vec[6] = v02; vec[7] = v12; vec[8] = v22;
}

// Reduced moments of the accepted pairs (p from the source, q its nearest
// target point, n that point's unit normal), with x = p - pbar, r = (q - p).n
// and the row J = [x cross n, n]:
//   m[0]       the number of pairs
//   m[1..3]    pbar = sum p / count
//   m[4]       indices outside [-1, nt) met by the gate (reported, not used)
//   m[5..25]   A = sum J^T J, its 21 upper entries row by row
//   m[26..31]  b = sum J^T r
//   m[32]      sum r^2
constexpr int kPlaneMoments = 33;

// The linearised point-to-plane step: x = (omega, tau) minimising
// sum (r - J x)^2 about the centroid pbar. A is scaled to unit diagonal,
// S = D^-1/2 A D^-1/2, and factored as L diag(d) L^T without pivoting. The
// rotation is the Cayley form of omega, the unit quaternion of (1, omega / 2):
// a proper rotation for every omega, equal to exp(omega) to second order, and
// free of transcendentals. t = tau + pbar - R pbar.
// delta = R (row-major) then t. stats = pairs, rms r before, the linear
// model's rms after sqrt(max(0, sum r^2 - b.x) / n), bad indices, 1 if solved
// (0 if refused), the smallest pivot of S (0 when refused before the
// factorisation). Refused (delta the identity, rms after = rms before) with
// fewer than 6 pairs, a diagonal entry of A <= 0 or a pivot <= kPlanePivotMin.
NV_HD inline void plane_solve(const double m[kPlaneMoments], double delta[12], double stats[6]) {
  const double n = m[0];
  step_begin(n, m[32], m[4], delta, stats);
  stats[4] = 0.0;
  stats[5] = 0.0;
  if (!(n >= 6.0)) return;

  double S[6][6], sc[6], bs[6];
  {
    int k = 5;
    for (int i = 0; i < 6; ++i)
      for (int j = i; j < 6; ++j) S[i][j] = S[j][i] = m[k++];
  }
  for (int i = 0; i < 6; ++i) {
    if (!(S[i][i] > 0.0)) return;
    sc[i] = 1.0 / nv_sqrt(S[i][i]);
  }
  for (int i = 0; i < 6; ++i) {
    for (int j = 0; j < 6; ++j) S[i][j] = i == j ? 1.0 : (S[i][j] * sc[i]) * sc[j];
    bs[i] = m[26 + i] * sc[i];
  }
  // S = L diag(d) L^T, L unit lower triangular
  double L[6][6], d[6];
  double pmin = 0.0;
  for (int j = 0; j < 6; ++j) {
    double dj = S[j][j];
    for (int k = 0; k < j; ++k) dj -= (L[j][k] * L[j][k]) * d[k];
    if (j == 0 || dj < pmin || !(dj == dj)) pmin = dj;
    if (!(dj > kPlanePivotMin)) {
      stats[5] = pmin;
      return;
    }
    d[j] = dj;
    for (int i = j + 1; i < 6; ++i) {
      double v = S[i][j];
      for (int k = 0; k < j; ++k) v -= (L[i][k] * L[j][k]) * d[k];
      L[i][j] = v / dj;
    }
  }
  double x[6];
  for (int i = 0; i < 6; ++i) {  // L z = bs
    double v = bs[i];
    for (int k = 0; k < i; ++k) v -= L[i][k] * x[k];
    x[i] = v;
  }
  for (int i = 0; i < 6; ++i) x[i] /= d[i];
  for (int i = 5; i >= 0; --i) {  // L^T y = z / d
    double v = x[i];
    for (int k = i + 1; k < 6; ++k) v -= L[k][i] * x[k];
    x[i] = v;
  }
  for (int i = 0; i < 6; ++i) x[i] *= sc[i];

  double qx = 0.5 * x[0], qy = 0.5 * x[1], qz = 0.5 * x[2];
  const double nrm = nv_sqrt((1.0 + qx * qx) + (qy * qy + qz * qz));
  const double w = 1.0 / nrm;
  qx /= nrm;
  qy /= nrm;
  qz /= nrm;
  double *R = delta;
  quat_to_rot(w, qx, qy, qz, R);
  const double *pb = m + 1;
  for (int i = 0; i < 3; ++i)
    delta[9 + i] = x[3 + i] + (pb[i] - ((R[3 * i] * pb[0] + R[3 * i + 1] * pb[1]) + R[3 * i + 2] * pb[2]));
  double bx = 0.0;
  for (int i = 0; i < 6; ++i) bx += m[26 + i] * x[i];
  const double res = m[32] - bx;
  stats[2] = nv_sqrt((res > 0.0 ? res : 0.0) / n);
  stats[4] = 1.0;
  stats[5] = pmin;
}

}  // namespace nv
