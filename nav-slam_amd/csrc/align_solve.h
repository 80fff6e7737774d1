// align_solve.h — closed-form rigid fit (Horn's unit-quaternion method) from
// the centred moments of a set of point pairs, and pose composition. Plain
// C++ for host and device alike: no HIP headers, no libm beyond sqrt, only
// + - * / sqrt in f64 and no contraction, so that the device (k_reg_solve,
// reg_step.h) and a host build (tests/align_solve_driver.cpp) give the same
// bits. Not part of the reference: its optimiser never fits a rotation
// (src/slam.c:300-389). step_begin, jacobi_angle and quat_to_rot are shared
// with plane_solve.h.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define NV_HD __host__ __device__
#else
#define NV_HD
#endif

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace nv {

// Centred moments of the accepted pairs (p from the source, q its target):
//   m[0]      n, the number of pairs
//   m[1..3]   pbar = sum p / n        m[4..6]  qbar = sum q / n
//   m[7]      sum |q - p|^2
//   m[8..16]  H = sum (p - pbar)(q - qbar)^T, row-major (row: p's axis)
//   m[17]     sum |p - pbar|^2        m[18]    sum |q - qbar|^2
//   m[19]     indices outside [-1, nt) met by the gate (reported, not used)
constexpr int kAlignMoments = 20;
constexpr int kJacobiSweeps = 30;
constexpr double kAlignEps = 0x1p-52;

NV_HD inline double nv_sqrt(double v) { return __builtin_sqrt(v); }
NV_HD inline double nv_abs(double v) { return v < 0.0 ? -v : v; }

// The opening of a step's solver: stats = n, rms before (sqrt(ss / n), twice:
// rms after = rms before until a fit replaces it), bad indices; delta = the
// identity.
NV_HD inline void step_begin(double n, double ss, double bad, double delta[12], double *stats) {
  const double rms0 = n > 0.0 ? nv_sqrt(ss / n) : 0.0;
  stats[0] = n;
  stats[1] = rms0;
  stats[2] = rms0;
  stats[3] = bad;
  for (int i = 0; i < 12; ++i) delta[i] = 0.0;
  delta[0] = delta[4] = delta[8] = 1.0;
}

// The Jacobi rotation that annihilates apq of the symmetric pivot block
// (app, apq; apq, aqq), apq != 0: t = tan, c = cos, s = sin of its angle.
NV_HD inline void jacobi_angle(double app, double aqq, double apq, double &t, double &c,
                               double &s) {
  const double theta = (aqq - app) / (2.0 * apq);
  const double at = nv_abs(theta);
  // for |theta| beyond 2^500 theta^2 + 1 would overflow: t = 1/(2 theta)
  t = at > 0x1p500 ? 0.5 / at : 1.0 / (at + nv_sqrt(theta * theta + 1.0));
  if (theta < 0.0) t = -t;
  c = 1.0 / nv_sqrt(t * t + 1.0);
  s = t * c;
}

// R (row-major) of the unit quaternion (w, x, y, z)
NV_HD inline void quat_to_rot(double w, double x, double y, double z, double R[9]) {
  R[0] = 1.0 - 2.0 * (y * y + z * z);
  R[1] = 2.0 * (x * y - w * z);
  R[2] = 2.0 * (x * z + w * y);
  R[3] = 2.0 * (x * y + w * z);
  R[4] = 1.0 - 2.0 * (x * x + z * z);
  R[5] = 2.0 * (y * z - w * x);
  R[6] = 2.0 * (x * z - w * y);
  R[7] = 2.0 * (y * z + w * x);
  R[8] = 1.0 - 2.0 * (x * x + y * y);
}

// delta = R (row-major) then t, with q ~ R p + t in the least-squares sense;
// stats = n, rms |q - p| before, rms |q - (R p + t)| after, bad indices.
// Fewer than 3 pairs: the identity, and rms after = rms before.
NV_HD inline void align_solve(const double m[kAlignMoments], double delta[12], double stats[4]) {
  const double n = m[0];
  step_begin(n, m[7], m[19], delta, stats);
  if (!(n >= 3.0)) return;

  const double Sxx = m[8], Sxy = m[9], Sxz = m[10];
  const double Syx = m[11], Syy = m[12], Syz = m[13];
  const double Szx = m[14], Szy = m[15], Szz = m[16];
  // Horn (1987) eq. 25: the unit quaternion of the best rotation is the
  // eigenvector of N at its largest eigenvalue
  double A[4][4];
  A[0][0] = (Sxx + Syy) + Szz;
  A[1][1] = (Sxx - Syy) - Szz;
  A[2][2] = (Syy - Sxx) - Szz;
  A[3][3] = (Szz - Sxx) - Syy;
  A[0][1] = A[1][0] = Syz - Szy;
  A[0][2] = A[2][0] = Szx - Sxz;
  A[0][3] = A[3][0] = Sxy - Syx;
  A[1][2] = A[2][1] = Sxy + Syx;
  A[1][3] = A[3][1] = Szx + Sxz;
  A[2][3] = A[3][2] = Syz + Szy;
  double V[4][4];
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 4; ++j) V[i][j] = i == j ? 1.0 : 0.0;

  // cyclic Jacobi: rotations (p,q) in row order until the off-diagonal norm
  // is at rounding level of the whole matrix
  for (int sweep = 0; sweep < kJacobiSweeps; ++sweep) {
    double off = 0.0, all = 0.0;
    for (int i = 0; i < 4; ++i)
      for (int j = 0; j < 4; ++j) {
        const double v = A[i][j] * A[i][j];
        all += v;
        if (i != j) off += v;
      }
    if (nv_sqrt(off) <= kAlignEps * nv_sqrt(all)) break;
    for (int p = 0; p < 3; ++p)
      for (int q = p + 1; q < 4; ++q) {
        const double apq = A[p][q];
        if (apq == 0.0) continue;
        double t, c, s;
        jacobi_angle(A[p][p], A[q][q], apq, t, c, s);
        for (int k = 0; k < 4; ++k) {  // A <- A J
          const double akp = A[k][p], akq = A[k][q];
          A[k][p] = c * akp - s * akq;
          A[k][q] = s * akp + c * akq;
        }
        for (int k = 0; k < 4; ++k) {  // A <- J^T A
          const double apk = A[p][k], aqk = A[q][k];
          A[p][k] = c * apk - s * aqk;
          A[q][k] = s * apk + c * aqk;
        }
        A[p][q] = A[q][p] = 0.0;
        for (int k = 0; k < 4; ++k) {  // V <- V J
          const double vkp = V[k][p], vkq = V[k][q];
          V[k][p] = c * vkp - s * vkq;
          V[k][q] = s * vkp + c * vkq;
        }
      }
  }
  int best = 0;  // largest diagonal entry, lowest index on ties (H = 0: identity)
  for (int i = 1; i < 4; ++i)
    if (A[i][i] > A[best][best]) best = i;
  double w = V[0][best], x = V[1][best], y = V[2][best], z = V[3][best];
  const double nrm = nv_sqrt((w * w + x * x) + (y * y + z * z));
  w /= nrm;
  x /= nrm;
  y /= nrm;
  z /= nrm;
  double *R = delta;
  quat_to_rot(w, x, y, z, R);
  const double *pb = m + 1, *qb = m + 4;
  for (int i = 0; i < 3; ++i)
    delta[9 + i] = qb[i] - ((R[3 * i] * pb[0] + R[3 * i + 1] * pb[1]) + R[3 * i + 2] * pb[2]);
  // sum |(q - qbar) - R (p - pbar)|^2 = Spp + Sqq - 2 sum_ij R_ij H_ji
  double tr = 0.0;
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) tr += R[3 * i + j] * m[8 + 3 * j + i];
  const double res = (m[17] + m[18]) - 2.0 * tr;
  stats[2] = nv_sqrt((res > 0.0 ? res : 0.0) / n);
}

// pose <- delta o pose: R' = dR R, t' = dR t + dt (both 12 doubles, R
// row-major then t), sums left to right
NV_HD inline void pose_compose(const double delta[12], double pose[12]) {
  double o[12];
  for (int i = 0; i < 3; ++i) {
    const double a = delta[3 * i], b = delta[3 * i + 1], c = delta[3 * i + 2];
    for (int j = 0; j < 3; ++j) o[3 * i + j] = (a * pose[j] + b * pose[3 + j]) + c * pose[6 + j];
    o[9 + i] = ((a * pose[9] + b * pose[10]) + c * pose[11]) + delta[9 + i];
  }
  for (int i = 0; i < 12; ++i) pose[i] = o[i];
}

}  // namespace nv
