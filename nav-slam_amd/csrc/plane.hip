// plane.hip — point-to-plane registration on the global k-NN's output:
// surface normals from each point's k-neighbourhood (k_normals) and the
// point-to-plane metric of the shared two-pass step (reg_step.h), whose
// linearised solver is plane_solve.h's. Fourth translation unit of
// libnavgpu.so. Beyond the reference, which has neither normals nor a
// rotation fit; the checkers are the numpy restatements in tests/reg_ref.py.
// DESIGN.md §11.
//
//   k_normals   mu, centred covariance, sym3_eig, orientation
//   pass A      n, sum p, bad indices
//   finish      pbar from the pass-A partials
//   pass B      A (21), b (6), sum r^2 about pbar
//   solve       plane_solve, stats, pose <- delta o pose
//
// The sums follow align.hip's rule (det_reduce.h): reproducible bit for bit,
// no floating-point atomics, a grid that depends on nq alone.
#include "navgpu_common.h"

#include "plane_solve.h"
#include "det_reduce.h"
#include "reg_step.h"

using namespace nv;

namespace {

// ------------------------------------------------------------------ normals
constexpr int kNormBlock = 256;
constexpr int kNormMaxGrid = 1024;  // 4 blocks (16 waves) on each of the 256 CUs

// One point per lane and trip. KMAX is k rounded up to 4, 8 or 16: the slot
// loops are fully unrolled over KMAX and a slot >= k counts as invalid, so
// every neighbour lives in a named register and all KMAX gathers are issued
// before the first is consumed. An index outside [0, n) is replaced by the
// point's own before the gather and never dereferenced. The second launch
// bound asks for four waves per SIMD: at most 128 VGPRs.
template <int KMAX>
__global__ __launch_bounds__(kNormBlock, 4) void k_normals(
    const double *__restrict__ pts, size_t n, const int32_t *__restrict__ idx, int stride, int k,
    bool has_vp, double vx, double vy, double vz, double *__restrict__ normals,
    double *__restrict__ curv) {
  for (size_t i = (size_t)blockIdx.x * kNormBlock + threadIdx.x; i < n;
       i += (size_t)gridDim.x * kNormBlock) {
    int j[KMAX];
    bool ok[KMAX];
#pragma unroll
    for (int s = 0; s < KMAX; ++s) j[s] = s < k ? idx[i * stride + s] : -1;
#pragma unroll
    for (int s = 0; s < KMAX; ++s) {
      ok[s] = (j[s] >= 0) & ((size_t)j[s] < n);
      j[s] = ok[s] ? j[s] : (int)i;
    }
    double x[KMAX][3];
#pragma unroll
    for (int s = 0; s < KMAX; ++s) {
#pragma unroll
      for (int c = 0; c < 3; ++c) x[s][c] = pts[3 * (size_t)j[s] + c];
    }
    double m = 0.0, mu[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int s = 0; s < KMAX; ++s) {
      if (ok[s]) {
        m += 1.0;
#pragma unroll
        for (int c = 0; c < 3; ++c) mu[c] += x[s][c];
      }
    }
    const double dm = m > 0.0 ? m : 1.0;
#pragma unroll
    for (int c = 0; c < 3; ++c) mu[c] /= dm;
    double C[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int s = 0; s < KMAX; ++s) {
      if (ok[s]) {
        const double a = x[s][0] - mu[0], b = x[s][1] - mu[1], c = x[s][2] - mu[2];
        C[0] += a * a;
        C[1] += a * b;
        C[2] += a * c;
        C[3] += b * b;
        C[4] += b * c;
        C[5] += c * c;
      }
    }
    double lam[3], vec[9];
    sym3_eig(C, lam, vec);
    double nx = vec[0], ny = vec[1], nz = vec[2];
    const bool valid = (m >= 3.0) & (lam[2] > 0.0) & (lam[1] > kPlaneLineTol * lam[2]);
    bool flip;
    if (has_vp) {
      // the point itself, read only here: a late load (its line was gathered
      // above whenever it is its own neighbour) and 6 VGPRs fewer at the peak
      const double px = pts[3 * i], py = pts[3 * i + 1], pz = pts[3 * i + 2];
      flip = (nx * (vx - px) + ny * (vy - py)) + nz * (vz - pz) < 0.0;
    } else {
      // the component of largest magnitude, lowest index on ties, is positive
      const double ax = nv_abs(nx), ay = nv_abs(ny), az = nv_abs(nz);
      double big = nx, ab = ax;
      if (ay > ab) {
        big = ny;
        ab = ay;
      }
      if (az > ab) big = nz;
      flip = big < 0.0;
    }
    if (flip) {
      nx = -nx;
      ny = -ny;
      nz = -nz;
    }
    const double tr = (lam[0] + lam[1]) + lam[2];
    normals[3 * i] = valid ? nx : 0.0;
    normals[3 * i + 1] = valid ? ny : 0.0;
    normals[3 * i + 2] = valid ? nz : 0.0;
    if (curv) curv[i] = valid ? (lam[0] > 0.0 ? lam[0] : 0.0) / tr : NAN;
  }
}

int normals_run(navgpu_ctx *ctx, const double *pts, size_t n, const int32_t *idx, int stride,
                int k, const double *viewpoint, double *normals, double *curv) {
  ARG_CHECK(ctx);
  ARG_CHECK(k >= 3 && k <= stride && stride <= 16);
  ARG_CHECK(n < (size_t)INT32_MAX);
  if (!n) return NAVGPU_OK;
  ARG_CHECK(pts && idx && normals);
  const bool has_vp = viewpoint != nullptr;
  const double vx = has_vp ? viewpoint[0] : 0.0, vy = has_vp ? viewpoint[1] : 0.0,
               vz = has_vp ? viewpoint[2] : 0.0;
  const unsigned grid = std::min<unsigned>(kNormMaxGrid, grid1d(n, kNormBlock));
  TimedRegion tr(ctx, "normals");
#define NV_NORMALS(KMAX)                                                                       \
  hipLaunchKernelGGL(k_normals<KMAX>, dim3(grid), dim3(kNormBlock), 0, ctx->stream, pts, n, idx, \
                     stride, k, has_vp, vx, vy, vz, normals, curv)
  if (k <= 4)
    NV_NORMALS(4);
  else if (k <= 8)
    NV_NORMALS(8);
  else
    NV_NORMALS(16);
#undef NV_NORMALS
  CHECK_LAUNCH("k_normals");
  return NAVGPU_OK;
}

// the k-NN of a cloud against itself into the workspace, then its normals
int cloud_normals_run(navgpu_ctx *ctx, const double *pts, size_t n, int k, const double *viewpoint,
                      double *normals, double *curv) {
  ARG_CHECK(ctx);
  ARG_CHECK(k >= 3 && k <= 16);
  ARG_CHECK(n < (size_t)INT32_MAX / 2);  // navgpu_knn_dev's range
  if (!n) return NAVGPU_OK;
  ARG_CHECK(pts && normals);
  int32_t *nni;
  double *nnd;
  RC(ws(ctx, kNormIdx, n * k, &nni));
  RC(ws(ctx, kNormDist, n * k, &nnd));
  RC(navgpu_knn_dev(ctx, pts, n, pts, n, k, nni, nnd));
  return normals_run(ctx, pts, n, nni, k, k, viewpoint, normals, curv);
}

// --------------------------------------------------------------- plane step
struct PlaneIn {
  const double *src, *tgt, *nrm, *curv;  // the target's are never null in a kernel (no_target)
  const int32_t *idx;
  const double *dist;
  const int32_t *mask;  // nullable
  size_t nq;
  int nt, stride;
  double max_dist, max_curv;
  bool has_target() const { return tgt && nrm && curv; }
  bool gates_are_numbers() const { return max_dist == max_dist && max_curv == max_curv; }
  void no_target(const double *p) { tgt = nrm = curv = p; }
};

// The shared gate (reg_step.h) and one more condition, the neighbour's
// curvature <= max_curv: a NaN curvature (no normal there) fails it.
struct PlaneMetric {
  // Independent queries in flight per lane. Pass B keeps 28 f64 accumulators
  // (56 VGPRs) per lane, and a query in flight holds p, q and the normal (18
  // VGPRs) beside its index, distance, mask and curvature: two of them stay
  // within the 128-VGPR budget of four waves per SIMD, four do not.
  static constexpr int kU = 2;
  static constexpr int kNA = 5;    // pass A: n, sum p, bad
  static constexpr int kNB = 28;   // pass B: A upper (21), b (6), sum r^2
  static constexpr int kRow = 32;  // doubles per partial row (256 B)
  static constexpr int kCentroids = 1;  // finish record: n, pbar, bad
  static constexpr int kStats = 6;
  static constexpr int kPart = kPlanePart, kOut = kPlaneOut;
  static constexpr const char *kRegion = "align_plane";
  using In = PlaneIn;
  struct Pair {
    double cv, p[3], t[3], nn[3];  // t and nn in pass B only
  };

  template <int PASS>
  static __device__ __forceinline__ void gather(const In &a, size_t q, int j, Pair &g) {
    g.cv = a.curv[j];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      g.p[c] = a.src[3 * q + c];
      if (PASS) {
        g.t[c] = a.tgt[3 * (size_t)j + c];
        g.nn[c] = a.nrm[3 * (size_t)j + c];
      }
    }
  }

  static __device__ __forceinline__ bool accept(const In &a, const Pair &g) {
    return g.cv <= a.max_curv;
  }

  static __device__ __forceinline__ void add_a(const Pair &g, double (&acc)[kNA]) {
    acc[0] += 1.0;
#pragma unroll
    for (int c = 0; c < 3; ++c) acc[1 + c] += g.p[c];
  }

  // pb = pbar
  static __device__ __forceinline__ void add_b(const Pair &g, const double (&pb)[3],
                                               double (&acc)[kNB]) {
    const double x = g.p[0] - pb[0], y = g.p[1] - pb[1], z = g.p[2] - pb[2];
    const double n0 = g.nn[0], n1 = g.nn[1], n2 = g.nn[2];
    double J[6];
    J[0] = y * n2 - z * n1;
    J[1] = z * n0 - x * n2;
    J[2] = x * n1 - y * n0;
    J[3] = n0;
    J[4] = n1;
    J[5] = n2;
    const double r = ((g.t[0] - g.p[0]) * n0 + (g.t[1] - g.p[1]) * n1) + (g.t[2] - g.p[2]) * n2;
    int e = 0;
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
      for (int k = i; k < 6; ++k) acc[e++] += J[i] * J[k];
#pragma unroll
    for (int i = 0; i < 6; ++i) acc[21 + i] += J[i] * r;
    acc[27] += r * r;
  }

  static __device__ void solve(const double *cent, const double *o, double d[12],
                               double st[kStats]) {
    double m[kPlaneMoments];
    for (int i = 0; i < 5; ++i) m[i] = cent[i];
    for (int i = 0; i < kNB; ++i) m[5 + i] = o[i];
    plane_solve(m, d, st);
  }

  static int upload_target(navgpu_ctx *ctx, In &in, size_t nt) {
    double *dt, *dn, *dc;
    RC(to_dev(ctx, kH1, in.tgt, 3 * nt, &dt));
    RC(to_dev(ctx, kPlaneNrm, in.nrm, 3 * nt, &dn));
    RC(to_dev(ctx, kPlaneCurv, in.curv, nt, &dc));
    in.tgt = dt;
    in.nrm = dn;
    in.curv = dc;
    return NAVGPU_OK;
  }
};

}  // namespace

extern "C" {

int navgpu_normals_dev(navgpu_ctx *ctx, const double *pts, size_t n, const int32_t *idx,
                       int stride, int k, const double *viewpoint, double *normals,
                       double *curv) {
  return normals_run(ctx, pts, n, idx, stride, k, viewpoint, normals, curv);
}

int navgpu_normals_host(navgpu_ctx *ctx, const double *pts, size_t n, const int32_t *idx,
                        int stride, int k, const double *viewpoint, double *normals,
                        double *curv) {
  ARG_CHECK(ctx);
  ARG_CHECK(k >= 3 && k <= stride && stride <= 16);
  if (!n) return NAVGPU_OK;
  ARG_CHECK(pts && idx && normals);
  double *dp, *dn, *dc;
  int32_t *di;
  RC(to_dev(ctx, kH0, pts, 3 * n, &dp));
  RC(to_dev(ctx, kH2, idx, n * stride, &di));
  RC(ws(ctx, kH1, 3 * n, &dn));
  RC(ws(ctx, kH3, n, &dc));
  RC(normals_run(ctx, dp, n, di, stride, k, viewpoint, dn, dc));
  HIP_TRY(hipMemcpyAsync(normals, dn, 24 * n, hipMemcpyDeviceToHost, ctx->stream));
  if (curv) HIP_TRY(hipMemcpyAsync(curv, dc, 8 * n, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return NAVGPU_OK;
}

int navgpu_cloud_normals_dev(navgpu_ctx *ctx, const double *pts, size_t n, int k,
                             const double *viewpoint, double *normals, double *curv) {
  return cloud_normals_run(ctx, pts, n, k, viewpoint, normals, curv);
}

int navgpu_cloud_normals_host(navgpu_ctx *ctx, const double *pts, size_t n, int k,
                              const double *viewpoint, double *normals, double *curv) {
  ARG_CHECK(ctx);
  ARG_CHECK(k >= 3 && k <= 16);
  if (!n) return NAVGPU_OK;
  ARG_CHECK(pts && normals);
  double *dp, *dn, *dc;
  RC(to_dev(ctx, kH0, pts, 3 * n, &dp));
  RC(ws(ctx, kH1, 3 * n, &dn));
  RC(ws(ctx, kH3, n, &dc));
  RC(cloud_normals_run(ctx, dp, n, k, viewpoint, dn, dc));
  HIP_TRY(hipMemcpyAsync(normals, dn, 24 * n, hipMemcpyDeviceToHost, ctx->stream));
  if (curv) HIP_TRY(hipMemcpyAsync(curv, dc, 8 * n, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return navgpu_knn_check(ctx);
}

int navgpu_align_plane_dev(navgpu_ctx *ctx, const double *src, size_t nq, const double *tgt,
                           size_t nt, const double *tgt_normals, const double *tgt_curv,
                           const int32_t *idx, const double *dist, int stride, double max_dist,
                           double max_curv, const int32_t *mask, double *delta, double *pose,
                           double *stats) {
  return step_run<PlaneMetric>(ctx, {src, tgt, tgt_normals, tgt_curv, idx, dist, mask, nq,
                                     (int)nt, stride, max_dist, max_curv},
                               nt, delta, pose, stats, nullptr);
}

int navgpu_align_plane_host(navgpu_ctx *ctx, const double *src, size_t nq, const double *tgt,
                            size_t nt, const double *tgt_normals, const double *tgt_curv,
                            const int32_t *idx, const double *dist, int stride, double max_dist,
                            double max_curv, const int32_t *mask, double Rm[9], double t[3],
                            double stats[6]) {
  return step_host<PlaneMetric>(ctx, {src, tgt, tgt_normals, tgt_curv, idx, dist, mask, nq,
                                      (int)nt, stride, max_dist, max_curv},
                                nt, Rm, t, stats);
}

int navgpu_icp_plane_dev(navgpu_ctx *ctx, const double *src, size_t nq, const double *tgt,
                         size_t nt, const double *tgt_normals, const double *tgt_curv, int iters,
                         double max_dist, double max_curv, const int32_t *mask, double *pose,
                         double *hist, double *stats) {
  return icp_run<PlaneMetric>(ctx, {src, tgt, tgt_normals, tgt_curv, nullptr, nullptr, mask, nq,
                                    (int)nt, 1, max_dist, max_curv},
                              nt, iters, pose, hist, stats);
}

int navgpu_icp_plane_host(navgpu_ctx *ctx, const double *src, size_t nq, const double *tgt,
                          size_t nt, int kn, const double *viewpoint, int iters, double max_dist,
                          double max_curv, const int32_t *mask, double pose[12], double *hist,
                          double *stats) {
  ARG_CHECK(ctx && pose);
  ARG_CHECK(iters >= 1 && iters <= 64);
  ARG_CHECK(kn >= 3 && kn <= 16);
  ARG_CHECK(nq == 0 || src);
  ARG_CHECK(nt == 0 || tgt);
  PlaneIn in{src, tgt, nullptr, nullptr, nullptr, nullptr, mask, nq, (int)nt, 1, max_dist,
             max_curv};
  RC(upload_queries(ctx, in));
  RC(PlaneMetric::upload_target(ctx, in, nt));  // the cloud alone: its normals are made here
  if (nt) {
    double *dn, *dc;
    RC(ws(ctx, kPlaneNrm, 3 * nt, &dn));
    RC(ws(ctx, kPlaneCurv, nt, &dc));
    RC(cloud_normals_run(ctx, in.tgt, nt, kn, viewpoint, dn, dc));
    in.nrm = dn;
    in.curv = dc;
  }
  return icp_finish_host<PlaneMetric>(ctx, in, nt, iters, pose, hist, stats);
}

int navgpu_icp_plane_normals_host(navgpu_ctx *ctx, const double *src, size_t nq,
                                  const double *tgt, size_t nt, const double *tgt_normals,
                                  const double *tgt_curv, int iters, double max_dist,
                                  double max_curv, const int32_t *mask, double pose[12],
                                  double *hist, double *stats) {
  ARG_CHECK(ctx && pose);
  ARG_CHECK(iters >= 1 && iters <= 64);
  ARG_CHECK(nq == 0 || src);
  ARG_CHECK(nt == 0 || (tgt && tgt_normals && tgt_curv));
  PlaneIn in{src, tgt, tgt_normals, tgt_curv, nullptr, nullptr, mask, nq, (int)nt, 1, max_dist,
             max_curv};
  RC(upload_queries(ctx, in));
  RC(PlaneMetric::upload_target(ctx, in, nt));
  return icp_finish_host<PlaneMetric>(ctx, in, nt, iters, pose, hist, stats);
}

}  // extern "C"
