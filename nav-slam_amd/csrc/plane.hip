// plane.hip — point-to-plane registration on the global k-NN's output:
// surface normals from each point's k-neighbourhood (k_normals), the gated
// point-to-plane moments (k_plane_moments), the linearised step
// (k_plane_solve, plane_solve.h) and the ICP loop over them. Fourth
// translation unit of libnavgpu.so. Beyond the reference, which has neither
// normals nor a rotation fit; the checkers are the numpy restatements in
// tests/test_gpu_plane.py. DESIGN.md §11.
//
//   k_normals           mu, centred covariance, sym3_eig, orientation
//   k_plane_moments<0>  pass A: n, sum p, bad indices
//   k_plane_finish      pbar from the pass-A partials
//   k_plane_moments<1>  pass B: A (21), b (6), sum r^2 about pbar
//   k_plane_solve       plane_solve, stats, pose <- delta o pose
//
// The sums follow align.hip's rule (det_reduce.h): reproducible bit for bit,
// no floating-point atomics, a grid that depends on nq alone.
#include "navgpu_common.h"

#include "plane_solve.h"
#include "det_reduce.h"

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
constexpr int kPlaneBlock = kRedBlock;
// Independent queries in flight per lane. Pass B keeps 28 f64 accumulators
// (56 VGPRs) per lane, and a query in flight holds p, q and the normal (18
// VGPRs) beside its index, distance, mask and curvature: two of them stay
// within the 128-VGPR budget of four waves per SIMD, four do not.
constexpr int kPlaneU = 2;
constexpr int kPlaneTile = kPlaneBlock * kPlaneU;  // queries per block and trip
constexpr int kPlaneMaxGrid = 1024;
constexpr int kPlaneRow = 32;  // doubles per partial row (256 B)
constexpr int kPA = 5;         // pass A: n, sum p, bad
constexpr int kPB = 28;        // pass B: A upper (21), b (6), sum r^2

struct PlaneIn {
  const double *src, *tgt, *nrm, *curv;  // the target's are never null here
  const int32_t *idx;
  const double *dist;
  const int32_t *mask;  // nullable
  size_t nq;
  int nt, stride;
  double max_dist, max_curv;
};

// One pass over the queries. k_align_moments' gate (index in range, distance
// <= max_dist, mask set) and one more condition, the neighbour's curvature
// <= max_curv: a NaN curvature (no normal there) fails it. A query rejected
// by the first three has its j replaced by 0 before any gather, so an index
// outside the cloud is counted (pass A) and never dereferenced.
template <int PASS>
__global__ __launch_bounds__(kPlaneBlock) void k_plane_moments(PlaneIn a,
                                                               const double *__restrict__ cent,
                                                               double *__restrict__ part) {
  constexpr int NV = PASS ? kPB : kPA;
  double acc[NV];
#pragma unroll
  for (int k = 0; k < NV; ++k) acc[k] = 0.0;
  double pb[3] = {0.0, 0.0, 0.0};
  if (PASS) {
#pragma unroll
    for (int c = 0; c < 3; ++c) pb[c] = cent[1 + c];
  }
  const size_t ntile = (a.nq + kPlaneTile - 1) / kPlaneTile;
  for (size_t tile = blockIdx.x; tile < ntile; tile += gridDim.x) {
    const size_t q0 = tile * kPlaneTile + threadIdx.x;
    size_t qq[kPlaneU];
    int j[kPlaneU], mk[kPlaneU];
    bool ok[kPlaneU], bad[kPlaneU];
    double d[kPlaneU], cv[kPlaneU];
    // every load of a phase is issued before the first is consumed
#pragma unroll
    for (int u = 0; u < kPlaneU; ++u) {
      const size_t q = q0 + (size_t)u * kPlaneBlock;
      qq[u] = q < a.nq ? q : a.nq - 1;  // ntile > 0 implies nq > 0
      j[u] = a.idx[qq[u] * a.stride];
      d[u] = a.dist[qq[u] * a.stride];
      mk[u] = 1;
    }
    if (a.mask) {
#pragma unroll
      for (int u = 0; u < kPlaneU; ++u) mk[u] = a.mask[qq[u]];
    }
#pragma unroll
    for (int u = 0; u < kPlaneU; ++u) {
      const bool in = q0 + (size_t)u * kPlaneBlock < a.nq;
      const int jj = j[u];
      ok[u] = in & (jj >= 0) & (jj < a.nt) & (d[u] <= a.max_dist) & (mk[u] != 0);
      bad[u] = in & ((jj < -1) | (jj >= a.nt));
      j[u] = ok[u] ? jj : 0;
    }
    double p[kPlaneU][3], t[kPlaneU][3], nn[kPlaneU][3];
#pragma unroll
    for (int u = 0; u < kPlaneU; ++u) {
      cv[u] = a.curv[j[u]];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        p[u][c] = a.src[3 * qq[u] + c];
        if (PASS) {
          t[u][c] = a.tgt[3 * (size_t)j[u] + c];
          nn[u][c] = a.nrm[3 * (size_t)j[u] + c];
        }
      }
    }
#pragma unroll
    for (int u = 0; u < kPlaneU; ++u) {
      const bool take = ok[u] & (cv[u] <= a.max_curv);
      if (PASS == 0) {
        if (bad[u]) acc[4] += 1.0;
        if (take) {
          acc[0] += 1.0;
#pragma unroll
          for (int c = 0; c < 3; ++c) acc[1 + c] += p[u][c];
        }
      } else if (take) {
        const double x = p[u][0] - pb[0], y = p[u][1] - pb[1], z = p[u][2] - pb[2];
        const double n0 = nn[u][0], n1 = nn[u][1], n2 = nn[u][2];
        double J[6];
        J[0] = y * n2 - z * n1;
        J[1] = z * n0 - x * n2;
        J[2] = x * n1 - y * n0;
        J[3] = n0;
        J[4] = n1;
        J[5] = n2;
        const double r = ((t[u][0] - p[u][0]) * n0 + (t[u][1] - p[u][1]) * n1) +
                         (t[u][2] - p[u][2]) * n2;
        int e = 0;
#pragma unroll
        for (int i = 0; i < 6; ++i)
#pragma unroll
          for (int k = i; k < 6; ++k) acc[e++] += J[i] * J[k];
#pragma unroll
        for (int i = 0; i < 6; ++i) acc[21 + i] += J[i] * r;
        acc[27] += r * r;
      }
    }
  }
  block_sum<NV>(acc, part + (size_t)blockIdx.x * kPlaneRow);
}

// cent = n, pbar, bad indices
__global__ __launch_bounds__(kPlaneBlock) void k_plane_finish(const double *__restrict__ partA,
                                                              int nblk, double *__restrict__ cent) {
  __shared__ double o[kPA];
  combine_rows<kPA, kPlaneRow>(partA, nblk, o);
  if (threadIdx.x == 0) {
    const double n = o[0];
    cent[0] = n;
    for (int c = 0; c < 3; ++c) cent[1 + c] = n > 0.0 ? o[1 + c] / n : 0.0;
    cent[4] = o[4];
  }
}

__global__ __launch_bounds__(kPlaneBlock) void k_plane_solve(const double *__restrict__ partB,
                                                             int nblk,
                                                             const double *__restrict__ cent,
                                                             double *__restrict__ delta,
                                                             double *__restrict__ stats,
                                                             double *pose, double *hist) {
  __shared__ double o[kPB];
  combine_rows<kPB, kPlaneRow>(partB, nblk, o);
  if (threadIdx.x != 0) return;
  double m[kPlaneMoments], d[12], st[6];
  for (int i = 0; i < 5; ++i) m[i] = cent[i];
  for (int i = 0; i < kPB; ++i) m[5 + i] = o[i];
  plane_solve(m, d, st);
  for (int i = 0; i < 12; ++i) delta[i] = d[i];
  for (int i = 0; i < 6; ++i) stats[i] = st[i];
  if (pose) {
    double P[12];
    for (int i = 0; i < 12; ++i) P[i] = pose[i];
    pose_compose(d, P);
    for (int i = 0; i < 12; ++i) pose[i] = P[i];
    if (hist)
      for (int i = 0; i < 12; ++i) hist[i] = P[i];
  }
}

// workspace of one plane step: pass-A rows, pass-B rows, the finish record
constexpr size_t kPlanePartDoubles = 2 * (size_t)kPlaneMaxGrid * kPlaneRow + kPlaneRow;

// The plane step on device pointers; hist (nullable) also receives the
// composed pose.
int plane_run(navgpu_ctx *ctx, const double *src, size_t nq, const double *tgt, size_t nt,
              const double *tgt_normals, const double *tgt_curv, const int32_t *idx,
              const double *dist, int stride, double max_dist, double max_curv,
              const int32_t *mask, double *delta, double *pose, double *stats, double *hist) {
  ARG_CHECK(ctx && delta && stats);
  ARG_CHECK(stride >= 1 && stride <= 16);
  ARG_CHECK(max_dist == max_dist && max_curv == max_curv);  // not a NaN
  ARG_CHECK(nq < (size_t)INT32_MAX && nt < (size_t)INT32_MAX);
  ARG_CHECK(nq == 0 || (src && idx && dist));
  ARG_CHECK(nt == 0 || (tgt && tgt_normals && tgt_curv));
  double *part;
  RC(ws(ctx, kPlanePart, kPlanePartDoubles, &part));
  double *partA = part, *partB = part + (size_t)kPlaneMaxGrid * kPlaneRow;
  double *cent = partB + (size_t)kPlaneMaxGrid * kPlaneRow;
  // an empty target accepts nothing, and j = 0 then reads the workspace
  const PlaneIn in{src, nt ? tgt : part, nt ? tgt_normals : part, nt ? tgt_curv : part, idx, dist,
                   mask, nq, (int)nt, stride, max_dist, max_curv};
  const unsigned grid = det_grid(nq, kPlaneTile, kPlaneMaxGrid);
  hipStream_t s = ctx->stream;
  TimedRegion tr(ctx, "align_plane");
  hipLaunchKernelGGL(k_plane_moments<0>, dim3(grid), dim3(kPlaneBlock), 0, s, in,
                     (const double *)nullptr, partA);
  CHECK_LAUNCH("k_plane_moments<0>");
  hipLaunchKernelGGL(k_plane_finish, dim3(1), dim3(kPlaneBlock), 0, s, (const double *)partA,
                     (int)grid, cent);
  CHECK_LAUNCH("k_plane_finish");
  hipLaunchKernelGGL(k_plane_moments<1>, dim3(grid), dim3(kPlaneBlock), 0, s, in,
                     (const double *)cent, partB);
  CHECK_LAUNCH("k_plane_moments<1>");
  hipLaunchKernelGGL(k_plane_solve, dim3(1), dim3(kPlaneBlock), 0, s, (const double *)partB,
                     (int)grid, (const double *)cent, delta, stats, pose, hist);
  CHECK_LAUNCH("k_plane_solve");
  return NAVGPU_OK;
}

int icp_plane_run(navgpu_ctx *ctx, const double *src, size_t nq, const double *tgt, size_t nt,
                  const double *tgt_normals, const double *tgt_curv, int iters, double max_dist,
                  double max_curv, const int32_t *mask, double *pose, double *hist,
                  double *stats) {
  ARG_CHECK(ctx && pose);
  ARG_CHECK(iters >= 1 && iters <= 64);
  ARG_CHECK(nq < (size_t)INT32_MAX / 2 && nt < (size_t)INT32_MAX / 2);  // navgpu_knn_dev's range
  ARG_CHECK(nq == 0 || src);
  ARG_CHECK(nt == 0 || (tgt && tgt_normals && tgt_curv));
  double *cur, *nnd, *scratch;
  int32_t *nni;
  RC(ws(ctx, kIcpCur, 3 * std::max<size_t>(nq, 1), &cur));
  RC(ws(ctx, kIcpIdx, std::max<size_t>(nq, 1), &nni));
  RC(ws(ctx, kIcpDist, std::max<size_t>(nq, 1), &nnd));
  RC(ws(ctx, kPlaneOut, 18, &scratch));
  for (int i = 0; i < iters; ++i) {
    {
      TimedRegion tr(ctx, "icp_transform");
      RC(navgpu_transform_pose_dev(ctx, src, nq, pose, cur));
    }
    RC(navgpu_knn_dev(ctx, tgt, nt, cur, nq, 1, nni, nnd));
    RC(plane_run(ctx, cur, nq, tgt, nt, tgt_normals, tgt_curv, nni, nnd, 1, max_dist, max_curv,
                 mask, scratch, pose, stats ? stats + 6 * (size_t)i : scratch + 12,
                 hist ? hist + 12 * (size_t)i : nullptr));
  }
  return NAVGPU_OK;
}

// host arrays onto the context's stream; a null or empty source gives null
template <class T>
int to_dev(navgpu_ctx *ctx, int slot, const T *host, size_t count, T **dev) {
  *dev = nullptr;
  if (!host || !count) return NAVGPU_OK;
  RC(ws(ctx, slot, count, dev));
  HIP_TRY(hipMemcpyAsync(*dev, host, count * sizeof(T), hipMemcpyHostToDevice, ctx->stream));
  return NAVGPU_OK;
}

// the ICP loop on uploaded clouds, its results back on the host
int icp_plane_finish_host(navgpu_ctx *ctx, const double *ds, size_t nq, const double *dt,
                          size_t nt, const double *dn, const double *dc, int iters,
                          double max_dist, double max_curv, const int32_t *dm, double pose[12],
                          double *hist, double *stats) {
  hipStream_t s = ctx->stream;
  double *dout;  // pose[12], hist[iters][12], stats[iters][6]
  RC(ws(ctx, kH5, 12 + 18 * (size_t)iters, &dout));
  double *dhist = dout + 12, *dstats = dhist + 12 * (size_t)iters;
  HIP_TRY(hipMemcpyAsync(dout, pose, 12 * sizeof(double), hipMemcpyHostToDevice, s));
  RC(icp_plane_run(ctx, ds, nq, dt, nt, dn, dc, iters, max_dist, max_curv, dm, dout, dhist,
                   dstats));
  HIP_TRY(hipMemcpyAsync(pose, dout, 12 * sizeof(double), hipMemcpyDeviceToHost, s));
  if (hist)
    HIP_TRY(hipMemcpyAsync(hist, dhist, 12 * sizeof(double) * iters, hipMemcpyDeviceToHost, s));
  if (stats)
    HIP_TRY(hipMemcpyAsync(stats, dstats, 6 * sizeof(double) * iters, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  return nq ? navgpu_knn_check(ctx) : NAVGPU_OK;
}

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
  return plane_run(ctx, src, nq, tgt, nt, tgt_normals, tgt_curv, idx, dist, stride, max_dist,
                   max_curv, mask, delta, pose, stats, nullptr);
}

int navgpu_align_plane_host(navgpu_ctx *ctx, const double *src, size_t nq, const double *tgt,
                            size_t nt, const double *tgt_normals, const double *tgt_curv,
                            const int32_t *idx, const double *dist, int stride, double max_dist,
                            double max_curv, const int32_t *mask, double Rm[9], double t[3],
                            double stats[6]) {
  ARG_CHECK(ctx && Rm && t && stats);
  ARG_CHECK(stride >= 1 && stride <= 16);
  ARG_CHECK(nq == 0 || (src && idx && dist));
  ARG_CHECK(nt == 0 || (tgt && tgt_normals && tgt_curv));
  double *ds, *dt, *dn, *dc, *dd, *dout;
  int32_t *di, *dm;
  RC(to_dev(ctx, kH0, src, 3 * nq, &ds));
  RC(to_dev(ctx, kH2, idx, nq * stride, &di));
  RC(to_dev(ctx, kH3, dist, nq * stride, &dd));
  RC(to_dev(ctx, kH4, mask, nq, &dm));
  RC(to_dev(ctx, kH1, tgt, 3 * nt, &dt));
  RC(to_dev(ctx, kPlaneNrm, tgt_normals, 3 * nt, &dn));
  RC(to_dev(ctx, kPlaneCurv, tgt_curv, nt, &dc));
  RC(ws(ctx, kH5, 18, &dout));
  RC(plane_run(ctx, ds, nq, dt, nt, dn, dc, di, dd, stride, max_dist, max_curv, dm, dout,
               nullptr, dout + 12, nullptr));
  double out[18];
  HIP_TRY(hipMemcpyAsync(out, dout, sizeof(out), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  memcpy(Rm, out, 9 * sizeof(double));
  memcpy(t, out + 9, 3 * sizeof(double));
  memcpy(stats, out + 12, 6 * sizeof(double));
  return NAVGPU_OK;
}

int navgpu_icp_plane_dev(navgpu_ctx *ctx, const double *src, size_t nq, const double *tgt,
                         size_t nt, const double *tgt_normals, const double *tgt_curv, int iters,
                         double max_dist, double max_curv, const int32_t *mask, double *pose,
                         double *hist, double *stats) {
  return icp_plane_run(ctx, src, nq, tgt, nt, tgt_normals, tgt_curv, iters, max_dist, max_curv,
                       mask, pose, hist, stats);
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
  double *ds, *dt, *dn = nullptr, *dc = nullptr;
  int32_t *dm;
  RC(to_dev(ctx, kH0, src, 3 * nq, &ds));
  RC(to_dev(ctx, kH4, mask, nq, &dm));
  RC(to_dev(ctx, kH1, tgt, 3 * nt, &dt));
  if (nt) {
    RC(ws(ctx, kPlaneNrm, 3 * nt, &dn));
    RC(ws(ctx, kPlaneCurv, nt, &dc));
    RC(cloud_normals_run(ctx, dt, nt, kn, viewpoint, dn, dc));
  }
  return icp_plane_finish_host(ctx, ds, nq, dt, nt, dn, dc, iters, max_dist, max_curv, dm, pose,
                               hist, stats);
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
  double *ds, *dt, *dn, *dc;
  int32_t *dm;
  RC(to_dev(ctx, kH0, src, 3 * nq, &ds));
  RC(to_dev(ctx, kH4, mask, nq, &dm));
  RC(to_dev(ctx, kH1, tgt, 3 * nt, &dt));
  RC(to_dev(ctx, kPlaneNrm, tgt_normals, 3 * nt, &dn));
  RC(to_dev(ctx, kPlaneCurv, tgt_curv, nt, &dc));
  return icp_plane_finish_host(ctx, ds, nq, dt, nt, dn, dc, iters, max_dist, max_curv, dm, pose,
                               hist, stats);
}

}  // extern "C"
