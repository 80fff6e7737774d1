// align.hip — 6-DOF rigid registration on the global k-NN's output: the
// gated correspondence moments (k_align_moments), the closed-form pose
// (k_align_solve, align_solve.h), a transform by a device-resident pose
// (k_transform_pose) and the ICP loop over them. Third translation unit of
// libnavgpu.so. Beyond the reference, whose optimiser is translation-only
// (src/slam.c:300-389); the checker is the numpy restatement in
// tests/test_gpu_align.py. DESIGN.md §10.
//
//   k_align_moments<0>  pass A: n, sum p, sum q, sum |q-p|^2, bad indices
//   k_align_finish      pbar, qbar from the pass-A partials
//   k_align_moments<1>  pass B: centred H, sum |p-pbar|^2, sum |q-qbar|^2
//   k_align_solve       Horn's closed form, stats, pose <- delta o pose
//   k_transform_pose    out = t + R p, the pose read from device memory
//
// Sums are reproducible bit for bit: per-thread f64 accumulators over a
// grid-stride loop, a fixed butterfly per wave, the waves of a block added in
// wave order, one partial row per block, the rows added in a fixed order. The
// grid is a function of nq alone. There are no floating-point atomics. The
// helpers are in det_reduce.h, shared with plane.hip.
#include "navgpu_common.h"

#include "align_solve.h"
#include "det_reduce.h"

using namespace nv;

namespace {

constexpr int kAlignBlock = kRedBlock;  // 4 waves, one per SIMD
// Independent queries in flight per lane: the 24-B target gather is a random
// access, so each lane issues kAlignU of them before it consumes the first.
constexpr int kAlignU = 4;
constexpr int kAlignTile = kAlignBlock * kAlignU;  // queries per block and trip
constexpr int kAlignMaxGrid = 1024;  // 4 blocks (16 waves) on each of the 256 CUs
constexpr int kAlignRow = 16;        // doubles per partial row (128 B)
constexpr int kNA = 9;               // pass A: n, sum p, sum q, sum |q-p|^2, bad
constexpr int kNB = 11;              // pass B: H, Spp, Sqq

struct AlignIn {
  const double *src, *tgt;  // tgt is never null here (align_run substitutes)
  const int32_t *idx;
  const double *dist;
  const int32_t *mask;  // nullable
  size_t nq;
  int nt, stride;
  double max_dist;
};

// One pass over the queries. A query is accepted when its slot-0 neighbour j
// is a target index, its distance passes the gate (a NaN fails `<=`) and its
// mask is set. A rejected query's j is replaced by 0 before the gather, so an
// index outside the cloud is counted (pass A) and never dereferenced.
template <int PASS>
__global__ __launch_bounds__(kAlignBlock) void k_align_moments(AlignIn a,
                                                               const double *__restrict__ cent,
                                                               double *__restrict__ part) {
  constexpr int NV = PASS ? kNB : kNA;
  double acc[NV];
#pragma unroll
  for (int k = 0; k < NV; ++k) acc[k] = 0.0;
  double pb[3] = {0.0, 0.0, 0.0}, qb[3] = {0.0, 0.0, 0.0};
  if (PASS) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      pb[c] = cent[1 + c];
      qb[c] = cent[4 + c];
    }
  }
  const size_t ntile = (a.nq + kAlignTile - 1) / kAlignTile;
  for (size_t tile = blockIdx.x; tile < ntile; tile += gridDim.x) {
    const size_t q0 = tile * kAlignTile + threadIdx.x;
    size_t qq[kAlignU];
    int j[kAlignU];
    bool ok[kAlignU], bad[kAlignU];
    // every load of a phase is issued before the first is consumed: no
    // branch inside a phase (the mask test is uniform and outside the loops)
    int mk[kAlignU];
    double d[kAlignU];
#pragma unroll
    for (int u = 0; u < kAlignU; ++u) {
      const size_t q = q0 + (size_t)u * kAlignBlock;
      qq[u] = q < a.nq ? q : a.nq - 1;  // ntile > 0 implies nq > 0
      j[u] = a.idx[qq[u] * a.stride];
      d[u] = a.dist[qq[u] * a.stride];
      mk[u] = 1;
    }
    if (a.mask) {
#pragma unroll
      for (int u = 0; u < kAlignU; ++u) mk[u] = a.mask[qq[u]];
    }
#pragma unroll
    for (int u = 0; u < kAlignU; ++u) {
      const bool in = q0 + (size_t)u * kAlignBlock < a.nq;
      const int jj = j[u];
      ok[u] = in & (jj >= 0) & (jj < a.nt) & (d[u] <= a.max_dist) & (mk[u] != 0);
      bad[u] = in & ((jj < -1) | (jj >= a.nt));
      j[u] = ok[u] ? jj : 0;
    }
    double p[kAlignU][3], t[kAlignU][3];
#pragma unroll
    for (int u = 0; u < kAlignU; ++u) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        p[u][c] = a.src[3 * qq[u] + c];
        t[u][c] = a.tgt[3 * (size_t)j[u] + c];
      }
    }
#pragma unroll
    for (int u = 0; u < kAlignU; ++u) {
      if (PASS == 0) {
        if (bad[u]) acc[8] += 1.0;
        if (ok[u]) {
          acc[0] += 1.0;
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            acc[1 + c] += p[u][c];
            acc[4 + c] += t[u][c];
          }
          const double dx = t[u][0] - p[u][0], dy = t[u][1] - p[u][1], dz = t[u][2] - p[u][2];
          acc[7] += (dx * dx + dy * dy) + dz * dz;
        }
      } else if (ok[u]) {
        double x[3], y[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          x[c] = p[u][c] - pb[c];
          y[c] = t[u][c] - qb[c];
        }
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
          for (int c = 0; c < 3; ++c) acc[3 * r + c] += x[r] * y[c];
        acc[9] += (x[0] * x[0] + x[1] * x[1]) + x[2] * x[2];
        acc[10] += (y[0] * y[0] + y[1] * y[1]) + y[2] * y[2];
      }
    }
  }
  block_sum<NV>(acc, part + (size_t)blockIdx.x * kAlignRow);
}

// cent = n, pbar, qbar, sum |q-p|^2, bad indices
__global__ __launch_bounds__(kAlignBlock) void k_align_finish(const double *__restrict__ partA,
                                                              int nblk, double *__restrict__ cent) {
  __shared__ double o[kNA];
  combine_rows<kNA, kAlignRow>(partA, nblk, o);
  if (threadIdx.x == 0) {
    const double n = o[0];
    cent[0] = n;
    for (int c = 0; c < 3; ++c) {
      cent[1 + c] = n > 0.0 ? o[1 + c] / n : 0.0;
      cent[4 + c] = n > 0.0 ? o[4 + c] / n : 0.0;
    }
    cent[7] = o[7];
    cent[8] = o[8];
  }
}

__global__ __launch_bounds__(kAlignBlock) void k_align_solve(const double *__restrict__ partB,
                                                             int nblk,
                                                             const double *__restrict__ cent,
                                                             double *__restrict__ delta,
                                                             double *__restrict__ stats,
                                                             double *pose, double *hist) {
  __shared__ double o[kNB];
  combine_rows<kNB, kAlignRow>(partB, nblk, o);
  if (threadIdx.x != 0) return;
  double m[kAlignMoments], d[12], st[4];
  for (int i = 0; i < 8; ++i) m[i] = cent[i];
  for (int i = 0; i < kNB; ++i) m[8 + i] = o[i];
  m[19] = cent[8];
  align_solve(m, d, st);
  for (int i = 0; i < 12; ++i) delta[i] = d[i];
  for (int i = 0; i < 4; ++i) stats[i] = st[i];
  if (pose) {
    double P[12];
    for (int i = 0; i < 12; ++i) P[i] = pose[i];
    pose_compose(d, P);
    for (int i = 0; i < 12; ++i) pose[i] = P[i];
    if (hist)
      for (int i = 0; i < 12; ++i) hist[i] = P[i];
  }
}

// k_transform (navgpu.hip) with R, t read from device memory: the same
// operation order, t + ((R0 x + R1 y) + R2 z)
__global__ __launch_bounds__(256) void k_transform_pose(const double *__restrict__ pts, size_t n,
                                                        const double *__restrict__ pose,
                                                        double *__restrict__ out) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double lx = pts[3 * i], ly = pts[3 * i + 1], lz = pts[3 * i + 2];
  const double rx = pose[0] * lx + pose[1] * ly + pose[2] * lz;
  const double ry = pose[3] * lx + pose[4] * ly + pose[5] * lz;
  const double rz = pose[6] * lx + pose[7] * ly + pose[8] * lz;
  out[3 * i] = pose[9] + rx;
  out[3 * i + 1] = pose[10] + ry;
  out[3 * i + 2] = pose[11] + rz;
}

// workspace of one align step: pass-A rows, pass-B rows, the finish record
constexpr size_t kAlignPartDoubles = 2 * (size_t)kAlignMaxGrid * kAlignRow + kAlignRow;

unsigned align_grid(size_t nq) {
  return det_grid(nq, kAlignTile, kAlignMaxGrid);
}

// The align step on device pointers; hist (nullable) also receives the
// composed pose.
int align_run(navgpu_ctx *ctx, const double *src, size_t nq, const double *tgt, size_t nt,
              const int32_t *idx, const double *dist, int stride, double max_dist,
              const int32_t *mask, double *delta, double *pose, double *stats, double *hist) {
  ARG_CHECK(ctx && delta && stats);
  ARG_CHECK(stride >= 1 && stride <= 16);
  ARG_CHECK(max_dist == max_dist);  // not a NaN
  ARG_CHECK(nq < (size_t)INT32_MAX && nt < (size_t)INT32_MAX);
  ARG_CHECK(nq == 0 || (src && idx && dist));
  ARG_CHECK(nt == 0 || tgt);
  double *part;
  RC(ws(ctx, kAlignPart, kAlignPartDoubles, &part));
  double *partA = part, *partB = part + (size_t)kAlignMaxGrid * kAlignRow;
  double *cent = partB + (size_t)kAlignMaxGrid * kAlignRow;
  // an empty target accepts nothing, and j = 0 then reads the workspace
  const AlignIn in{src, nt ? tgt : part, idx, dist, mask, nq, (int)nt, stride, max_dist};
  const unsigned grid = align_grid(nq);
  hipStream_t s = ctx->stream;
  TimedRegion tr(ctx, "align");
  hipLaunchKernelGGL(k_align_moments<0>, dim3(grid), dim3(kAlignBlock), 0, s, in,
                     (const double *)nullptr, partA);
  CHECK_LAUNCH("k_align_moments<0>");
  hipLaunchKernelGGL(k_align_finish, dim3(1), dim3(kAlignBlock), 0, s, (const double *)partA,
                     (int)grid, cent);
  CHECK_LAUNCH("k_align_finish");
  hipLaunchKernelGGL(k_align_moments<1>, dim3(grid), dim3(kAlignBlock), 0, s, in,
                     (const double *)cent, partB);
  CHECK_LAUNCH("k_align_moments<1>");
  hipLaunchKernelGGL(k_align_solve, dim3(1), dim3(kAlignBlock), 0, s, (const double *)partB,
                     (int)grid, (const double *)cent, delta, stats, pose, hist);
  CHECK_LAUNCH("k_align_solve");
  return NAVGPU_OK;
}

int transform_pose_run(navgpu_ctx *ctx, const double *pts, size_t n, const double *pose,
                       double *out) {
  if (!n) return NAVGPU_OK;
  ARG_CHECK(pts && pose && out);
  hipLaunchKernelGGL(k_transform_pose, dim3(grid1d(n, 256)), dim3(256), 0, ctx->stream, pts, n,
                     pose, out);
  CHECK_LAUNCH("k_transform_pose");
  return NAVGPU_OK;
}

}  // namespace

extern "C" {

int navgpu_align_dev(navgpu_ctx *ctx, const double *src, size_t nq, const double *tgt, size_t nt,
                     const int32_t *idx, const double *dist, int stride, double max_dist,
                     const int32_t *mask, double *delta, double *pose, double *stats) {
  return align_run(ctx, src, nq, tgt, nt, idx, dist, stride, max_dist, mask, delta, pose, stats,
                   nullptr);
}

int navgpu_align_host(navgpu_ctx *ctx, const double *src, size_t nq, const double *tgt, size_t nt,
                      const int32_t *idx, const double *dist, int stride, double max_dist,
                      const int32_t *mask, double Rm[9], double t[3], double stats[4]) {
  ARG_CHECK(ctx && Rm && t && stats);
  ARG_CHECK(stride >= 1 && stride <= 16);
  ARG_CHECK(nq == 0 || (src && idx && dist));
  ARG_CHECK(nt == 0 || tgt);
  double *ds = nullptr, *dt = nullptr, *dd = nullptr, *dout;
  int32_t *di = nullptr, *dm = nullptr;
  hipStream_t s = ctx->stream;
  if (nq) {
    RC(ws(ctx, kH0, 3 * nq, &ds));
    RC(ws(ctx, kH2, nq * stride, &di));
    RC(ws(ctx, kH3, nq * stride, &dd));
    HIP_TRY(hipMemcpyAsync(ds, src, 24 * nq, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(di, idx, 4 * nq * stride, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(dd, dist, 8 * nq * stride, hipMemcpyHostToDevice, s));
    if (mask) {
      RC(ws(ctx, kH4, nq, &dm));
      HIP_TRY(hipMemcpyAsync(dm, mask, 4 * nq, hipMemcpyHostToDevice, s));
    }
  }
  if (nt) {
    RC(ws(ctx, kH1, 3 * nt, &dt));
    HIP_TRY(hipMemcpyAsync(dt, tgt, 24 * nt, hipMemcpyHostToDevice, s));
  }
  RC(ws(ctx, kH5, 16, &dout));
  RC(align_run(ctx, ds, nq, dt, nt, di, dd, stride, max_dist, dm, dout, nullptr, dout + 12,
               nullptr));
  double out[16];
  HIP_TRY(hipMemcpyAsync(out, dout, sizeof(out), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  memcpy(Rm, out, 9 * sizeof(double));
  memcpy(t, out + 9, 3 * sizeof(double));
  memcpy(stats, out + 12, 4 * sizeof(double));
  return NAVGPU_OK;
}

int navgpu_transform_pose_dev(navgpu_ctx *ctx, const double *pts, size_t n, const double *pose_dev,
                              double *out) {
  ARG_CHECK(ctx);
  return transform_pose_run(ctx, pts, n, pose_dev, out);
}

int navgpu_icp_dev(navgpu_ctx *ctx, const double *src, size_t nq, const double *tgt, size_t nt,
                   int iters, double max_dist, const int32_t *mask, double *pose, double *hist,
                   double *stats) {
  ARG_CHECK(ctx && pose);
  ARG_CHECK(iters >= 1 && iters <= 64);
  ARG_CHECK(nq < (size_t)INT32_MAX / 2 && nt < (size_t)INT32_MAX / 2);  // navgpu_knn_dev's range
  ARG_CHECK(nq == 0 || src);
  ARG_CHECK(nt == 0 || tgt);
  double *cur, *nnd, *scratch;
  int32_t *nni;
  RC(ws(ctx, kIcpCur, 3 * std::max<size_t>(nq, 1), &cur));
  RC(ws(ctx, kIcpIdx, std::max<size_t>(nq, 1), &nni));
  RC(ws(ctx, kIcpDist, std::max<size_t>(nq, 1), &nnd));
  RC(ws(ctx, kAlignOut, 16, &scratch));
  for (int i = 0; i < iters; ++i) {
    {
      TimedRegion tr(ctx, "icp_transform");
      RC(transform_pose_run(ctx, src, nq, pose, cur));
    }
    RC(navgpu_knn_dev(ctx, tgt, nt, cur, nq, 1, nni, nnd));
    RC(align_run(ctx, cur, nq, tgt, nt, nni, nnd, 1, max_dist, mask, scratch, pose,
                 stats ? stats + 4 * (size_t)i : scratch + 12,
                 hist ? hist + 12 * (size_t)i : nullptr));
  }
  return NAVGPU_OK;
}

int navgpu_icp_host(navgpu_ctx *ctx, const double *src, size_t nq, const double *tgt, size_t nt,
                    int iters, double max_dist, const int32_t *mask, double pose[12], double *hist,
                    double *stats) {
  ARG_CHECK(ctx && pose);
  ARG_CHECK(iters >= 1 && iters <= 64);
  ARG_CHECK(nq == 0 || src);
  ARG_CHECK(nt == 0 || tgt);
  double *ds = nullptr, *dt = nullptr, *dout;
  int32_t *dm = nullptr;
  hipStream_t s = ctx->stream;
  if (nq) {
    RC(ws(ctx, kH0, 3 * nq, &ds));
    HIP_TRY(hipMemcpyAsync(ds, src, 24 * nq, hipMemcpyHostToDevice, s));
    if (mask) {
      RC(ws(ctx, kH4, nq, &dm));
      HIP_TRY(hipMemcpyAsync(dm, mask, 4 * nq, hipMemcpyHostToDevice, s));
    }
  }
  if (nt) {
    RC(ws(ctx, kH1, 3 * nt, &dt));
    HIP_TRY(hipMemcpyAsync(dt, tgt, 24 * nt, hipMemcpyHostToDevice, s));
  }
  // pose[12], hist[iters][12], stats[iters][4]
  RC(ws(ctx, kH5, 12 + 16 * (size_t)iters, &dout));
  double *dhist = dout + 12, *dstats = dhist + 12 * (size_t)iters;
  HIP_TRY(hipMemcpyAsync(dout, pose, 12 * sizeof(double), hipMemcpyHostToDevice, s));
  RC(navgpu_icp_dev(ctx, ds, nq, dt, nt, iters, max_dist, dm, dout, dhist, dstats));
  HIP_TRY(hipMemcpyAsync(pose, dout, 12 * sizeof(double), hipMemcpyDeviceToHost, s));
  if (hist)
    HIP_TRY(hipMemcpyAsync(hist, dhist, 12 * sizeof(double) * iters, hipMemcpyDeviceToHost, s));
  if (stats)
    HIP_TRY(hipMemcpyAsync(stats, dstats, 4 * sizeof(double) * iters, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  return nq ? navgpu_knn_check(ctx) : NAVGPU_OK;
}

}  // extern "C"
