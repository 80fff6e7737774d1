// reg_step.h — what the registration metrics of align.hip (point-to-point)
// and plane.hip (point-to-plane) share: the gate on a query's neighbour, the
// two-pass moments kernel, the finish and solve kernels, the step driver, the
// ICP loop and the host staging. Internal; included after navgpu_common.h and
// det_reduce.h. DESIGN.md §10 and §11.
//
//   k_reg_moments<P, 0>  pass A: n, the coordinate sums, ..., bad indices
//   k_reg_finish<P>      the centroids from the pass-A partials
//   k_reg_moments<P, 1>  pass B: the metric's sums about the centroids
//   k_reg_solve<P>       the metric's solver, stats, pose <- delta o pose
//
// A metric is a policy struct P:
//   kU                queries in flight per lane
//   kNA, kNB, kRow    sums of pass A and of pass B, doubles per partial row.
//                     Pass A's sums are n, 3 * kCentroids coordinate sums, any
//                     further sums, and the count of bad indices last.
//   kCentroids        centroids the finish kernel divides by n. The finish
//                     record is pass A's sums with those divided.
//   kStats            doubles of the step's statistics
//   kPart, kOut       workspace slots of the partial rows and of the ICP
//                     loop's scratch delta and stats
//   kRegion           name of the timed region
//   In                the kernel's inputs: src, tgt, idx, dist, mask, nq, nt,
//                     stride, max_dist and the metric's own, with
//                     has_target(), gates_are_numbers() and no_target(p)
//                     (every target array <- p)
//   Pair              what a query in flight holds
//   gather<PASS>      loads a Pair; accept: the metric's own condition on it
//   add_a, add_b      one accepted Pair into the sums of pass A / pass B
//   solve             the finish record and pass B's sums to delta and stats
//   upload_target     In's target arrays from the host to the device
#pragma once

namespace nv {
namespace {

constexpr int kRegBlock = kRedBlock;  // 4 waves, one per SIMD
constexpr int kRegMaxGrid = 1024;     // 4 blocks (16 waves) on each of the 256 CUs

template <int U>
struct Gated {
  size_t qq[U];  // the query, clamped into [0, nq)
  int j[U];      // its slot-0 neighbour, or 0 when rejected
  bool ok[U], bad[U];
};

// The gate on the U queries of a lane. A query is accepted when its slot-0
// neighbour j is a target index, its distance passes the gate (a NaN fails
// `<=`) and its mask is set. A rejected query's j is replaced by 0 before any
// gather, so an index outside the cloud is counted (bad, pass A) and never
// dereferenced. Every load of a phase is issued before the first is consumed:
// no branch inside a phase (the mask test is uniform and outside the loops).
template <int U, class In>
__device__ __forceinline__ void gate(const In &a, size_t q0, Gated<U> &g) {
  int j[U], mk[U];
  double d[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const size_t q = q0 + (size_t)u * kRegBlock;
    g.qq[u] = q < a.nq ? q : a.nq - 1;  // called with nq > 0
    j[u] = a.idx[g.qq[u] * a.stride];
    d[u] = a.dist[g.qq[u] * a.stride];
    mk[u] = 1;
  }
  if (a.mask) {
#pragma unroll
    for (int u = 0; u < U; ++u) mk[u] = a.mask[g.qq[u]];
  }
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const bool in = q0 + (size_t)u * kRegBlock < a.nq;
    const int jj = j[u];
    g.ok[u] = in & (jj >= 0) & (jj < a.nt) & (d[u] <= a.max_dist) & (mk[u] != 0);
    g.bad[u] = in & ((jj < -1) | (jj >= a.nt));
    g.j[u] = g.ok[u] ? jj : 0;
  }
}

// One pass over the queries: gate, gather, accumulate, one partial row.
template <class P, int PASS>
__global__ __launch_bounds__(kRegBlock) void k_reg_moments(typename P::In a,
                                                           const double *__restrict__ cent,
                                                           double *__restrict__ part) {
  constexpr int NV = PASS ? P::kNB : P::kNA;
  constexpr int kTile = kRegBlock * P::kU;  // queries per block and trip
  double acc[NV];
#pragma unroll
  for (int k = 0; k < NV; ++k) acc[k] = 0.0;
  double c[3 * P::kCentroids];
#pragma unroll
  for (int i = 0; i < 3 * P::kCentroids; ++i) c[i] = PASS ? cent[1 + i] : 0.0;
  const size_t ntile = (a.nq + kTile - 1) / kTile;
  for (size_t tile = blockIdx.x; tile < ntile; tile += gridDim.x) {
    Gated<P::kU> g;
    gate(a, tile * kTile + threadIdx.x, g);  // ntile > 0 implies nq > 0
    typename P::Pair pr[P::kU];
#pragma unroll
    for (int u = 0; u < P::kU; ++u) P::template gather<PASS>(a, g.qq[u], g.j[u], pr[u]);
#pragma unroll
    for (int u = 0; u < P::kU; ++u) {
      const bool take = g.ok[u] & P::accept(a, pr[u]);
      if constexpr (PASS == 0) {
        if (g.bad[u]) acc[P::kNA - 1] += 1.0;
        if (take) P::add_a(pr[u], acc);
      } else {
        if (take) P::add_b(pr[u], c, acc);
      }
    }
  }
  block_sum<NV>(acc, part + (size_t)blockIdx.x * P::kRow);
}

template <class P>
__global__ __launch_bounds__(kRegBlock) void k_reg_finish(const double *__restrict__ partA,
                                                          int nblk, double *__restrict__ cent) {
  __shared__ double o[P::kNA];
  combine_rows<P::kNA, P::kRow>(partA, nblk, o);
  if (threadIdx.x == 0) {
    const double n = o[0];
    cent[0] = n;
    for (int i = 1; i <= 3 * P::kCentroids; ++i) cent[i] = n > 0.0 ? o[i] / n : 0.0;
    for (int i = 3 * P::kCentroids + 1; i < P::kNA; ++i) cent[i] = o[i];
  }
}

template <class P>
__global__ __launch_bounds__(kRegBlock) void k_reg_solve(const double *__restrict__ partB,
                                                         int nblk,
                                                         const double *__restrict__ cent,
                                                         double *__restrict__ delta,
                                                         double *__restrict__ stats,
                                                         double *pose, double *hist) {
  __shared__ double o[P::kNB];
  combine_rows<P::kNB, P::kRow>(partB, nblk, o);
  if (threadIdx.x != 0) return;
  double d[12], st[P::kStats];
  P::solve(cent, o, d, st);
  for (int i = 0; i < 12; ++i) delta[i] = d[i];
  for (int i = 0; i < P::kStats; ++i) stats[i] = st[i];
  if (pose) {
    double Q[12];
    for (int i = 0; i < 12; ++i) Q[i] = pose[i];
    pose_compose(d, Q);
    for (int i = 0; i < 12; ++i) pose[i] = Q[i];
    if (hist)
      for (int i = 0; i < 12; ++i) hist[i] = Q[i];
  }
}

// One step on device pointers: delta[12], stats[P::kStats], pose (nullable)
// <- delta o pose, and hist (nullable) also receives the composed pose.
// in.nt is (int)nt.
template <class P>
int step_run(navgpu_ctx *ctx, typename P::In in, size_t nt, double *delta, double *pose,
             double *stats, double *hist) {
  ARG_CHECK(ctx && delta && stats);
  ARG_CHECK(in.stride >= 1 && in.stride <= 16);
  ARG_CHECK(in.gates_are_numbers());  // not a NaN
  ARG_CHECK(in.nq < (size_t)INT32_MAX && nt < (size_t)INT32_MAX);
  ARG_CHECK(in.nq == 0 || (in.src && in.idx && in.dist));
  ARG_CHECK(nt == 0 || in.has_target());
  // workspace of one step: pass-A rows, pass-B rows, the finish record
  constexpr size_t kRows = (size_t)kRegMaxGrid * P::kRow;
  double *part;
  RC(ws(ctx, P::kPart, 2 * kRows + P::kRow, &part));
  double *partA = part, *partB = part + kRows, *cent = partB + kRows;
  // an empty target accepts nothing, and j = 0 then reads the workspace
  if (!nt) in.no_target(part);
  const unsigned grid = det_grid(in.nq, kRegBlock * P::kU, kRegMaxGrid);
  hipStream_t s = ctx->stream;
  TimedRegion tr(ctx, P::kRegion);
  hipLaunchKernelGGL((k_reg_moments<P, 0>), dim3(grid), dim3(kRegBlock), 0, s, in,
                     (const double *)nullptr, partA);
  CHECK_LAUNCH("k_reg_moments<0>");
  hipLaunchKernelGGL(k_reg_finish<P>, dim3(1), dim3(kRegBlock), 0, s, (const double *)partA,
                     (int)grid, cent);
  CHECK_LAUNCH("k_reg_finish");
  hipLaunchKernelGGL((k_reg_moments<P, 1>), dim3(grid), dim3(kRegBlock), 0, s, in,
                     (const double *)cent, partB);
  CHECK_LAUNCH("k_reg_moments<1>");
  hipLaunchKernelGGL(k_reg_solve<P>, dim3(1), dim3(kRegBlock), 0, s, (const double *)partB,
                     (int)grid, (const double *)cent, delta, stats, pose, hist);
  CHECK_LAUNCH("k_reg_solve");
  return NAVGPU_OK;
}

// The ICP loop on device pointers: `iters` times transform in.src by pose,
// its 1-NN in the target, one step. in.idx and in.dist are not read.
template <class P>
int icp_run(navgpu_ctx *ctx, typename P::In in, size_t nt, int iters, double *pose,
            double *hist, double *stats) {
  ARG_CHECK(ctx && pose);
  ARG_CHECK(iters >= 1 && iters <= 64);
  // navgpu_knn_dev's range
  ARG_CHECK(in.nq < (size_t)INT32_MAX / 2 && nt < (size_t)INT32_MAX / 2);
  ARG_CHECK(in.nq == 0 || in.src);
  ARG_CHECK(nt == 0 || in.has_target());
  const double *src = in.src;
  const size_t nq = in.nq;
  double *cur, *nnd, *scratch;
  int32_t *nni;
  RC(ws(ctx, kIcpCur, 3 * std::max<size_t>(nq, 1), &cur));
  RC(ws(ctx, kIcpIdx, std::max<size_t>(nq, 1), &nni));
  RC(ws(ctx, kIcpDist, std::max<size_t>(nq, 1), &nnd));
  RC(ws(ctx, P::kOut, 12 + P::kStats, &scratch));
  in.src = cur;
  in.idx = nni;
  in.dist = nnd;
  in.stride = 1;
  for (int i = 0; i < iters; ++i) {
    {
      TimedRegion tr(ctx, "icp_transform");
      RC(transform_pose_run(ctx, src, nq, pose, cur));
    }
    RC(navgpu_knn_dev(ctx, in.tgt, nt, cur, nq, 1, nni, nnd));
    RC(step_run<P>(ctx, in, nt, scratch, pose,
                   stats ? stats + P::kStats * (size_t)i : scratch + 12,
                   hist ? hist + 12 * (size_t)i : nullptr));
  }
  return NAVGPU_OK;
}

// ------------------------------------------------------------ host staging
// host arrays onto the context's stream; a null or empty source gives null
template <class T>
int to_dev(navgpu_ctx *ctx, int slot, const T *host, size_t count, T **dev) {
  *dev = nullptr;
  if (!host || !count) return NAVGPU_OK;
  RC(ws(ctx, slot, count, dev));
  HIP_TRY(hipMemcpyAsync(*dev, host, count * sizeof(T), hipMemcpyHostToDevice, ctx->stream));
  return NAVGPU_OK;
}

// in's src, idx, dist and mask from the host to the device
template <class In>
int upload_queries(navgpu_ctx *ctx, In &in) {
  double *ds, *dd;
  int32_t *di, *dm;
  RC(to_dev(ctx, kH0, in.src, 3 * in.nq, &ds));
  RC(to_dev(ctx, kH2, in.idx, in.nq * in.stride, &di));
  RC(to_dev(ctx, kH3, in.dist, in.nq * in.stride, &dd));
  RC(to_dev(ctx, kH4, in.mask, in.nq, &dm));
  in.src = ds;
  in.idx = di;
  in.dist = dd;
  in.mask = dm;
  return NAVGPU_OK;
}

// one step on host arrays, its delta and stats back on the host
template <class P>
int step_host(navgpu_ctx *ctx, typename P::In in, size_t nt, double Rm[9], double t[3],
              double *stats) {
  ARG_CHECK(ctx && Rm && t && stats);
  ARG_CHECK(in.stride >= 1 && in.stride <= 16);
  ARG_CHECK(in.nq == 0 || (in.src && in.idx && in.dist));
  ARG_CHECK(nt == 0 || in.has_target());
  RC(upload_queries(ctx, in));
  RC(P::upload_target(ctx, in, nt));
  double *dout, out[12 + P::kStats];
  RC(ws(ctx, kH5, 12 + P::kStats, &dout));
  RC(step_run<P>(ctx, in, nt, dout, nullptr, dout + 12, nullptr));
  HIP_TRY(hipMemcpyAsync(out, dout, sizeof(out), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  memcpy(Rm, out, 9 * sizeof(double));
  memcpy(t, out + 9, 3 * sizeof(double));
  memcpy(stats, out + 12, P::kStats * sizeof(double));
  return NAVGPU_OK;
}

// the ICP loop on uploaded clouds, its results back on the host
template <class P>
int icp_finish_host(navgpu_ctx *ctx, const typename P::In &in, size_t nt, int iters,
                    double pose[12], double *hist, double *stats) {
  hipStream_t s = ctx->stream;
  double *dout;  // pose[12], hist[iters][12], stats[iters][P::kStats]
  RC(ws(ctx, kH5, 12 + (12 + P::kStats) * (size_t)iters, &dout));
  double *dhist = dout + 12, *dstats = dhist + 12 * (size_t)iters;
  HIP_TRY(hipMemcpyAsync(dout, pose, 12 * sizeof(double), hipMemcpyHostToDevice, s));
  RC(icp_run<P>(ctx, in, nt, iters, dout, dhist, dstats));
  HIP_TRY(hipMemcpyAsync(pose, dout, 12 * sizeof(double), hipMemcpyDeviceToHost, s));
  if (hist)
    HIP_TRY(hipMemcpyAsync(hist, dhist, 12 * sizeof(double) * iters, hipMemcpyDeviceToHost, s));
  if (stats)
    HIP_TRY(hipMemcpyAsync(stats, dstats, P::kStats * sizeof(double) * iters,
                           hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  return in.nq ? navgpu_knn_check(ctx) : NAVGPU_OK;
}

}  // namespace
}  // namespace nv
