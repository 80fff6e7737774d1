// align.hip — 6-DOF rigid registration on the global k-NN's output: the
// point-to-point metric of the shared two-pass step (reg_step.h), whose
// closed-form pose is align_solve.h's, and a transform by a device-resident
// pose (k_transform_pose). Third translation unit of libnavgpu.so. Beyond the
// reference, whose optimiser is translation-only (src/slam.c:300-389); the
// checker is the numpy restatement in tests/reg_ref.py. DESIGN.md §10.
//
//   pass A   n, sum p, sum q, sum |q-p|^2, bad indices
//   finish   pbar, qbar from the pass-A partials
//   pass B   centred H, sum |p-pbar|^2, sum |q-qbar|^2
//   solve    Horn's closed form, stats, pose <- delta o pose
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
#include "reg_step.h"

using namespace nv;

namespace {

struct AlignIn {
  const double *src, *tgt;  // tgt is never null in a kernel (no_target)
  const int32_t *idx;
  const double *dist;
  const int32_t *mask;  // nullable
  size_t nq;
  int nt, stride;
  double max_dist;
  bool has_target() const { return tgt != nullptr; }
  bool gates_are_numbers() const { return max_dist == max_dist; }
  void no_target(const double *p) { tgt = p; }
};

struct AlignMetric {
  // Independent queries in flight per lane: the 24-B target gather is a random
  // access, so each lane issues kU of them before it consumes the first.
  static constexpr int kU = 4;
  static constexpr int kNA = 9;    // pass A: n, sum p, sum q, sum |q-p|^2, bad
  static constexpr int kNB = 11;   // pass B: H, Spp, Sqq
  static constexpr int kRow = 16;  // doubles per partial row (128 B)
  static constexpr int kCentroids = 2;  // finish record: n, pbar, qbar, sum |q-p|^2, bad
  static constexpr int kStats = 4;
  static constexpr int kPart = kAlignPart, kOut = kAlignOut;
  static constexpr const char *kRegion = "align";
  using In = AlignIn;
  struct Pair {
    double p[3], t[3];
  };

  template <int PASS>
  static __device__ __forceinline__ void gather(const In &a, size_t q, int j, Pair &g) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      g.p[c] = a.src[3 * q + c];
      g.t[c] = a.tgt[3 * (size_t)j + c];
    }
  }

  static __device__ __forceinline__ bool accept(const In &, const Pair &) { return true; }

  static __device__ __forceinline__ void add_a(const Pair &g, double (&acc)[kNA]) {
    acc[0] += 1.0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      acc[1 + c] += g.p[c];
      acc[4 + c] += g.t[c];
    }
    const double dx = g.t[0] - g.p[0], dy = g.t[1] - g.p[1], dz = g.t[2] - g.p[2];
    acc[7] += (dx * dx + dy * dy) + dz * dz;
  }

  // cen = pbar, qbar
  static __device__ __forceinline__ void add_b(const Pair &g, const double (&cen)[6],
                                               double (&acc)[kNB]) {
    double x[3], y[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      x[c] = g.p[c] - cen[c];
      y[c] = g.t[c] - cen[3 + c];
    }
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int c = 0; c < 3; ++c) acc[3 * r + c] += x[r] * y[c];
    acc[9] += (x[0] * x[0] + x[1] * x[1]) + x[2] * x[2];
    acc[10] += (y[0] * y[0] + y[1] * y[1]) + y[2] * y[2];
  }

  static __device__ void solve(const double *cent, const double *o, double d[12],
                               double st[kStats]) {
    double m[kAlignMoments];
    for (int i = 0; i < 8; ++i) m[i] = cent[i];
    for (int i = 0; i < kNB; ++i) m[8 + i] = o[i];
    m[19] = cent[8];
    align_solve(m, d, st);
  }

  static int upload_target(navgpu_ctx *ctx, In &in, size_t nt) {
    double *dt;
    RC(to_dev(ctx, kH1, in.tgt, 3 * nt, &dt));
    in.tgt = dt;
    return NAVGPU_OK;
  }
};

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

}  // namespace

int nv::transform_pose_run(navgpu_ctx *ctx, const double *pts, size_t n, const double *pose,
                           double *out) {
  if (!n) return NAVGPU_OK;
  ARG_CHECK(pts && pose && out);
  hipLaunchKernelGGL(k_transform_pose, dim3(grid1d(n, 256)), dim3(256), 0, ctx->stream, pts, n,
                     pose, out);
  CHECK_LAUNCH("k_transform_pose");
  return NAVGPU_OK;
}

extern "C" {

int navgpu_align_dev(navgpu_ctx *ctx, const double *src, size_t nq, const double *tgt, size_t nt,
                     const int32_t *idx, const double *dist, int stride, double max_dist,
                     const int32_t *mask, double *delta, double *pose, double *stats) {
  return step_run<AlignMetric>(ctx, {src, tgt, idx, dist, mask, nq, (int)nt, stride, max_dist},
                               nt, delta, pose, stats, nullptr);
}

int navgpu_align_host(navgpu_ctx *ctx, const double *src, size_t nq, const double *tgt, size_t nt,
                      const int32_t *idx, const double *dist, int stride, double max_dist,
                      const int32_t *mask, double Rm[9], double t[3], double stats[4]) {
  return step_host<AlignMetric>(ctx, {src, tgt, idx, dist, mask, nq, (int)nt, stride, max_dist},
                                nt, Rm, t, stats);
}

int navgpu_transform_pose_dev(navgpu_ctx *ctx, const double *pts, size_t n, const double *pose_dev,
                              double *out) {
  ARG_CHECK(ctx);
  return transform_pose_run(ctx, pts, n, pose_dev, out);
}

int navgpu_icp_dev(navgpu_ctx *ctx, const double *src, size_t nq, const double *tgt, size_t nt,
                   int iters, double max_dist, const int32_t *mask, double *pose, double *hist,
                   double *stats) {
  return icp_run<AlignMetric>(ctx, {src, tgt, nullptr, nullptr, mask, nq, (int)nt, 1, max_dist},
                              nt, iters, pose, hist, stats);
}

int navgpu_icp_host(navgpu_ctx *ctx, const double *src, size_t nq, const double *tgt, size_t nt,
                    int iters, double max_dist, const int32_t *mask, double pose[12], double *hist,
                    double *stats) {
  ARG_CHECK(ctx && pose);
  ARG_CHECK(iters >= 1 && iters <= 64);
  ARG_CHECK(nq == 0 || src);
  ARG_CHECK(nt == 0 || tgt);
  AlignIn in{src, tgt, nullptr, nullptr, mask, nq, (int)nt, 1, max_dist};
  RC(upload_queries(ctx, in));
  RC(AlignMetric::upload_target(ctx, in, nt));
  return icp_finish_host<AlignMetric>(ctx, in, nt, iters, pose, hist, stats);
}

}  // extern "C"
