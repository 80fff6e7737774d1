// det_reduce.h — the reproducible f64 reductions of align.hip and plane.hip
// (DESIGN.md §10 "Determinism"): per-thread accumulators, a fixed butterfly
// per wave, the waves of a block added in wave order, one partial row per
// block, the rows added in a fixed order. No floating-point atomics. Device
// code for blocks of kRedBlock threads; internal, included after
// navgpu_common.h.
#pragma once

namespace {

constexpr int kRedBlock = 256;  // 4 waves, one per SIMD
constexpr int kRedWaves = kRedBlock / kWave;

// all 64 lanes end with the same sum, added in the same order every run
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = kWave / 2; o; o >>= 1) v += __shfl_xor(v, o, kWave);
  return v;
}

// the block's sum of each of acc[0..NV): out[k] (LDS or global) by thread k
template <int NV>
__device__ __forceinline__ void block_sum(double (&acc)[NV], double *out) {
  __shared__ double sh[kRedWaves][NV];
  const int lane = threadIdx.x & (kWave - 1), wid = threadIdx.x / kWave;
#pragma unroll
  for (int k = 0; k < NV; ++k) acc[k] = wave_sum(acc[k]);
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < NV; ++k) sh[wid][k] = acc[k];
  }
  __syncthreads();
  if (threadIdx.x < NV) {
    double s = sh[0][threadIdx.x];
    for (int w = 1; w < kRedWaves; ++w) s += sh[w][threadIdx.x];
    out[threadIdx.x] = s;
  }
}

// the sum over the nblk partial rows of ROW doubles, in a fixed order: thread
// t adds rows t, t + 256, ... ascending, then the block's fixed tree; out:
// LDS, NV doubles
template <int NV, int ROW>
__device__ __forceinline__ void combine_rows(const double *__restrict__ part, int nblk,
                                             double *out) {
  double acc[NV];
#pragma unroll
  for (int k = 0; k < NV; ++k) acc[k] = 0.0;
  for (int r = threadIdx.x; r < nblk; r += kRedBlock) {
#pragma unroll
    for (int k = 0; k < NV; ++k) acc[k] += part[(size_t)r * ROW + k];
  }
  block_sum<NV>(acc, out);
  __syncthreads();
}

// blocks of a launch whose blocks take `tile` queries per trip: a function of
// nq alone, so the partial rows and their order are too
inline unsigned det_grid(size_t nq, int tile, int max_grid) {
  return (unsigned)std::max<size_t>(1, std::min<size_t>(max_grid, (nq + tile - 1) / tile));
}

}  // namespace
