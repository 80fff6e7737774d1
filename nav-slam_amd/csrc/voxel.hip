// voxel.hip — voxel-grid downsampling of a cloud: one output point per
// occupied cell of a regular grid, with the cell's centroid, count and centred
// covariance sums, in ascending order of the cell key. Fifth translation unit
// of libnavgpu.so. Beyond the reference, which has no such function; the
// checker is the numpy restatement in tests/voxel_ref.py. DESIGN.md §12.
//
//   k_vox_min      per-axis minimum of the finite points (no origin given)
//   k_vox_setup    the origin into stats[4..6], counters cleared
//   k_vox_keys     key of each point (voxel_key.h), dropped points counted
//   8 x { k_vox_hist, k_vox_offsets, k_vox_scatter }
//                  stable least-significant-digit radix sort of (key, index)
//   k_vox_heads, k_vox_scan_sums, k_vox_number
//                  segment heads, their scan: voxel numbers, labels, cells
//   2 x { k_vox_seg_agg, k_vox_seg_carry, k_vox_seg_out }
//                  segmented sums by sorted position: centroids, then the
//                  covariance about them
//
// Reproducible bit for bit (§10 "Determinism"): no floating-point atomics,
// integer atomics for counts only (dropped points; a tile's digits, in LDS), ranks from a stable in-block ranking, every
// floating-point sum in an order fixed by the sorted keys.
#include "navgpu_common.h"

#include "voxel_key.h"
#include "det_reduce.h"

using namespace nv;

namespace {

constexpr int kVoxBlock = 256;  // 4 waves, one per SIMD
constexpr int kVoxWaves = kVoxBlock / kWave;
constexpr int kVoxMinMaxGrid = 1024;
// radix sort: 8 passes of 8 bits over the 64-bit key (63 key bits, and the
// all-ones key of a dropped point)
constexpr int kRadixBits = 8;
constexpr int kRadix = 1 << kRadixBits;
constexpr int kRadixPasses = 64 / kRadixBits;
constexpr int kSortRounds = 4;                        // keys per thread
constexpr int kSortTile = kVoxBlock * kSortRounds;    // keys per block
constexpr int kSegTile = kVoxBlock;                   // sorted positions per block
constexpr int kAggRow = 8;                            // doubles per aggregate row: flag, <= 6 sums
static_assert(kRadix == kVoxBlock, "one thread per digit value");

// counters of a call (uint32): dropped non-finite, dropped out of range, then
// the digit totals of a pass (written by k_vox_offsets)
constexpr int kCtrTotals = 2;
constexpr int kCtrCount = kCtrTotals + kRadix;

__device__ __forceinline__ double dmin(double a, double b) { return b < a ? b : a; }

// ------------------------------------------------------------------- origin
__global__ __launch_bounds__(kVoxBlock) void k_vox_min(const double *__restrict__ pts, size_t n,
                                                       double *__restrict__ part) {
  double m[3] = {INFINITY, INFINITY, INFINITY};
  for (size_t i = (size_t)blockIdx.x * kVoxBlock + threadIdx.x; i < n;
       i += (size_t)gridDim.x * kVoxBlock) {
    const double x = pts[3 * i], y = pts[3 * i + 1], z = pts[3 * i + 2];
    if (vox_finite(x) && vox_finite(y) && vox_finite(z)) {
      m[0] = dmin(m[0], x);
      m[1] = dmin(m[1], y);
      m[2] = dmin(m[2], z);
    }
  }
  __shared__ double sh[kVoxWaves][3];
  const int lane = threadIdx.x & (kWave - 1), wid = threadIdx.x / kWave;
#pragma unroll
  for (int c = 0; c < 3; ++c)
#pragma unroll
    for (int o = kWave / 2; o; o >>= 1) m[c] = dmin(m[c], __shfl_xor(m[c], o, kWave));
  if (lane == 0)
    for (int c = 0; c < 3; ++c) sh[wid][c] = m[c];
  __syncthreads();
  if (threadIdx.x < 3) {
    double s = sh[0][threadIdx.x];
    for (int w = 1; w < kVoxWaves; ++w) s = dmin(s, sh[w][threadIdx.x]);
    part[3 * (size_t)blockIdx.x + threadIdx.x] = s;
  }
}

// One block. The origin: the given one, or the minimum over the nblk partial
// rows of k_vox_min (0 when no point is finite). Clears the counters; an empty
// cloud's stats are complete here.
__global__ __launch_bounds__(kVoxBlock) void k_vox_setup(const double *__restrict__ part, int nblk,
                                                         bool has_org, double ox, double oy,
                                                         double oz, bool empty,
                                                         double *__restrict__ stats,
                                                         uint32_t *__restrict__ ctr) {
  for (int i = threadIdx.x; i < kCtrCount; i += kVoxBlock) ctr[i] = 0u;
  double m[3] = {INFINITY, INFINITY, INFINITY};
  if (!has_org) {
    for (int r = threadIdx.x; r < nblk; r += kVoxBlock)
      for (int c = 0; c < 3; ++c) m[c] = dmin(m[c], part[3 * (size_t)r + c]);
  }
  __shared__ double sh[kVoxWaves][3];
  const int lane = threadIdx.x & (kWave - 1), wid = threadIdx.x / kWave;
#pragma unroll
  for (int c = 0; c < 3; ++c)
#pragma unroll
    for (int o = kWave / 2; o; o >>= 1) m[c] = dmin(m[c], __shfl_xor(m[c], o, kWave));
  if (lane == 0)
    for (int c = 0; c < 3; ++c) sh[wid][c] = m[c];
  __syncthreads();
  if (threadIdx.x < 3) {
    double s = sh[0][threadIdx.x];
    for (int w = 1; w < kVoxWaves; ++w) s = dmin(s, sh[w][threadIdx.x]);
    const double given = threadIdx.x == 0 ? ox : threadIdx.x == 1 ? oy : oz;
    stats[4 + threadIdx.x] = has_org ? given : (s < INFINITY ? s : 0.0);
  }
  if (empty && threadIdx.x < 4) stats[threadIdx.x] = 0.0;
}

// --------------------------------------------------------------------- keys
__global__ __launch_bounds__(kVoxBlock) void k_vox_keys(const double *__restrict__ pts, size_t n,
                                                        double voxel,
                                                        const double *__restrict__ stats,
                                                        uint64_t *__restrict__ keys,
                                                        uint32_t *__restrict__ vals,
                                                        uint32_t *__restrict__ ctr) {
  const size_t i = (size_t)blockIdx.x * kVoxBlock + threadIdx.x;
  const double o[3] = {stats[4], stats[5], stats[6]};
  int why = kVoxKept;
  if (i < n) {
    const double p[3] = {pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]};
    keys[i] = vox_key(p, o, voxel, &why);
    vals[i] = (uint32_t)i;
  }
  // counts: integer adds, the same total in any order
  const unsigned long long nf = __ballot(why == kVoxNonFinite);
  const unsigned long long oor = __ballot(why == kVoxOutOfRange);
  if ((threadIdx.x & (kWave - 1)) == 0) {
    if (nf) atomicAdd(&ctr[0], (uint32_t)__popcll(nf));
    if (oor) atomicAdd(&ctr[1], (uint32_t)__popcll(oor));
  }
}

// --------------------------------------------------------------------- sort
__device__ __forceinline__ int digit_of(uint64_t key, int shift) {
  return (int)((key >> shift) & (uint64_t)(kRadix - 1));
}

// hist[d * nblk + b] = keys of block b's tile whose digit is d
__global__ __launch_bounds__(kVoxBlock) void k_vox_hist(const uint64_t *__restrict__ keys,
                                                        size_t n, int shift,
                                                        uint32_t *__restrict__ hist) {
  __shared__ uint32_t h[kRadix];
  h[threadIdx.x] = 0u;
  __syncthreads();
  const size_t base = (size_t)blockIdx.x * kSortTile;
  const unsigned long long below = (1ull << (threadIdx.x & (kWave - 1))) - 1ull;
#pragma unroll
  for (int r = 0; r < kSortRounds; ++r) {
    const size_t p = base + (size_t)r * kVoxBlock + threadIdx.x;
    const bool in = p < n;
    const int d = in ? digit_of(keys[p], shift) : 0;
    // one add per wave and digit value, by the lowest lane that holds it:
    // the high digits are the same in most keys, and 64 adds to one LDS
    // address would run one after another
    unsigned long long same = __ballot(in);
#pragma unroll
    for (int b = 0; b < kRadixBits; ++b) {
      const bool bit = (d >> b) & 1;
      const unsigned long long m = __ballot(bit);
      same &= bit ? m : ~m;
    }
    if (in && (same & below) == 0ull) atomicAdd(&h[d], (uint32_t)__popcll(same));
  }
  __syncthreads();
  hist[(size_t)threadIdx.x * gridDim.x + blockIdx.x] = h[threadIdx.x];
}

// Block d: hist[d * nblk + b] <- keys with digit d in blocks before b, and
// totals[d] <- keys with digit d (no atomic: the row's own sum).
__global__ __launch_bounds__(kVoxBlock) void k_vox_offsets(uint32_t *__restrict__ hist, int nblk,
                                                           uint32_t *__restrict__ totals) {
  __shared__ int scratch[kVoxWaves + 1];
  int carry = 0;
  uint32_t *row = hist + (size_t)blockIdx.x * nblk;
  for (int b0 = 0; b0 < nblk; b0 += kVoxBlock) {
    const int b = b0 + threadIdx.x;
    const int v = b < nblk ? (int)row[b] : 0;
    int total;
    const int ex = block_excl_scan(v, scratch, &total);
    if (b < nblk) row[b] = (uint32_t)(carry + ex);
    carry += total;
  }
  if (threadIdx.x == 0) totals[blockIdx.x] = (uint32_t)carry;
}

// One tile of kSortTile keys per block, wave w the 256 consecutive keys from
// w * 256, 64 at a time: a key's rank among the tile's keys of its digit is
// the count in earlier waves, in earlier rounds of its wave, and in lower
// lanes of its round (a ballot per digit bit), so equal digits keep their
// order: the sort is stable. No atomic counter. Where the tile's first key of
// digit d goes: the keys with a smaller digit (a scan of totals, thread =
// digit) and those with digit d in earlier blocks (hist).
__global__ __launch_bounds__(kVoxBlock) void k_vox_scatter(
    const uint64_t *__restrict__ keys, const uint32_t *__restrict__ vals,
    uint64_t *__restrict__ keys_out, uint32_t *__restrict__ vals_out, size_t n, int shift,
    const uint32_t *__restrict__ hist, const uint32_t *__restrict__ totals) {
  __shared__ uint32_t run[kVoxWaves][kRadix];
  __shared__ int scratch[kVoxWaves + 1];
  const int lane = threadIdx.x & (kWave - 1), wid = threadIdx.x / kWave;
#pragma unroll
  for (int w = 0; w < kVoxWaves; ++w) run[w][threadIdx.x] = 0u;
  __syncthreads();
  const size_t base = (size_t)blockIdx.x * kSortTile + (size_t)wid * (kSortRounds * kWave) + lane;
  uint64_t key[kSortRounds];
  uint32_t val[kSortRounds], rank[kSortRounds];
  bool in[kSortRounds];
#pragma unroll
  for (int r = 0; r < kSortRounds; ++r) {
    const size_t p = base + (size_t)r * kWave;
    in[r] = p < n;
    key[r] = in[r] ? keys[p] : kVoxNoKey;
    val[r] = in[r] ? vals[p] : 0u;
  }
  const unsigned long long below = (1ull << lane) - 1ull;
#pragma unroll
  for (int r = 0; r < kSortRounds; ++r) {
    const int d = digit_of(key[r], shift);
    unsigned long long same = __ballot(in[r]);
#pragma unroll
    for (int b = 0; b < kRadixBits; ++b) {
      const bool bit = (d >> b) & 1;
      const unsigned long long m = __ballot(bit);
      same &= bit ? m : ~m;
    }
    const uint32_t before = (uint32_t)__popcll(same & below);
    rank[r] = run[wid][d] + before;
    wave_sync_mem();
    if (in[r] && before == 0u) run[wid][d] += (uint32_t)__popcll(same);
    wave_sync_mem();
  }
  int total;
  const int smaller = block_excl_scan((int)totals[threadIdx.x], scratch, &total);
  {
    // thread = digit: the waves' counts to their starts
    uint32_t at = (uint32_t)smaller + hist[(size_t)threadIdx.x * gridDim.x + blockIdx.x];
#pragma unroll
    for (int w = 0; w < kVoxWaves; ++w) {
      const uint32_t c = run[w][threadIdx.x];
      run[w][threadIdx.x] = at;
      at += c;
    }
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < kSortRounds; ++r) {
    const size_t dst = (size_t)run[wid][digit_of(key[r], shift)] + rank[r];
    if (in[r] && dst < n) {  // dst < n by construction; the test costs nothing
      keys_out[dst] = key[r];
      vals_out[dst] = val[r];
    }
  }
}

// ----------------------------------------------------------- voxel numbering
// sorted position p is kept when its key is one, and a head when it is the
// first of its key
__device__ __forceinline__ void seg_flags(const uint64_t *__restrict__ keys, size_t n, size_t p,
                                          uint64_t &key, bool &kept, bool &head) {
  key = p < n ? keys[p] : kVoxNoKey;
  kept = key != kVoxNoKey;
  head = kept && (p == 0 || keys[p - 1] != key);
}

__global__ __launch_bounds__(kVoxBlock) void k_vox_heads(const uint64_t *__restrict__ keys,
                                                         size_t n, int32_t *__restrict__ bsum) {
  __shared__ int scratch[kVoxWaves + 1];
  uint64_t key;
  bool kept, head;
  seg_flags(keys, n, (size_t)blockIdx.x * kSegTile + threadIdx.x, key, kept, head);
  int total;
  block_excl_scan(head ? 1 : 0, scratch, &total);
  if (threadIdx.x == 0) bsum[blockIdx.x] = total;
}

// One block: bsum <- its exclusive scan; the call's stats[0..3]. Thread t takes
// the ceil(nsb / 256) consecutive entries from t times that: its sum, one
// block scan of the 256 sums, its entries again.
__global__ __launch_bounds__(kVoxBlock) void k_vox_scan_sums(int32_t *__restrict__ bsum, int nsb,
                                                             size_t n,
                                                             const uint32_t *__restrict__ ctr,
                                                             double *__restrict__ stats) {
  __shared__ int scratch[kVoxWaves + 1];
  const int per = (nsb + kVoxBlock - 1) / kVoxBlock;
  const int b0 = min(nsb, (int)threadIdx.x * per), b1 = min(nsb, b0 + per);
  int sum = 0;
  for (int b = b0; b < b1; ++b) sum += bsum[b];
  int total;
  int at = block_excl_scan(sum, scratch, &total);
  for (int b = b0; b < b1; ++b) {
    const int v = bsum[b];
    bsum[b] = at;
    at += v;
  }
  if (threadIdx.x == 0) {
    const double nf = (double)ctr[0], oor = (double)ctr[1];
    stats[0] = (double)total;
    stats[1] = ((double)n - nf) - oor;
    stats[2] = nf;
    stats[3] = oor;
  }
}

// vox[p], the voxel of sorted position p (-1: dropped); seg[j], where voxel j
// starts; labels and cells. Voxels numbered cap and above are written to the
// workspace (vox, seg) and to labels only.
__global__ __launch_bounds__(kVoxBlock) void k_vox_number(
    const uint64_t *__restrict__ keys, const uint32_t *__restrict__ vals, size_t n,
    const int32_t *__restrict__ bsum, size_t cap, int32_t *__restrict__ vox,
    int32_t *__restrict__ seg, int32_t *__restrict__ labels, int32_t *__restrict__ cells) {
  __shared__ int scratch[kVoxWaves + 1];
  const size_t p = (size_t)blockIdx.x * kSegTile + threadIdx.x;
  uint64_t key;
  bool kept, head;
  seg_flags(keys, n, p, key, kept, head);
  int total;
  const int ex = block_excl_scan(head ? 1 : 0, scratch, &total);
  if (p >= n) return;
  const int j = kept ? bsum[blockIdx.x] + ex + (head ? 1 : 0) - 1 : -1;
  vox[p] = j;
  if (labels) {
    const uint32_t i = vals[p];
    if (i < n) labels[i] = j;
  }
  if (head) {
    seg[j] = (int32_t)p;  // j < n: seg holds n entries
    if (cells && (size_t)j < cap) {
      int32_t c[3];
      vox_unpack(key, c);
      cells[3 * (size_t)j] = c[0];
      cells[3 * (size_t)j + 1] = c[1];
      cells[3 * (size_t)j + 2] = c[2];
    }
  }
}

// --------------------------------------------------------- segmented sums
// Inclusive segmented scan of v over the block's threads in thread order, a
// carry (the open segment's sum so far) entering thread 0. f: this thread
// starts a segment; on return: a segment starts at or before this thread in
// the block. The order of the additions is fixed: the shifts of a wave, then
// the waves before it in wave order, then the carry first of all.
template <int NV>
__device__ __forceinline__ void block_seg_scan(double (&v)[NV], bool &f, const double (&carry)[NV],
                                               double (*sh_v)[NV], int *sh_f) {
  const int lane = threadIdx.x & (kWave - 1), wid = threadIdx.x / kWave;
  int fl = f ? 1 : 0;
#pragma unroll
  for (int o = 1; o < kWave; o <<= 1) {
    const int tf = __shfl_up(fl, o, kWave);
    double tv[NV];
#pragma unroll
    for (int k = 0; k < NV; ++k) tv[k] = __shfl_up(v[k], o, kWave);
    if (lane >= o) {
      if (!fl) {
#pragma unroll
        for (int k = 0; k < NV; ++k) v[k] = tv[k] + v[k];
      }
      fl |= tf;
    }
  }
  if (lane == kWave - 1) {
#pragma unroll
    for (int k = 0; k < NV; ++k) sh_v[wid][k] = v[k];
    sh_f[wid] = fl;
  }
  __syncthreads();
  double c[NV];
#pragma unroll
  for (int k = 0; k < NV; ++k) c[k] = carry[k];
  int cf = 0;
#pragma unroll
  for (int w = 0; w < kVoxWaves - 1; ++w) {
    if (w < wid) {
      const int wf = sh_f[w];
#pragma unroll
      for (int k = 0; k < NV; ++k) c[k] = wf ? sh_v[w][k] : c[k] + sh_v[w][k];
      cf |= wf;
    }
  }
  if (!fl) {
#pragma unroll
    for (int k = 0; k < NV; ++k) v[k] = c[k] + v[k];
  }
  f = (fl | cf) != 0;
  __syncthreads();
}

struct SegIn {
  const double *pts;
  const uint64_t *keys;
  const uint32_t *vals;
  const int32_t *vox;
  const double *cent;  // the centroid of every voxel (workspace), pass 1
  size_t n;
};

// The term of sorted position p: pass 0 the point, pass 1 the products of its
// offsets from its voxel's centroid (xx, xy, xz, yy, yz, zz). A dropped
// position is a segment of its own with the sum 0.
template <int PASS, int NV>
__device__ __forceinline__ void seg_term(const SegIn &a, size_t p, double (&v)[NV], bool &kept,
                                         bool &head, uint64_t &key) {
  seg_flags(a.keys, a.n, p, key, kept, head);
#pragma unroll
  for (int k = 0; k < NV; ++k) v[k] = 0.0;
  if (!kept) return;
  uint32_t i = a.vals[p];
  i = i < a.n ? i : 0u;
  const double x = a.pts[3 * (size_t)i], y = a.pts[3 * (size_t)i + 1], z = a.pts[3 * (size_t)i + 2];
  if constexpr (PASS == 0) {
    v[0] = x;
    v[1] = y;
    v[2] = z;
  } else {
    const size_t j = (size_t)a.vox[p];
    const double dx = x - a.cent[3 * j], dy = y - a.cent[3 * j + 1], dz = z - a.cent[3 * j + 2];
    v[0] = dx * dx;
    v[1] = dx * dy;
    v[2] = dx * dz;
    v[3] = dy * dy;
    v[4] = dy * dz;
    v[5] = dz * dz;
  }
}

// the block's aggregate: whether a segment starts in it, and the sum of its
// last (open) segment
template <int PASS>
__global__ __launch_bounds__(kVoxBlock) void k_vox_seg_agg(SegIn a, double *__restrict__ agg) {
  constexpr int NV = PASS ? 6 : 3;
  __shared__ double sh_v[kVoxWaves][NV];
  __shared__ int sh_f[kVoxWaves];
  double v[NV], zero[NV];
  bool kept, head;
  uint64_t key;
  seg_term<PASS, NV>(a, (size_t)blockIdx.x * kSegTile + threadIdx.x, v, kept, head, key);
#pragma unroll
  for (int k = 0; k < NV; ++k) zero[k] = 0.0;
  bool f = head || !kept;
  block_seg_scan<NV>(v, f, zero, sh_v, sh_f);
  if (threadIdx.x == kVoxBlock - 1) {
    double *row = agg + (size_t)blockIdx.x * kAggRow;
    row[0] = f ? 1.0 : 0.0;
#pragma unroll
    for (int k = 0; k < NV; ++k) row[1 + k] = v[k];
  }
}

// One block: carry[b] (a row of kAggRow doubles, the sums from [1]) = the sum
// of the segment open at the start of block b, from the aggregates before it.
// Thread t takes the ceil(nsb / 256) consecutive rows from t times that: their
// aggregate, one block scan of the 256 aggregates, the rows again.
template <int NV>
__global__ __launch_bounds__(kVoxBlock) void k_vox_seg_carry(const double *__restrict__ agg,
                                                             int nsb, double *__restrict__ carry) {
  __shared__ double sh_v[kVoxWaves][NV];
  __shared__ int sh_f[kVoxWaves];
  __shared__ double incl[kVoxBlock][NV];
  const int per = (nsb + kVoxBlock - 1) / kVoxBlock;
  const int b0 = min(nsb, (int)threadIdx.x * per), b1 = min(nsb, b0 + per);
  double v[NV], zero[NV];
#pragma unroll
  for (int k = 0; k < NV; ++k) v[k] = zero[k] = 0.0;
  bool f = false;
#pragma unroll 4
  for (int b = b0; b < b1; ++b) {
    const double *row = agg + (size_t)b * kAggRow;
    const bool fb = row[0] != 0.0;
#pragma unroll
    for (int k = 0; k < NV; ++k) v[k] = fb ? row[1 + k] : v[k] + row[1 + k];
    f |= fb;
  }
  block_seg_scan<NV>(v, f, zero, sh_v, sh_f);
#pragma unroll
  for (int k = 0; k < NV; ++k) incl[threadIdx.x][k] = v[k];
  __syncthreads();
  double c[NV];
#pragma unroll
  for (int k = 0; k < NV; ++k) c[k] = threadIdx.x ? incl[threadIdx.x - 1][k] : 0.0;
#pragma unroll 4
  for (int b = b0; b < b1; ++b) {
    const double *row = agg + (size_t)b * kAggRow;
    double *out = carry + (size_t)b * kAggRow;
    const bool fb = row[0] != 0.0;
#pragma unroll
    for (int k = 0; k < NV; ++k) {
      out[1 + k] = c[k];
      c[k] = fb ? row[1 + k] : c[k] + row[1 + k];
    }
  }
}

// The scan again with the carry; the last position of a voxel holds its sums.
// Pass 0: centroid = sum / count into the workspace (every voxel) and, below
// cap, into centroids and counts. Pass 1: the sums into cov below cap.
template <int PASS>
__global__ __launch_bounds__(kVoxBlock) void k_vox_seg_out(SegIn a, const double *__restrict__ carry,
                                                           const int32_t *__restrict__ seg,
                                                           size_t cap, double *__restrict__ cent_ws,
                                                           double *__restrict__ out,
                                                           int32_t *__restrict__ counts) {
  constexpr int NV = PASS ? 6 : 3;
  __shared__ double sh_v[kVoxWaves][NV];
  __shared__ int sh_f[kVoxWaves];
  const size_t p = (size_t)blockIdx.x * kSegTile + threadIdx.x;
  double v[NV], c[NV];
  bool kept, head;
  uint64_t key;
  seg_term<PASS, NV>(a, p, v, kept, head, key);
#pragma unroll
  for (int k = 0; k < NV; ++k) c[k] = carry[(size_t)blockIdx.x * kAggRow + 1 + k];
  bool f = head || !kept;
  block_seg_scan<NV>(v, f, c, sh_v, sh_f);
  if (!kept) return;
  if (p + 1 < a.n && a.keys[p + 1] == key) return;  // not the last of its voxel
  const size_t j = (size_t)a.vox[p];
  if constexpr (PASS == 0) {
    const int32_t m = (int32_t)(p + 1) - seg[j];
    const double dm = (double)m;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const double ck = v[k] / dm;
      cent_ws[3 * j + k] = ck;
      if (j < cap) out[3 * j + k] = ck;
    }
    if (counts && j < cap) counts[j] = m;
  } else {
    if (j < cap) {
#pragma unroll
      for (int k = 0; k < 6; ++k) out[6 * j + k] = v[k];
    }
  }
}

// ------------------------------------------------------------------- driver
// a host array onto the context's stream; an empty one gives null
int cloud_to_dev(navgpu_ctx *ctx, int slot, const double *host, size_t count, double **dev) {
  *dev = nullptr;
  if (!host || !count) return NAVGPU_OK;
  RC(ws(ctx, slot, count, dev));
  HIP_TRY(hipMemcpyAsync(*dev, host, count * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  return NAVGPU_OK;
}

int voxel_check(navgpu_ctx *ctx, size_t n, double voxel, const double *origin) {
  ARG_CHECK(ctx);
  ARG_CHECK(vox_voxel_ok(voxel));
  ARG_CHECK(vox_origin_ok(origin));
  if (n >= (size_t)1 << 31) {
    set_err("voxel_downsample: n = %zu is not below 2^31", n);
    return NAVGPU_ERANGE;
  }
  return NAVGPU_OK;
}

template <int PASS>
int seg_sums_run(navgpu_ctx *ctx, const SegIn &in, unsigned nsb, double *agg, double *carry,
                 const int32_t *seg, size_t cap, double *cent_ws, double *out, int32_t *counts) {
  constexpr int NV = PASS ? 6 : 3;
  hipStream_t s = ctx->stream;
  hipLaunchKernelGGL(k_vox_seg_agg<PASS>, dim3(nsb), dim3(kVoxBlock), 0, s, in, agg);
  CHECK_LAUNCH("k_vox_seg_agg");
  hipLaunchKernelGGL(k_vox_seg_carry<NV>, dim3(1), dim3(kVoxBlock), 0, s, (const double *)agg,
                     (int)nsb, carry);
  CHECK_LAUNCH("k_vox_seg_carry");
  hipLaunchKernelGGL(k_vox_seg_out<PASS>, dim3(nsb), dim3(kVoxBlock), 0, s, in,
                     (const double *)carry, seg, cap, cent_ws, out, counts);
  CHECK_LAUNCH("k_vox_seg_out");
  return NAVGPU_OK;
}

int voxel_run(navgpu_ctx *ctx, const double *pts, size_t n, double voxel, const double *origin,
              size_t cap, double *centroids, int32_t *counts, double *cov, int32_t *cells,
              int32_t *labels, double *stats) {
  RC(voxel_check(ctx, n, voxel, origin));
  ARG_CHECK(stats);
  ARG_CHECK(n == 0 || pts);
  ARG_CHECK(cap == 0 || centroids);
  const bool has_org = origin != nullptr;
  const double ox = has_org ? origin[0] : 0.0, oy = has_org ? origin[1] : 0.0,
               oz = has_org ? origin[2] : 0.0;
  const unsigned nmin = det_grid(n, kVoxBlock, kVoxMinMaxGrid);
  const unsigned nkb = grid1d(n, kVoxBlock);   // blocks of the key kernel
  const unsigned nrb = grid1d(n, kSortTile);   // blocks (tiles) of the sort
  const unsigned nsb = grid1d(n, kSegTile);    // blocks of the segmented sums
  const size_t n1 = std::max<size_t>(n, 1);
  uint64_t *keys;
  uint32_t *vals, *ctr;
  int32_t *num;
  double *part, *cent_ws;
  RC(ws(ctx, kVoxKeys, 2 * n1, &keys));
  RC(ws(ctx, kVoxVals, 2 * n1, &vals));
  RC(ws(ctx, kVoxHist, (size_t)kCtrCount + (size_t)kRadix * std::max(nrb, 1u), &ctr));
  RC(ws(ctx, kVoxNum, 2 * n1 + nsb + 1, &num));
  RC(ws(ctx, kVoxPart, 3 * (size_t)kVoxMinMaxGrid + 2 * ((size_t)nsb + 1) * kAggRow, &part));
  RC(ws(ctx, kVoxCent, 3 * n1, &cent_ws));
  uint32_t *totals = ctr + kCtrTotals, *hist = ctr + kCtrCount;
  int32_t *vox = num, *seg = num + n1, *bsum = num + 2 * n1;
  double *agg = part + 3 * (size_t)kVoxMinMaxGrid, *carry = agg + ((size_t)nsb + 1) * kAggRow;
  hipStream_t s = ctx->stream;
  TimedRegion tr(ctx, "voxel");
  if (!has_org && n) {
    hipLaunchKernelGGL(k_vox_min, dim3(nmin), dim3(kVoxBlock), 0, s, pts, n, part);
    CHECK_LAUNCH("k_vox_min");
  }
  hipLaunchKernelGGL(k_vox_setup, dim3(1), dim3(kVoxBlock), 0, s, (const double *)part,
                     n ? (int)nmin : 0, has_org, ox, oy, oz, n == 0, stats, ctr);
  CHECK_LAUNCH("k_vox_setup");
  if (!n) return NAVGPU_OK;
  hipLaunchKernelGGL(k_vox_keys, dim3(nkb), dim3(kVoxBlock), 0, s, pts, n, voxel,
                     (const double *)stats, keys, vals, ctr);
  CHECK_LAUNCH("k_vox_keys");
  uint64_t *ka = keys, *kb = keys + n1;
  uint32_t *va = vals, *vb = vals + n1;
  for (int pass = 0; pass < kRadixPasses; ++pass) {
    const int shift = pass * kRadixBits;
    hipLaunchKernelGGL(k_vox_hist, dim3(nrb), dim3(kVoxBlock), 0, s, (const uint64_t *)ka, n,
                       shift, hist);
    CHECK_LAUNCH("k_vox_hist");
    hipLaunchKernelGGL(k_vox_offsets, dim3(kRadix), dim3(kVoxBlock), 0, s, hist, (int)nrb,
                       totals);
    CHECK_LAUNCH("k_vox_offsets");
    hipLaunchKernelGGL(k_vox_scatter, dim3(nrb), dim3(kVoxBlock), 0, s, (const uint64_t *)ka,
                       (const uint32_t *)va, kb, vb, n, shift, (const uint32_t *)hist,
                       (const uint32_t *)totals);
    CHECK_LAUNCH("k_vox_scatter");
    std::swap(ka, kb);
    std::swap(va, vb);
  }
  // an even number of passes: the sorted arrays are ka, va (the first halves)
  hipLaunchKernelGGL(k_vox_heads, dim3(nsb), dim3(kVoxBlock), 0, s, (const uint64_t *)ka, n, bsum);
  CHECK_LAUNCH("k_vox_heads");
  hipLaunchKernelGGL(k_vox_scan_sums, dim3(1), dim3(kVoxBlock), 0, s, bsum, (int)nsb, n,
                     (const uint32_t *)ctr, stats);
  CHECK_LAUNCH("k_vox_scan_sums");
  hipLaunchKernelGGL(k_vox_number, dim3(nsb), dim3(kVoxBlock), 0, s, (const uint64_t *)ka,
                     (const uint32_t *)va, n, (const int32_t *)bsum, cap, vox, seg, labels, cells);
  CHECK_LAUNCH("k_vox_number");
  const SegIn in{pts, ka, va, vox, cent_ws, n};
  RC(seg_sums_run<0>(ctx, in, nsb, agg, carry, seg, cap, cent_ws, centroids, counts));
  if (cov) RC(seg_sums_run<1>(ctx, in, nsb, agg, carry, seg, cap, cent_ws, cov, nullptr));
  return NAVGPU_OK;
}

}  // namespace

extern "C" {

int navgpu_voxel_downsample_dev(navgpu_ctx *ctx, const double *pts, size_t n, double voxel,
                                const double *origin, size_t cap, double *centroids,
                                int32_t *counts, double *cov, int32_t *cells, int32_t *labels,
                                double *stats) {
  return voxel_run(ctx, pts, n, voxel, origin, cap, centroids, counts, cov, cells, labels, stats);
}

int navgpu_voxel_downsample_host(navgpu_ctx *ctx, const double *pts, size_t n, double voxel,
                                 const double *origin, size_t cap, double *centroids,
                                 int32_t *counts, double *cov, int32_t *cells, int32_t *labels,
                                 double *stats) {
  RC(voxel_check(ctx, n, voxel, origin));
  ARG_CHECK(stats);
  ARG_CHECK(n == 0 || pts);
  ARG_CHECK(cap == 0 || centroids);
  double *dp, *dc, *dcov = nullptr, *dst;
  int32_t *dcnt = nullptr, *dcell = nullptr, *dlab = nullptr;
  RC(cloud_to_dev(ctx, kH0, pts, 3 * n, &dp));
  RC(ws(ctx, kH1, 3 * std::max<size_t>(cap, 1), &dc));
  if (counts) RC(ws(ctx, kH2, std::max<size_t>(cap, 1), &dcnt));
  if (cov) RC(ws(ctx, kH3, 6 * std::max<size_t>(cap, 1), &dcov));
  if (cells) RC(ws(ctx, kH4, 3 * std::max<size_t>(cap, 1), &dcell));
  if (labels) RC(ws(ctx, kH5, std::max<size_t>(n, 1), &dlab));
  RC(ws(ctx, kVoxOut, 7, &dst));
  RC(voxel_run(ctx, dp, n, voxel, origin, cap, dc, dcnt, dcov, dcell, dlab, dst));
  hipStream_t s = ctx->stream;
  HIP_TRY(hipMemcpyAsync(stats, dst, 7 * sizeof(double), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  const size_t nv = (size_t)stats[0], m = std::min(nv, cap);
  if (m) {
    HIP_TRY(hipMemcpyAsync(centroids, dc, 24 * m, hipMemcpyDeviceToHost, s));
    if (counts) HIP_TRY(hipMemcpyAsync(counts, dcnt, 4 * m, hipMemcpyDeviceToHost, s));
    if (cov) HIP_TRY(hipMemcpyAsync(cov, dcov, 48 * m, hipMemcpyDeviceToHost, s));
    if (cells) HIP_TRY(hipMemcpyAsync(cells, dcell, 12 * m, hipMemcpyDeviceToHost, s));
  }
  if (labels && n) HIP_TRY(hipMemcpyAsync(labels, dlab, 4 * n, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  if (nv > cap) {
    set_err("voxel_downsample: %zu voxels, capacity %zu", nv, cap);
    return NAVGPU_ERANGE;
  }
  return NAVGPU_OK;
}

}  // extern "C"
