// voxel_key.h — the cell and key rule of the voxel-grid downsampling
// (voxel.hip): cell from coordinate, the drop rule, pack and
// unpack, and the argument checks. Plain C++ for host and device alike, the
// way align_solve.h is written: no HIP headers, only f64 IEEE subtraction,
// division and floor with no contraction, so that the device (k_vox_keys), the
// host variant's argument checks and a host build
// (tests/voxel_key_driver.cpp) give the same cells.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define NV_VK_HD __host__ __device__
#else
#define NV_VK_HD
#endif

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace nv {

constexpr int kVoxCellBits = 21;                       // bits of a cell per axis
constexpr double kVoxCellLimit = 2097152.0;            // 2^21: a cell is in [0, 2^21)
constexpr uint64_t kVoxCellMask = (1ull << kVoxCellBits) - 1;
constexpr uint64_t kVoxNoKey = ~0ull;                  // a dropped point: sorts last

// what became of a point
constexpr int kVoxKept = 0, kVoxNonFinite = 1, kVoxOutOfRange = 2;

// false for a NaN and for either infinity
NV_VK_HD inline bool vox_finite(double v) { return v - v == 0.0; }

// t = floor((x - o) / voxel) on each axis. A point is dropped when a
// coordinate is not finite, or when a t fails 0 <= t < 2^21: the comparison is
// made in double, so the conversion below never sees a value out of range (a
// NaN t, from an overflowing difference, fails it too).
NV_VK_HD inline int vox_cell(const double p[3], const double o[3], double voxel, int32_t c[3]) {
  if (!(vox_finite(p[0]) && vox_finite(p[1]) && vox_finite(p[2]))) return kVoxNonFinite;
  double t[3];
  for (int a = 0; a < 3; ++a) t[a] = __builtin_floor((p[a] - o[a]) / voxel);
  for (int a = 0; a < 3; ++a)
    if (!(t[a] >= 0.0 && t[a] < kVoxCellLimit)) return kVoxOutOfRange;
  for (int a = 0; a < 3; ++a) c[a] = (int32_t)t[a];
  return kVoxKept;
}

// key = ix 2^42 + iy 2^21 + iz: 63 bits, ascending key = ascending (ix, iy, iz)
NV_VK_HD inline uint64_t vox_pack(const int32_t c[3]) {
  return ((uint64_t)c[0] << (2 * kVoxCellBits)) | ((uint64_t)c[1] << kVoxCellBits) |
         (uint64_t)c[2];
}

NV_VK_HD inline void vox_unpack(uint64_t key, int32_t c[3]) {
  c[0] = (int32_t)((key >> (2 * kVoxCellBits)) & kVoxCellMask);
  c[1] = (int32_t)((key >> kVoxCellBits) & kVoxCellMask);
  c[2] = (int32_t)(key & kVoxCellMask);
}

// the key of a point, kVoxNoKey when it is dropped; *why: kVoxKept, ...
NV_VK_HD inline uint64_t vox_key(const double p[3], const double o[3], double voxel, int *why) {
  int32_t c[3];
  *why = vox_cell(p, o, voxel, c);
  return *why == kVoxKept ? vox_pack(c) : kVoxNoKey;
}

// voxel finite and > 0; a given origin finite
NV_VK_HD inline bool vox_voxel_ok(double voxel) { return vox_finite(voxel) && voxel > 0.0; }
NV_VK_HD inline bool vox_origin_ok(const double *o) {
  return !o || (vox_finite(o[0]) && vox_finite(o[1]) && vox_finite(o[2]));
}

}  // namespace nv
