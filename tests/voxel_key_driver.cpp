// Stand-alone host driver of nav-slam_amd/csrc/voxel_key.h for
// tests/test_voxel_key.py (built there with the address and undefined-
// behaviour sanitizers). Reads commands from stdin, numbers as C hex floats:
//   key  voxel o[3] p[3] -> why ix iy iz key unpacked[3]   (cell -1 when dropped)
//   args voxel o[3]      -> voxel_ok origin_ok
#include <cinttypes>
#include <cstdio>
#include <cstring>

#include "voxel_key.h"

static bool read_n(double *v, int n) {
  for (int i = 0; i < n; ++i)
    if (std::scanf("%la", &v[i]) != 1) return false;
  return true;
}

int main() {
  char cmd[16];
  while (std::scanf("%15s", cmd) == 1) {
    double a[7];
    if (!std::strcmp(cmd, "key")) {
      if (!read_n(a, 7)) return 2;
      int32_t c[3] = {-1, -1, -1}, back[3] = {-1, -1, -1};
      const int why = nv::vox_cell(a + 4, a + 1, a[0], c);
      int why2;
      const uint64_t key = nv::vox_key(a + 4, a + 1, a[0], &why2);
      if (why2 != why) return 4;
      if (why == nv::kVoxKept) {
        if (key != nv::vox_pack(c)) return 5;
        nv::vox_unpack(key, back);
      } else if (key != nv::kVoxNoKey) {
        return 6;
      }
      std::printf("%d %d %d %d %" PRIu64 " %d %d %d\n", why, c[0], c[1], c[2], key, back[0],
                  back[1], back[2]);
    } else if (!std::strcmp(cmd, "args")) {
      if (!read_n(a, 4)) return 2;
      std::printf("%d %d\n", nv::vox_voxel_ok(a[0]) ? 1 : 0, nv::vox_origin_ok(a + 1) ? 1 : 0);
    } else {
      return 3;
    }
  }
  return 0;
}
