// Stand-alone host driver of nav-slam_amd/csrc/align_solve.h for
// tests/test_align_solve.py (built there with the address and undefined-
// behaviour sanitizers). Reads commands from stdin, one per line, numbers as
// C hex floats:
//   solve   m[20]              -> delta[12] stats[4]
//   compose delta[12] pose[12] -> pose[12]
#include <cstdio>
#include <cstring>

#include "align_solve.h"

static bool read_n(double *v, int n) {
  for (int i = 0; i < n; ++i)
    if (std::scanf("%la", &v[i]) != 1) return false;
  return true;
}

static void print_n(const double *v, int n) {
  for (int i = 0; i < n; ++i) std::printf("%a%c", v[i], i + 1 == n ? '\n' : ' ');
}

int main() {
  char cmd[16];
  while (std::scanf("%15s", cmd) == 1) {
    if (!std::strcmp(cmd, "solve")) {
      double m[nv::kAlignMoments], out[16];
      if (!read_n(m, nv::kAlignMoments)) return 2;
      nv::align_solve(m, out, out + 12);
      print_n(out, 16);
    } else if (!std::strcmp(cmd, "compose")) {
      double d[12], p[12];
      if (!read_n(d, 12) || !read_n(p, 12)) return 2;
      nv::pose_compose(d, p);
      print_n(p, 12);
    } else {
      return 3;
    }
  }
  return 0;
}
