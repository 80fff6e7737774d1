// Stand-alone host driver of nav-slam_amd/csrc/plane_solve.h for
// tests/test_plane_solve.py (built there with the address and undefined-
// behaviour sanitizers). Reads commands from stdin, one per line, numbers as
// C hex floats:
//   eig3  c[6]   -> lam[3] vec[9]      (c = xx xy xz yy yz zz)
//   plane m[33]  -> delta[12] stats[6]
#include <cstdio>
#include <cstring>

#include "plane_solve.h"

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
    if (!std::strcmp(cmd, "eig3")) {
      double c[6], out[12];
      if (!read_n(c, 6)) return 2;
      nv::sym3_eig(c, out, out + 3);
      print_n(out, 12);
    } else if (!std::strcmp(cmd, "plane")) {
      double m[nv::kPlaneMoments], out[18];
      if (!read_n(m, nv::kPlaneMoments)) return 2;
      nv::plane_solve(m, out, out + 12);
      print_n(out, 18);
    } else {
      return 3;
    }
  }
  return 0;
}
