// Host driver of csrc/geom.h (plain C++17, no HIP): the rotated and the axis-aligned IoU of box
// pairs on a CPU, so the 12-slot Poly and the clip can run under host sanitizers
// (tests/test_cpu_geom_cases.py builds it with -fsanitize=address,undefined).
//
//   geom_host CASES
//
// Every line of CASES holds 10 numbers, two boxes (x y w l yaw) that are rounded to f32 as the
// kernels read them -> prints "rotated_iou axis_iou" of (first, second) with 9 significant
// digits, which identify an f32 ("inf" / "nan" are accepted and printed as such).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "geom.h"

int main(int argc, char** argv) {
  if (argc != 2) {
    std::fprintf(stderr, "usage: %s CASES\n", argv[0]);
    return 2;
  }
  std::FILE* f = std::fopen(argv[1], "r");
  if (!f) {
    std::fprintf(stderr, "%s: cannot open %s\n", argv[0], argv[1]);
    return 2;
  }
  char line[4096];
  long lineno = 0;
  while (std::fgets(line, sizeof line, f)) {
    ++lineno;
    std::vector<double> v;
    char* s = line;
    for (;;) {
      char* e = nullptr;
      const double x = std::strtod(s, &e);
      if (e == s) break;
      v.push_back(x);
      s = e;
    }
    if (v.empty()) continue;
    if (v.size() != 10) {
      std::fprintf(stderr, "%s: line %ld holds %zu numbers (10 expected)\n", argv[0], lineno, v.size());
      std::fclose(f);
      return 2;
    }
    float a[5], b[5];
    for (int k = 0; k < 5; ++k) {
      a[k] = (float)v[k];
      b[k] = (float)v[5 + k];
    }
    std::printf("%.9g %.9g\n", (double)ivit::rotated_iou(a, b), (double)ivit::axis_iou(a, b));
  }
  std::fclose(f);
  return 0;
}
