// Host driver of csrc/geom_ad.h (plain C++17, no HIP): the rotated IoU and its gradient on a CPU,
// so the math can run under host sanitizers (tests/test_cpu_riou_cases.py builds it with
// -fsanitize=address,undefined).
//
//   riou_host CASES
//
// Every line of CASES holds either
//   10 numbers: a box (x y w l yaw) and a target box  -> prints "iou g0 g1 g2 g3 g4"
//   16 numbers: six raw outputs, an anchor (5), a target (5), the raw outputs and the anchor
//               rounded to f32 as the loss kernel reads them -> prints "iou g0 .. g5"
// with 17 significant digits ("inf" / "nan" are accepted and printed as such).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "geom_ad.h"

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
    double iou = 0.0;
    if (v.size() == 10) {
      double g[5];
      ivit::ad::riou_grad(v.data(), v.data() + 5, &iou, g);
      std::printf("%.17g %.17g %.17g %.17g %.17g %.17g\n", iou, g[0], g[1], g[2], g[3], g[4]);
    } else if (v.size() == 16) {
      float d[6], a[5];
      for (int k = 0; k < 6; ++k) d[k] = (float)v[k];
      for (int k = 0; k < 5; ++k) a[k] = (float)v[6 + k];
      double box[5], g[5], gr[6];
      ivit::ad::decode_f64(d, a, box);
      ivit::ad::riou_grad(box, v.data() + 11, &iou, g);
      ivit::ad::decode_chain(d, a, box, g, gr);
      std::printf("%.17g %.17g %.17g %.17g %.17g %.17g %.17g\n", iou, gr[0], gr[1], gr[2], gr[3], gr[4], gr[5]);
    } else {
      std::fprintf(stderr, "%s: line %ld holds %zu numbers (10 or 16 expected)\n", argv[0], lineno, v.size());
      std::fclose(f);
      return 2;
    }
  }
  std::fclose(f);
  return 0;
}
