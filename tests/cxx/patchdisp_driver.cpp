// C++ caller of ictr_patchdisp (include/ictr.h) on pyramids of include/ctr_shim.hpp. Used by the tests.
//   patchdisp_driver frames.f32 pts.f32 w h K psz lv_f lv_l maxiter eps
// frames.f32: the left and the right frame, 2 x h x w float32, row-major, native byte order. pts.f32: K x 2 float32 (x, y).
// Tracks the points left -> right along x and prints one line per point: x and y as hexadecimal floats (%a; "nan" for a
// lost point), the status, the iteration count; then a line "form F" with the kernel form of the launch.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "ctr_shim.hpp"

using namespace CTR;

static bool read_f32(const char *fn, std::vector<float> &v) {
  FILE *f = fopen(fn, "rb");
  const bool ok = f && fread(v.data(), sizeof(float), v.size(), f) == v.size();
  if (f) fclose(f);
  return ok;
}

int main(int argc, char **argv) {
  if (argc != 11) {
    fprintf(stderr, "usage: %s frames.f32 pts.f32 w h K psz lv_f lv_l maxiter eps\n", argv[0]);
    return 2;
  }
  const int w = atoi(argv[3]), h = atoi(argv[4]), K = atoi(argv[5]), psz = atoi(argv[6]), lv_f = atoi(argv[7]);
  const int lv_l = atoi(argv[8]), maxiter = atoi(argv[9]);
  const float eps = (float)atof(argv[10]);
  if (w < 1 || h < 1 || K < 0) {
    fprintf(stderr, "bad sizes\n");
    return 2;
  }
  std::vector<float> frames((size_t)2 * w * h), pts((size_t)2 * K);
  if (!read_f32(argv[1], frames) || !read_f32(argv[2], pts)) {
    fprintf(stderr, "cannot read 2 frames of %d x %d and %d points\n", w, h, K);
    return 1;
  }
  try {
    Pyramid left(frames.data(), w, h, lv_f, true, psz), right(frames.data() + (size_t)w * h, w, h, lv_f, false, psz);
    std::vector<float> soa((size_t)2 * K), out((size_t)2 * K);  // x[K] y[K]
    std::vector<int> status(K), iters(K);
    for (int k = 0; k < K; ++k) {
      soa[k] = pts[2 * k];
      soa[k + K] = pts[2 * k + 1];
    }
    check(ictr_patchdisp(left.handle(), right.handle(), soa.data(), K, psz, lv_f, lv_l, maxiter, eps, out.data(),
                         status.data(), iters.data()),
          "ictr_patchdisp");
    for (int k = 0; k < K; ++k) {
      if (std::isnan(out[k]))
        printf("nan nan %d %d\n", status[k], iters[k]);
      else
        printf("%a %a %d %d\n", (double)out[k], (double)out[k + K], status[k], iters[k]);
    }
    printf("form %d\n", ictr_patchdisp_last_form());
  } catch (const std::exception &e) {
    fprintf(stderr, "%s\n", e.what());
    return 1;
  }
  return 0;
}
