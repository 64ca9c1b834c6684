// C++ caller of CTR::CoarseFlowClass with a finest level above 0 and of CTR::UpsampleFlow (include/ctr_shim.hpp). Used by
// the tests.
//   c2fup_driver frames.f32 w h pad lv_f lv_l step psz maxiter eps
// frames.f32: frame A and frame B, 2 x h x w float32, row-major, native byte order. Builds both pyramids (levels 0 .. lv_f,
// padded by pad), runs the coarse-to-fine flow A -> B on an object made with lv_l and prints one line per pixel in row-major
// order: u and v of the result as hexadecimal floats (%a). Then "level lv_l w_l h_l" (LvL and LevelDims), and, per pixel
// again, CTR::UpsampleFlow of that level's field as ReadLevel gives it (host arrays): the same bits once more.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "ctr_shim.hpp"

using namespace CTR;

int main(int argc, char **argv) {
  if (argc != 11) {
    fprintf(stderr, "usage: %s frames.f32 w h pad lv_f lv_l step psz maxiter eps\n", argv[0]);
    return 2;
  }
  const int w = atoi(argv[2]), h = atoi(argv[3]), pad = atoi(argv[4]), lv_f = atoi(argv[5]), lv_l = atoi(argv[6]);
  const int step = atoi(argv[7]), psz = atoi(argv[8]), maxiter = atoi(argv[9]);
  if (w < 1 || h < 1 || pad < 1 || lv_f < 0 || lv_f > 15 || lv_l < 1) {
    fprintf(stderr, "bad sizes\n");
    return 2;
  }
  const size_t n = (size_t)w * h;
  std::vector<float> frames(2 * n), out(2 * n), again(2 * n);
  FILE *f = fopen(argv[1], "rb");
  const bool ok = f && fread(frames.data(), sizeof(float), frames.size(), f) == frames.size();
  if (f) fclose(f);
  if (!ok) {
    fprintf(stderr, "cannot read 2 frames of %d x %d\n", w, h);
    return 1;
  }
  try {
    Pyramid a(frames.data(), w, h, lv_f, true, pad), b(frames.data() + n, w, h, lv_f, true, pad);
    CoarseFlowClass c(w, h, lv_f, step, psz, lv_l);
    c.SetParams(maxiter, (float)atof(argv[10]));
    c.Run(a, b);
    c.Result(out.data());
    for (size_t i = 0; i < n; ++i) printf("%a %a\n", (double)out[2 * i], (double)out[2 * i + 1]);
    int wl = 0, hl = 0;
    c.LevelDims(c.LvL(), &wl, &hl, nullptr, nullptr);
    printf("level %d %d %d\n", c.LvL(), wl, hl);
    std::vector<float> field(2 * (size_t)wl * hl);
    c.ReadLevel(c.LvL(), field.data(), nullptr, nullptr);
    UpsampleFlow(field.data(), wl, hl, c.LvL(), again.data(), w, h);
    for (size_t i = 0; i < n; ++i) printf("%a %a\n", (double)again[2 * i], (double)again[2 * i + 1]);
  } catch (const std::exception &e) {
    fprintf(stderr, "%s\n", e.what());
    return 1;
  }
  return 0;
}
