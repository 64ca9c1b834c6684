// C++ caller of CTR::CoarseFlowClass on colour frames (include/ctr_shim.hpp: SetChannels, RunRGB, ReadLevelBiasRGB). Used by
// the tests.
//   c2frgb_driver frames.f32 w h pad lv_f step psz maxiter eps patnorm refine
// frames.f32: frame A and frame B as three planes each, 2 x 3 x h x w float32, row-major, native byte order. Builds the six
// pyramids (levels 0 .. lv_f, padded by pad), runs the coarse-to-fine flow A -> B on three channels (patnorm: 0 / 1;
// refine: 0, or n_outer of a refinement with n_sor = 2 per level) and prints one line per pixel in row-major order: u and v
// as hexadecimal floats (%a); then one line per level from lv_f down: "level l" and the number of nodes of each status
// 0 .. 4; then, with patnorm, one line per node of level 0: its three betas as hexadecimal floats.
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "ctr_shim.hpp"

using namespace CTR;

int main(int argc, char **argv) {
  if (argc != 12) {
    fprintf(stderr, "usage: %s frames.f32 w h pad lv_f step psz maxiter eps patnorm refine\n", argv[0]);
    return 2;
  }
  const int w = atoi(argv[2]), h = atoi(argv[3]), pad = atoi(argv[4]), lv_f = atoi(argv[5]), step = atoi(argv[6]);
  const int psz = atoi(argv[7]), maxiter = atoi(argv[8]), patnorm = atoi(argv[10]), refine = atoi(argv[11]);
  if (w < 1 || h < 1 || pad < 1 || lv_f < 0 || lv_f > 15) {
    fprintf(stderr, "bad sizes\n");
    return 2;
  }
  const size_t n = (size_t)w * h;
  std::vector<float> frames(6 * n), out(2 * n);
  FILE *f = fopen(argv[1], "rb");
  const bool ok = f && fread(frames.data(), sizeof(float), frames.size(), f) == frames.size();
  if (f) fclose(f);
  if (!ok) {
    fprintf(stderr, "cannot read 2 frames of 3 x %d x %d\n", w, h);
    return 1;
  }
  try {
    std::unique_ptr<Pyramid> pyr[6];
    const Pyramid *a[3], *b[3];
    for (int k = 0; k < 6; ++k) pyr[k].reset(new Pyramid(frames.data() + k * n, w, h, lv_f, true, pad));
    for (int c = 0; c < 3; ++c) a[c] = pyr[c].get(), b[c] = pyr[3 + c].get();
    CoarseFlowClass c(w, h, lv_f, step, psz);
    c.SetChannels(3);
    c.SetParams(maxiter, (float)atof(argv[9]));
    c.SetPatnorm(patnorm != 0);
    if (refine > 0) c.SetRefine(true, 16.0f, 13.0f, 4.5f, refine, 2);
    c.RunRGB(a, b);
    c.Result(out.data());
    for (size_t i = 0; i < n; ++i) printf("%a %a\n", (double)out[2 * i], (double)out[2 * i + 1]);
    for (int l = lv_f; l >= 0; --l) {
      int nx = 0, ny = 0;
      c.LevelDims(l, nullptr, nullptr, &nx, &ny);
      std::vector<unsigned char> st((size_t)nx * ny);
      c.ReadLevel(l, nullptr, nullptr, st.data());
      int cnt[5] = {0, 0, 0, 0, 0};
      for (unsigned char s : st) ++cnt[s < 5 ? s : 0];
      printf("level %d %d %d %d %d %d\n", l, cnt[0], cnt[1], cnt[2], cnt[3], cnt[4]);
    }
    if (patnorm) {
      int nx = 0, ny = 0;
      c.LevelDims(0, nullptr, nullptr, &nx, &ny);
      std::vector<float> bias((size_t)3 * nx * ny);
      c.ReadLevelBiasRGB(0, bias.data());
      for (size_t i = 0; i < (size_t)nx * ny; ++i)
        printf("%a %a %a\n", (double)bias[3 * i], (double)bias[3 * i + 1], (double)bias[3 * i + 2]);
    }
    if (c.Channels() != 3) return 3;
  } catch (const std::exception &e) {
    fprintf(stderr, "%s\n", e.what());
    return 1;
  }
  return 0;
}
