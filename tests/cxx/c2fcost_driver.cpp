// C++ caller of CTR::CoarseFlowClass with the Huber patch cost (include/ctr_shim.hpp). Used by the tests.
//   c2fcost_driver frames.f32 w h pad lv_f step psz maxiter eps patnorm x_only huber_k
// frames.f32: frame A and frame B, 2 x h x w float32, row-major, native byte order. Builds both pyramids (levels 0 .. lv_f,
// padded by pad), checks that SetCost refuses cost 1, an unknown code and a huber_k of 0, -1, NaN and infinity and that the
// object then still reports L2, sets SetCost(ICTR_C2F_COST_HUBER, huber_k) (and SetPatnorm / SetXOnly as asked), runs the
// coarse-to-fine flow A -> B and prints one line per pixel in row-major order: u and v as hexadecimal floats (%a); then one
// line per level from lv_f down: "level l", the number of nodes of each status 0 .. 4, and the level's node displacements
// after the fill in row-major order (x y per node) as hexadecimal floats.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "ctr_shim.hpp"

using namespace CTR;

static bool refused(CoarseFlowClass &c, int cost, float k) {
  try {
    c.SetCost(cost, k);
  } catch (const std::exception &) {
    return true;
  }
  return false;
}

int main(int argc, char **argv) {
  if (argc != 13) {
    fprintf(stderr, "usage: %s frames.f32 w h pad lv_f step psz maxiter eps patnorm x_only huber_k\n", argv[0]);
    return 2;
  }
  const int w = atoi(argv[2]), h = atoi(argv[3]), pad = atoi(argv[4]), lv_f = atoi(argv[5]), step = atoi(argv[6]);
  const int psz = atoi(argv[7]), maxiter = atoi(argv[8]), patnorm = atoi(argv[10]), x_only = atoi(argv[11]);
  const float huber_k = (float)atof(argv[12]);
  if (w < 1 || h < 1 || pad < 1 || lv_f < 0 || lv_f > 15) {
    fprintf(stderr, "bad sizes\n");
    return 2;
  }
  const size_t n = (size_t)w * h;
  std::vector<float> frames(2 * n), out(2 * n);
  FILE *f = fopen(argv[1], "rb");
  const bool ok = f && fread(frames.data(), sizeof(float), frames.size(), f) == frames.size();
  if (f) fclose(f);
  if (!ok) {
    fprintf(stderr, "cannot read 2 frames of %d x %d\n", w, h);
    return 1;
  }
  try {
    Pyramid a(frames.data(), w, h, lv_f, true, pad), b(frames.data() + n, w, h, lv_f, true, pad);
    CoarseFlowClass c(w, h, lv_f, step, psz);
    c.SetParams(maxiter, (float)atof(argv[9]));
    int cost = -1;
    float k = 0.0f;
    const bool all_refused = refused(c, 1, 5.0f) && refused(c, 3, 5.0f) && refused(c, -1, 5.0f) &&
                             refused(c, ICTR_C2F_COST_HUBER, 0.0f) && refused(c, ICTR_C2F_COST_HUBER, -1.0f) &&
                             refused(c, ICTR_C2F_COST_HUBER, NAN) && refused(c, ICTR_C2F_COST_HUBER, INFINITY) &&
                             refused(c, ICTR_C2F_COST_L2, NAN);
    c.GetCost(&cost, &k);
    if (!all_refused || cost != ICTR_C2F_COST_L2 || k != 5.0f) {
      fprintf(stderr, "a bad SetCost was accepted or changed the object (cost %d, huber_k %g)\n", cost, (double)k);
      return 1;
    }
    c.SetCost(ICTR_C2F_COST_HUBER, huber_k);
    c.GetCost(&cost, &k);
    if (cost != ICTR_C2F_COST_HUBER || k != huber_k) {
      fprintf(stderr, "SetCost(ICTR_C2F_COST_HUBER, %g) did not hold\n", (double)huber_k);
      return 1;
    }
    if (patnorm) c.SetPatnorm(true);
    if (x_only) c.SetXOnly(true);
    c.Run(a, b);
    c.Result(out.data());
    for (size_t i = 0; i < n; ++i) printf("%a %a\n", (double)out[2 * i], (double)out[2 * i + 1]);
    for (int l = lv_f; l >= 0; --l) {
      int nx = 0, ny = 0;
      c.LevelDims(l, nullptr, nullptr, &nx, &ny);
      std::vector<unsigned char> st((size_t)nx * ny);
      std::vector<float> d(2 * (size_t)nx * ny);
      c.ReadLevel(l, nullptr, d.data(), st.data());
      int cnt[5] = {0, 0, 0, 0, 0};
      for (unsigned char s : st) ++cnt[s < 5 ? s : 0];
      printf("level %d %d %d %d %d %d", l, cnt[0], cnt[1], cnt[2], cnt[3], cnt[4]);
      for (float v : d) printf(" %a", (double)v);
      printf("\n");
    }
  } catch (const std::exception &e) {
    fprintf(stderr, "%s\n", e.what());
    return 1;
  }
  return 0;
}
