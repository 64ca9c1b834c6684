// C++ caller of CTR::CoarseFlowSet (include/ctr_shim.hpp). Used by the tests.
//   c2fset_driver frames.f32 w h pad lv_f step psz n patnorm
// frames.f32: n + 1 frames, (n + 1) x h x w float32, row-major, native byte order. Builds the n + 1 pyramids (levels
// 0 .. lv_f, padded by pad) and n coarse-to-fine flows, member m for the pair (frame m, frame m + 1), so that neighbouring
// members share a pyramid. Checks that a set with the same object twice, a set of no members and a set whose second member
// has another maxiter are refused, runs the n members in lockstep and prints "ops <operations>", then per member from 0 one
// line per pixel in row-major order, u and v as hexadecimal floats (%a), and one line per level from lv_f down: "level l",
// the number of nodes of each status 0 .. 4, and the level's node displacements after the fill (x y per node).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "ctr_shim.hpp"

using namespace CTR;

static bool refused(CoarseFlowClass *const *m, int n, const char *needle) {
  try {
    CoarseFlowSet s(m, n);
  } catch (const std::exception &e) {
    return strstr(e.what(), needle) != nullptr;
  }
  return false;
}

int main(int argc, char **argv) {
  if (argc != 10) {
    fprintf(stderr, "usage: %s frames.f32 w h pad lv_f step psz n patnorm\n", argv[0]);
    return 2;
  }
  const int w = atoi(argv[2]), h = atoi(argv[3]), pad = atoi(argv[4]), lv_f = atoi(argv[5]), step = atoi(argv[6]);
  const int psz = atoi(argv[7]), n = atoi(argv[8]), patnorm = atoi(argv[9]);
  if (w < 1 || h < 1 || pad < 1 || lv_f < 0 || lv_f > 15 || n < 2 || n > ICTR_C2FSET_MAX) {
    fprintf(stderr, "bad sizes (n is 2 .. %d)\n", (int)ICTR_C2FSET_MAX);
    return 2;
  }
  const size_t px = (size_t)w * h;
  std::vector<float> frames((size_t)(n + 1) * px), out(2 * px);
  FILE *f = fopen(argv[1], "rb");
  const bool ok = f && fread(frames.data(), sizeof(float), frames.size(), f) == frames.size();
  if (f) fclose(f);
  if (!ok) {
    fprintf(stderr, "cannot read %d frames of %d x %d\n", n + 1, w, h);
    return 1;
  }
  try {
    std::vector<std::unique_ptr<Pyramid>> pyr;
    for (int i = 0; i <= n; ++i) pyr.emplace_back(new Pyramid(frames.data() + i * px, w, h, lv_f, true, pad));
    std::vector<std::unique_ptr<CoarseFlowClass>> flow;
    std::vector<CoarseFlowClass *> m;
    std::vector<const Pyramid *> a, b;
    for (int i = 0; i < n; ++i) {
      flow.emplace_back(new CoarseFlowClass(w, h, lv_f, step, psz));
      if (patnorm) flow.back()->SetPatnorm(true);
      m.push_back(flow.back().get());
      a.push_back(pyr[i].get());
      b.push_back(pyr[i + 1].get());
    }
    CoarseFlowClass *twice[2] = {m[0], m[0]};
    CoarseFlowClass other(w, h, lv_f, step, psz);
    if (patnorm) other.SetPatnorm(true);
    other.SetParams(3);
    CoarseFlowClass *differ[2] = {m[0], &other};
    if (!refused(twice, 2, "member 1 is the same object as member 0") || !refused(m.data(), 0, "n is 0") ||
        !refused(differ, 2, "member 1 differs from member 0 in maxiter")) {
      fprintf(stderr, "a bad set was accepted, or refused without its reason\n");
      return 1;
    }
    CoarseFlowSet set(m.data(), n);
    if (set.Size() != n || set.Operations() != 0) {
      fprintf(stderr, "a new set reports %d members and %d operations\n", set.Size(), set.Operations());
      return 1;
    }
    set.Run(a.data(), b.data());
    printf("ops %d\n", set.Operations());
    for (int i = 0; i < n; ++i) {
      CoarseFlowClass &c = *m[i];
      c.Result(out.data());
      for (size_t k = 0; k < px; ++k) printf("%a %a\n", (double)out[2 * k], (double)out[2 * k + 1]);
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
    }
  } catch (const std::exception &e) {
    fprintf(stderr, "%s\n", e.what());
    return 1;
  }
  return 0;
}
