// C++ caller of CTR::PointTrackClass (include/ctr_shim.hpp). Used by the tests.
//   pointtrack_driver frames.f32 out.txt w h nframes bsize maxcorners lv_f psz step
// frames.f32: nframes x h x w float32, row-major, native byte order. Pushes the frames and writes every block as the track
// window holds it before compaction: a line "block b K", then K lines of 2 * bsize coordinates (x row, then y row), the
// valid flag and the absolute movement.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "ctr_shim.hpp"

using namespace CTR;

static std::string fmt(double v, int digits) {
  if (std::isnan(v)) return "nan";
  char b[64];
  snprintf(b, sizeof(b), "%.*g", digits, v);
  return b;
}

int main(int argc, char **argv) {
  if (argc != 11) {
    fprintf(stderr, "usage: %s frames.f32 out.txt w h nframes bsize maxcorners lv_f psz step\n", argv[0]);
    return 2;
  }
  const int w = atoi(argv[3]), h = atoi(argv[4]), n = atoi(argv[5]), bsize = atoi(argv[6]), mc = atoi(argv[7]);
  const int lv_f = atoi(argv[8]), psz = atoi(argv[9]), step = atoi(argv[10]);
  if (w < 1 || h < 1 || n < 1 || bsize < 1 || mc < 1) {
    fprintf(stderr, "bad sizes\n");
    return 2;
  }
  std::vector<float> frames((size_t)n * w * h);
  FILE *f = fopen(argv[1], "rb");
  if (!f || fread(frames.data(), sizeof(float), frames.size(), f) != frames.size()) {
    fprintf(stderr, "%s: cannot read %d frames of %d x %d\n", argv[1], n, w, h);
    return 1;
  }
  fclose(f);
  try {
    PointTrackClass pt(w, h, bsize, mc, lv_f, psz, step);
    for (int k = 0; k < n; ++k) pt.PushFrame(frames.data() + (size_t)k * w * h);
    std::vector<float> tr((size_t)mc * 2 * bsize);
    std::vector<uint8_t> valid(mc);
    std::vector<double> am(mc);
    FILE *o = fopen(argv[2], "w");
    if (!o) return 1;
    for (int64_t b = 0; b < pt.FrameCounter(); ++b) {
      const int K = pt.ReadBlock(b, tr.data(), valid.data(), am.data());
      fprintf(o, "block %lld %d\n", (long long)b, K);
      for (int i = 0; i < K; ++i) {
        std::string s;
        for (int c = 0; c < 2 * bsize; ++c) s += fmt(tr[(size_t)i * 2 * bsize + c], 9) + " ";
        fprintf(o, "%s%d %s\n", s.c_str(), (int)valid[i], fmt(am[i], 17).c_str());
      }
    }
    fclose(o);
  } catch (const std::exception &e) {
    fprintf(stderr, "%s\n", e.what());
    return 1;
  }
  return 0;
}
