// C++ caller of CTR::FlowRefineClass (include/ctr_shim.hpp). Used by the tests.
//   flowrefine_driver frames.f32 flow.f32 w h pad alpha gamma delta n_outer n_sor omega x_only
// frames.f32: frame A and frame B, 2 x h x w float32, row-major, native byte order. flow.f32: h x w x 2 float32 (u, v).
// Refines the flow A -> B from the host field and prints one line per pixel in row-major order: u and v as hexadecimal
// floats (%a).
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
  if (argc != 13) {
    fprintf(stderr, "usage: %s frames.f32 flow.f32 w h pad alpha gamma delta n_outer n_sor omega x_only\n", argv[0]);
    return 2;
  }
  const int w = atoi(argv[3]), h = atoi(argv[4]), pad = atoi(argv[5]);
  if (w < 1 || h < 1 || pad < 1) {
    fprintf(stderr, "bad sizes\n");
    return 2;
  }
  const size_t n = (size_t)w * h;
  std::vector<float> frames(2 * n), flow(2 * n), out(2 * n);
  if (!read_f32(argv[1], frames) || !read_f32(argv[2], flow)) {
    fprintf(stderr, "cannot read 2 frames and a flow of %d x %d\n", w, h);
    return 1;
  }
  try {
    Pyramid a(frames.data(), w, h, 0, false, pad), b(frames.data() + n, w, h, 0, false, pad);
    FlowRefineClass r(w, h);
    r.SetParams((float)atof(argv[6]), (float)atof(argv[7]), (float)atof(argv[8]), atoi(argv[9]), atoi(argv[10]),
                (float)atof(argv[11]));
    r.Run(a, b, StereoTrackClass::Flow(flow.data()), atoi(argv[12]) != 0);
    r.Result(out.data());
    for (size_t i = 0; i < n; ++i) printf("%a %a\n", (double)out[2 * i], (double)out[2 * i + 1]);
  } catch (const std::exception &e) {
    fprintf(stderr, "%s\n", e.what());
    return 1;
  }
  return 0;
}
