// C++ caller of CTR::FlowDensifyClass (include/ctr_shim.hpp). Used by the tests.
//   densify_driver frames.f32 nodes.f32 lost.u8 w h pad step psz minerr power
// frames.f32: frame A and frame B, 2 x h x w float32, row-major, native byte order. nodes.f32: ny x nx x 2 float32 node
// displacements of a grid of `step`, lost.u8: ny x nx bytes (1: lost). Injects the nodes into a flow grid, densifies A -> B
// and prints one line per pixel in row-major order: u and v as hexadecimal floats (%a).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "ctr_shim.hpp"

using namespace CTR;

template <class T>
static bool read_raw(const char *fn, std::vector<T> &v) {
  FILE *f = fopen(fn, "rb");
  const bool ok = f && fread(v.data(), sizeof(T), v.size(), f) == v.size();
  if (f) fclose(f);
  return ok;
}

int main(int argc, char **argv) {
  if (argc != 11) {
    fprintf(stderr, "usage: %s frames.f32 nodes.f32 lost.u8 w h pad step psz minerr power\n", argv[0]);
    return 2;
  }
  const int w = atoi(argv[4]), h = atoi(argv[5]), pad = atoi(argv[6]), step = atoi(argv[7]), psz = atoi(argv[8]);
  if (w < 1 || h < 1 || pad < 1 || step < 1) {
    fprintf(stderr, "bad sizes\n");
    return 2;
  }
  ictr_flowgrid *grid = nullptr;
  int nx = 0, ny = 0;
  if (ictr_flowgrid_create(&grid, w, h, step) || ictr_flowgrid_dims(grid, &nx, &ny)) {
    fprintf(stderr, "%s\n", ictr_last_error());
    return 1;
  }
  int rc = 0;
  const size_t n = (size_t)w * h;
  std::vector<float> frames(2 * n), nodes(2 * (size_t)nx * ny), out(2 * n);
  std::vector<uint8_t> lost((size_t)nx * ny);
  if (!read_raw(argv[1], frames) || !read_raw(argv[2], nodes) || !read_raw(argv[3], lost)) {
    fprintf(stderr, "cannot read 2 frames of %d x %d and a node table of %d x %d\n", w, h, nx, ny);
    rc = 1;
  } else if (ictr_flowgrid_set_nodes(grid, nodes.data(), lost.data())) {
    fprintf(stderr, "%s\n", ictr_last_error());
    rc = 1;
  } else {
    try {
      Pyramid a(frames.data(), w, h, 0, false, pad), b(frames.data() + n, w, h, 0, false, pad);
      FlowDensifyClass z(w, h);
      z.SetParams((float)atof(argv[9]), atoi(argv[10]));
      z.Run(grid, a, b, psz);
      z.Result(out.data());
      for (size_t i = 0; i < n; ++i) printf("%a %a\n", (double)out[2 * i], (double)out[2 * i + 1]);
    } catch (const std::exception &e) {
      fprintf(stderr, "%s\n", e.what());
      rc = 1;
    }
  }
  ictr_flowgrid_destroy(grid);
  return rc;
}
