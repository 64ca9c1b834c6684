// Host caller of csrc/ictr_handover_hd.h (ho_point, ho_npairs, ho_offset) as plain C++. Used by
// tests/test_windowcams_cpu.py, built with -ffp-contract=off and the address / undefined-behaviour sanitizers.
//   handover_hd_host in.bin out.bin
// in.bin:  int64 M, bsize; f64 fx, fy, cx, cy, baseline; f64 xy_t[M][4][bsize] (left x, y, right x, y per frame)
// out.bin: int64 npairs, offset; f64 X[3][M]
#include <cstdint>
#include <cstdio>
#include <vector>

#include "ictr_handover_hd.h"

using namespace ictr;

int main(int argc, char **argv) {
  if (argc != 3) return 2;
  FILE *f = fopen(argv[1], "rb"), *o = fopen(argv[2], "wb");
  if (!f || !o) return 1;
  int64_t hdr[2];
  double prm[5];
  if (fread(hdr, sizeof(int64_t), 2, f) != 2 || fread(prm, sizeof(double), 5, f) != 5) return 1;
  const int64_t M = hdr[0], B = hdr[1];
  if (M < 0 || B < 1 || B > 256) return 1;
  std::vector<double> xy_t((size_t)(M * 4 * B)), X((size_t)(3 * M));
  if (M > 0 && fread(xy_t.data(), sizeof(double), xy_t.size(), f) != xy_t.size()) return 1;
  const HoCam cam = {prm[0], prm[1], prm[2], prm[3]};
  const double bf = prm[4] * cam.fx;
  for (int64_t m = 0; m < M; ++m) {
    const double *row = xy_t.data() + (size_t)(m * 4 * B);
    double p[3];
    ho_point(row[0], row[(size_t)B], row[(size_t)(2 * B)], bf, cam, p);
    for (int c = 0; c < 3; ++c) X[(size_t)(c * M + m)] = p[c];
  }
  const int64_t half[2] = {ho_npairs((int)B), ho_offset((int)B)};
  fwrite(half, sizeof(int64_t), 2, o);
  if (M > 0) fwrite(X.data(), sizeof(double), X.size(), o);
  fclose(f);
  fclose(o);
  return 0;
}
