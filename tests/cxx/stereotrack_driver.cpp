// C++ caller of CTR::StereoTrackClass (include/ctr_shim.hpp). Used by the tests.
//   stereotrack_driver in.bin out.bin
// in.bin:  int64 H, W, bsize, N (0: every pixel in meshgrid order); f64 th_ratio, th_abs; f32 disp_lr[bsize][H][W],
//          disp_rl[bsize][H][W], flow_l[bsize][2][H][W][2] (fwd, bwd), flow_r likewise; f64 xy0[N][2] when N > 0
// out.bin: int64 M; int64 rows[M]; f64 xy_t[M][4][bsize]   (the files of tests/cxx/stereotrack_hd_host.cpp)
#include <cstdint>
#include <cstdio>
#include <vector>

#include "ctr_shim.hpp"

using namespace CTR;

int main(int argc, char **argv) {
  if (argc != 3) {
    fprintf(stderr, "usage: %s in.bin out.bin\n", argv[0]);
    return 2;
  }
  FILE *f = fopen(argv[1], "rb");
  int64_t hdr[4];
  double th[2];
  if (!f || fread(hdr, sizeof(int64_t), 4, f) != 4 || fread(th, sizeof(double), 2, f) != 2 || hdr[0] < 2 || hdr[0] > 32768 ||
      hdr[1] < 2 || hdr[1] > 32768 || hdr[2] < 1 || hdr[2] > 256 || hdr[3] < 0 || hdr[3] > (1 << 24)) {
    fprintf(stderr, "%s: cannot read the header\n", argv[1]);
    return 1;
  }
  const int64_t H = hdr[0], W = hdr[1], B = hdr[2], N = hdr[3];
  const size_t px = (size_t)(H * W);
  std::vector<float> dlr(px * B), drl(px * B), fl(px * B * 4), fr(px * B * 4);
  std::vector<double> xy0((size_t)(2 * N));
  if (fread(dlr.data(), sizeof(float), dlr.size(), f) != dlr.size() || fread(drl.data(), sizeof(float), drl.size(), f) != drl.size() ||
      fread(fl.data(), sizeof(float), fl.size(), f) != fl.size() || fread(fr.data(), sizeof(float), fr.size(), f) != fr.size() ||
      (N && fread(xy0.data(), sizeof(double), xy0.size(), f) != xy0.size())) {
    fprintf(stderr, "%s: truncated\n", argv[1]);
    return 1;
  }
  fclose(f);
  try {
    typedef StereoTrackClass S;
    S win((int)W, (int)H, (int)B, th[0], th[1]);
    win.Open(N ? xy0.data() : nullptr, N, S::Plane(dlr.data(), -1), S::Plane(drl.data()));
    for (int64_t k = 1; k < B; ++k) {
      const float *l = fl.data() + px * 4 * (k - 1), *r = fr.data() + px * 4 * (k - 1);
      win.Advance(S::Flow(l), S::Flow(l + px * 2), S::Flow(r), S::Flow(r + px * 2), S::Plane(dlr.data() + px * k, -1),
                  S::Plane(drl.data() + px * k));
    }
    const int64_t M = win.Count();
    std::vector<int64_t> rows((size_t)M);
    std::vector<double> xy_t((size_t)(M * 4 * B));
    win.Read(xy_t.data(), rows.data());
    FILE *o = fopen(argv[2], "wb");
    if (!o) return 1;
    fwrite(&M, sizeof(M), 1, o);
    fwrite(rows.data(), sizeof(int64_t), rows.size(), o);
    fwrite(xy_t.data(), sizeof(double), xy_t.size(), o);
    fclose(o);
    printf("kept %lld of %lld\n", (long long)M, (long long)(N ? N : H * W));
  } catch (const std::exception &e) {
    fprintf(stderr, "%s\n", e.what());
    return 1;
  }
  return 0;
}
