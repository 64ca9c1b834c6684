// Host caller of csrc/ictr_stereotrack_hd.h (st_gather, st_open, st_advance over StMem fields) as plain C++. Used by
// tests/test_stereotrack_cpu.py, built with -ffp-contract=off and the address / undefined-behaviour sanitizers.
//   stereotrack_hd_host in.bin out.bin
// in.bin:  int64 H, W, bsize, N (0: every pixel in meshgrid order); f64 th_ratio, th_abs; f32 disp_lr[bsize][H][W],
//          disp_rl[bsize][H][W], flow_l[bsize][2][H][W][2] (fwd, bwd), flow_r likewise; f64 xy0[N][2] when N > 0
// out.bin: int64 M; int64 rows[M]; f64 xy_t[M][4][bsize]
#include <cstdint>
#include <cstdio>
#include <vector>

#include "ictr_stereotrack_hd.h"

using namespace ictr;

int main(int argc, char **argv) {
  if (argc != 3) return 2;
  FILE *f = fopen(argv[1], "rb"), *o = fopen(argv[2], "wb");
  if (!f || !o) return 1;
  int64_t hdr[4];
  double th[2];
  if (fread(hdr, sizeof(int64_t), 4, f) != 4 || fread(th, sizeof(double), 2, f) != 2) return 1;
  const int64_t H = hdr[0], W = hdr[1], B = hdr[2];
  if (H < 2 || W < 2 || B < 1 || hdr[3] < 0) return 1;
  const size_t px = (size_t)(H * W);
  std::vector<float> dlr(px * B), drl(px * B), fl(px * B * 4), fr(px * B * 4);
  if (fread(dlr.data(), sizeof(float), dlr.size(), f) != dlr.size()) return 1;
  if (fread(drl.data(), sizeof(float), drl.size(), f) != drl.size()) return 1;
  if (fread(fl.data(), sizeof(float), fl.size(), f) != fl.size()) return 1;
  if (fread(fr.data(), sizeof(float), fr.size(), f) != fr.size()) return 1;
  const int64_t N = hdr[3] ? hdr[3] : H * W;
  std::vector<double> xy0((size_t)(2 * N));
  if (hdr[3]) {
    if (fread(xy0.data(), sizeof(double), xy0.size(), f) != xy0.size()) return 1;
  } else {
    for (int64_t i = 0; i < N; ++i) {
      xy0[2 * i] = (double)(i % W);
      xy0[2 * i + 1] = (double)(i / W);
    }
  }
  std::vector<StMem> lr, rl, lf, lb, rf, rb;
  for (int64_t k = 0; k < B; ++k) {
    lr.push_back(StMem{dlr.data() + px * k, (int)W, (int)H, 1, 0, -1.0});  // the script's -imgs_d[fr][0]
    rl.push_back(StMem{drl.data() + px * k, (int)W, (int)H, 1, 0, 1.0});
    lf.push_back(StMem{fl.data() + px * 2 * (2 * k), (int)W, (int)H, 2, 0, 1.0});
    lb.push_back(StMem{fl.data() + px * 2 * (2 * k + 1), (int)W, (int)H, 2, 0, 1.0});
    rf.push_back(StMem{fr.data() + px * 2 * (2 * k), (int)W, (int)H, 2, 0, 1.0});
    rb.push_back(StMem{fr.data() + px * 2 * (2 * k + 1), (int)W, (int)H, 2, 0, 1.0});
  }
  std::vector<int64_t> rows;
  std::vector<double> out, row((size_t)(4 * B));
  for (int64_t i = 0; i < N; ++i) {
    if (!st_track_host(lr.data(), rl.data(), lf.data(), lb.data(), rf.data(), rb.data(), (int)B, xy0[2 * i], xy0[2 * i + 1],
                       th[0], th[1], row.data()))
      continue;
    rows.push_back(i);
    out.insert(out.end(), row.begin(), row.end());
  }
  const int64_t M = (int64_t)rows.size();
  fwrite(&M, sizeof(M), 1, o);
  fwrite(rows.data(), sizeof(int64_t), rows.size(), o);
  fwrite(out.data(), sizeof(double), out.size(), o);
  fclose(f);
  fclose(o);
  return 0;
}
