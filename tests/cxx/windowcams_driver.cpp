// C++ caller of the window hand-over (CTR::StereoTrackClass, StaticSplitClass, CamFitClass of include/ctr_shim.hpp):
// fields in, one camera per frame out, the window never leaves the device. Used by the tests.
//   windowcams_driver in.bin
// in.bin: int64 H, W, bsize, N (0: every pixel in meshgrid order); f64 th_ratio, th_abs; f32 disp_lr[bsize][H][W],
//         disp_rl[bsize][H][W], flow_l[bsize][2][H][W][2] (fwd, bwd), flow_r likewise; f64 xy0[N][2] when N > 0 (the file of
//         tests/cxx/stereotrack_driver.cpp); then f64 fc[2], cc[2], baseline, thresh; int64 ntrials, seed
// stdout: "kept M best_trial T best_count C", then per frame "frame f status s iters i n n G <12 hex floats> err <left>
//         <right>" (hex floats: every bit)
#include <cstdint>
#include <cstdio>
#include <vector>

#include "ctr_shim.hpp"

using namespace CTR;

int main(int argc, char **argv) {
  if (argc != 2) {
    fprintf(stderr, "usage: %s in.bin\n", argv[0]);
    return 2;
  }
  FILE *f = fopen(argv[1], "rb");
  int64_t hdr[4];
  double th[2];
  if (!f || fread(hdr, sizeof(int64_t), 4, f) != 4 || fread(th, sizeof(double), 2, f) != 2 || hdr[0] < 2 || hdr[0] > 32768 ||
      hdr[1] < 2 || hdr[1] > 32768 || hdr[2] < 2 || hdr[2] > 65 || hdr[3] < 0 || hdr[3] > (1 << 24)) {
    fprintf(stderr, "%s: cannot read the header\n", argv[1]);
    return 1;
  }
  const int64_t H = hdr[0], W = hdr[1], B = hdr[2], N = hdr[3];
  const size_t px = (size_t)(H * W);
  std::vector<float> dlr(px * B), drl(px * B), fl(px * B * 4), fr(px * B * 4);
  std::vector<double> xy0((size_t)(2 * N));
  double prm[6];  // fc, cc, baseline, thresh
  int64_t run[2];  // ntrials, seed
  if (fread(dlr.data(), sizeof(float), dlr.size(), f) != dlr.size() || fread(drl.data(), sizeof(float), drl.size(), f) != drl.size() ||
      fread(fl.data(), sizeof(float), fl.size(), f) != fl.size() || fread(fr.data(), sizeof(float), fr.size(), f) != fr.size() ||
      (N && fread(xy0.data(), sizeof(double), xy0.size(), f) != xy0.size()) || fread(prm, sizeof(double), 6, f) != 6 ||
      fread(run, sizeof(int64_t), 2, f) != 2) {
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
    StaticSplitClass split(M, 2 * (B / 2));
    CamFitClass fit(M, B);
    split.SetPairsFromWindow(win);
    split.Run(run[0], prm[5], (uint64_t)run[1]);
    fit.SetCamera(prm, prm + 2);
    fit.SetPointsFromWindow(win, prm[4]);
    fit.SetObservationsFromWindow(win, false);
    fit.SetMaskFromSplit(split);
    std::vector<double> G0((size_t)(12 * B), 0.0), G((size_t)(12 * B)), el((size_t)B), er((size_t)B);
    for (int64_t k = 0; k < B; ++k) G0[12 * k] = G0[12 * k + 5] = G0[12 * k + 10] = 1.0;
    fit.Run(G0.data());
    int64_t best[2];
    split.Wait(&best[0], &best[1], nullptr, nullptr, nullptr, nullptr);
    std::vector<int32_t> iters((size_t)B), status((size_t)B);
    std::vector<int64_t> n((size_t)B);
    fit.Wait(G.data(), nullptr, nullptr, iters.data(), status.data(), n.data());
    fit.Reproject(G.data(), nullptr, el.data());
    fit.SetObservationsFromWindow(win, true);
    const double dt[3] = {prm[4], 0.0, 0.0};
    fit.Reproject(G.data(), dt, er.data());
    printf("kept %lld best_trial %lld best_count %lld\n", (long long)M, (long long)best[0], (long long)best[1]);
    for (int64_t k = 0; k < B; ++k) {
      printf("frame %lld status %d iters %d n %lld G", (long long)k, status[k], iters[k], (long long)n[k]);
      for (int q = 0; q < 12; ++q) printf(" %a", G[12 * k + q]);
      printf(" err %a %a\n", el[k], er[k]);
    }
  } catch (const std::exception &e) {
    fprintf(stderr, "%s\n", e.what());
    return 1;
  }
  return 0;
}
