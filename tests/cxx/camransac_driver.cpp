// C++ caller of CTR::CamRansacClass and CTR::CamFitClass (include/ctr_shim.hpp). Used by the tests.
//   camransac_driver in.bin ntrials thresh seed
// in.bin:  int64 N, F, S, has_mask; f64 fc[2], cc[2], offset[3]; f64 X[3][N], xy[S][F][2][N]; uint64 words[ceil(N / 64)]
//          when has_mask
// stdout:  "best_trial T best_count C draws a b c d", then per frame "frame k G <12 hex floats> p <6 hex floats>" of the
//          winner, "words <hex words>", "dd <N hex floats>", and per frame "fit k status s iters i G <12 hex floats>" of
//          the camera fit started from the winner's poses on its inlier words (handed over on the device)
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "ctr_shim.hpp"

using namespace CTR;

int main(int argc, char **argv) {
  if (argc != 5) {
    fprintf(stderr, "usage: %s in.bin ntrials thresh seed\n", argv[0]);
    return 2;
  }
  FILE *f = fopen(argv[1], "rb");
  int64_t hdr[4];
  double cam[7];
  if (!f || fread(hdr, sizeof(int64_t), 4, f) != 4 || fread(cam, sizeof(double), 7, f) != 7 || hdr[0] < 4 ||
      hdr[0] > (1 << 22) || hdr[1] < 1 || hdr[1] > 64 || hdr[2] < 1 || hdr[2] > 2) {
    fprintf(stderr, "%s: cannot read the header\n", argv[1]);
    return 1;
  }
  const int64_t N = hdr[0], F = hdr[1], S = hdr[2], W = (N + 63) / 64;
  std::vector<double> X((size_t)(3 * N)), xy((size_t)(2 * S * F * N));
  std::vector<uint64_t> mask((size_t)W);
  if (fread(X.data(), sizeof(double), X.size(), f) != X.size() || fread(xy.data(), sizeof(double), xy.size(), f) != xy.size() ||
      (hdr[3] && fread(mask.data(), sizeof(uint64_t), mask.size(), f) != mask.size())) {
    fprintf(stderr, "%s: truncated\n", argv[1]);
    return 1;
  }
  fclose(f);
  const int64_t ntrials = atoll(argv[2]);
  const double thresh = strtod(argv[3], nullptr);
  const uint64_t seed = strtoull(argv[4], nullptr, 10);
  try {
    CamRansacClass ran(N, F, S);
    ran.SetPoints(X.data());
    ran.SetObservations(xy.data());
    ran.SetCamera(cam, cam + 2);
    if (S == 2) ran.SetOffset(cam + 4);
    ran.SetMask(hdr[3] ? mask.data() : nullptr);
    ran.Run(ntrials, thresh, seed);
    CamFitClass fit(N, F);
    fit.SetPoints(X.data());
    fit.SetObservations(xy.data());  // side 0 comes first
    fit.SetCamera(cam, cam + 2);
    fit.SetMaskFromRansac(ran);      // while the run is in flight
    int64_t best[2];
    int32_t draws[4];
    std::vector<double> G((size_t)(12 * F)), p((size_t)(6 * F)), dd((size_t)N);
    std::vector<uint64_t> words((size_t)W);
    ran.Wait(&best[0], &best[1], draws, G.data(), p.data(), words.data(), dd.data());
    printf("best_trial %lld best_count %lld draws %d %d %d %d\n", (long long)best[0], (long long)best[1], draws[0], draws[1],
           draws[2], draws[3]);
    for (int64_t k = 0; k < F; ++k) {
      printf("frame %lld G", (long long)k);
      for (int q = 0; q < 12; ++q) printf(" %a", G[(size_t)(12 * k + q)]);
      printf(" p");
      for (int q = 0; q < 6; ++q) printf(" %a", p[(size_t)(6 * k + q)]);
      printf("\n");
    }
    printf("words");
    for (int64_t w = 0; w < W; ++w) printf(" %016" PRIx64, words[(size_t)w]);
    printf("\ndd");
    for (int64_t m = 0; m < N; ++m) printf(" %a", dd[(size_t)m]);
    printf("\n");
    if (best[0] >= 0) {
      fit.Run(G.data());
      std::vector<double> Gf((size_t)(12 * F));
      std::vector<int32_t> iters((size_t)F), status((size_t)F);
      fit.Wait(Gf.data(), nullptr, nullptr, iters.data(), status.data(), nullptr);
      for (int64_t k = 0; k < F; ++k) {
        printf("fit %lld status %d iters %d G", (long long)k, status[(size_t)k], iters[(size_t)k]);
        for (int q = 0; q < 12; ++q) printf(" %a", Gf[(size_t)(12 * k + q)]);
        printf("\n");
      }
    }
  } catch (const std::exception &e) {
    fprintf(stderr, "%s\n", e.what());
    return 1;
  }
  return 0;
}
