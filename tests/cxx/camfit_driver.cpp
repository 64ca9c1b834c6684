// C++ caller of CTR::CamFitClass (include/ctr_shim.hpp). Used by the tests.
//   camfit_driver in.bin noiter minres
// in.bin:  int64 N, F, has_mask; f64 fc[2], cc[2]; f64 X[3][N], xy[F][2][N], G0[F][12]; uint64 words[ceil(N / 64)] when
//          has_mask
// stdout:  one line per frame, the lines of python -m invcompcamtrack_amd.run_fit_cameras byte for byte
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "ctr_shim.hpp"

using namespace CTR;

int main(int argc, char **argv) {
  if (argc != 4) {
    fprintf(stderr, "usage: %s in.bin noiter minres\n", argv[0]);
    return 2;
  }
  FILE *f = fopen(argv[1], "rb");
  int64_t hdr[3];
  double cam[4];
  if (!f || fread(hdr, sizeof(int64_t), 3, f) != 3 || fread(cam, sizeof(double), 4, f) != 4 || hdr[0] < 1 ||
      hdr[0] > (1 << 22) || hdr[1] < 1 || hdr[1] > 4096) {
    fprintf(stderr, "%s: cannot read the header\n", argv[1]);
    return 1;
  }
  const int64_t N = hdr[0], F = hdr[1];
  std::vector<double> X((size_t)(3 * N)), xy((size_t)(2 * F * N)), G0((size_t)(12 * F));
  std::vector<uint64_t> words((size_t)((N + 63) / 64));
  if (fread(X.data(), sizeof(double), X.size(), f) != X.size() || fread(xy.data(), sizeof(double), xy.size(), f) != xy.size() ||
      fread(G0.data(), sizeof(double), G0.size(), f) != G0.size() ||
      (hdr[2] && fread(words.data(), sizeof(uint64_t), words.size(), f) != words.size())) {
    fprintf(stderr, "%s: truncated\n", argv[1]);
    return 1;
  }
  fclose(f);
  const int noiter = atoi(argv[2]);
  const double minres = strtod(argv[3], nullptr);
  try {
    CamFitClass fit(N, F);
    fit.SetPoints(X.data());
    fit.SetObservations(xy.data());
    fit.SetCamera(cam, cam + 2);
    fit.SetMask(hdr[2] ? words.data() : nullptr);
    fit.Run(G0.data(), noiter, 2.0, 10.0, minres);
    std::vector<double> G((size_t)(12 * F)), cost((size_t)F), damp((size_t)F), err((size_t)F);
    std::vector<int32_t> iters((size_t)F), status((size_t)F);
    std::vector<int64_t> n((size_t)F);
    fit.Wait(G.data(), cost.data(), damp.data(), iters.data(), status.data(), n.data());
    fit.Reproject(G.data(), nullptr, err.data());
    for (int64_t k = 0; k < F; ++k) {
      printf("frame %lld: status %d iters %d n %lld cost %.17g damp %.17g reproj %.17g G", (long long)k, status[(size_t)k],
             iters[(size_t)k], (long long)n[(size_t)k], cost[(size_t)k], damp[(size_t)k], err[(size_t)k]);
      for (int q = 0; q < 12; ++q) printf(" %.17g", G[(size_t)(12 * k + q)]);
      printf("\n");
    }
  } catch (const std::exception &e) {
    fprintf(stderr, "%s\n", e.what());
    return 1;
  }
  return 0;
}
