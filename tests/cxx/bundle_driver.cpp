// C++ caller of CTR::BundleClass (include/ctr_shim.hpp). Used by the tests.
//   bundle_driver in.bin noiter minres
// in.bin:  int64 N, F, S, has_mask; f64 fc[2], cc[2], offset[3]; f64 X[3][N], xy[S][F][2][N], G0[F][12]; uint64
//          words[ceil(N / 64)] when has_mask
// stdout:  the lines of python -m invcompcamtrack_amd.run_bundle byte for byte, every number as a hexadecimal float
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
  int64_t hdr[4];
  double par[7];
  if (!f || fread(hdr, sizeof(int64_t), 4, f) != 4 || fread(par, sizeof(double), 7, f) != 7 || hdr[0] < 8 ||
      hdr[0] > (1 << 22) || hdr[1] < 2 || hdr[1] > 32 || hdr[2] < 1 || hdr[2] > 2) {
    fprintf(stderr, "%s: cannot read the header\n", argv[1]);
    return 1;
  }
  const int64_t N = hdr[0], F = hdr[1], S = hdr[2];
  std::vector<double> X((size_t)(3 * N)), xy((size_t)(2 * S * F * N)), G0((size_t)(12 * F));
  std::vector<uint64_t> words((size_t)((N + 63) / 64));
  if (fread(X.data(), sizeof(double), X.size(), f) != X.size() || fread(xy.data(), sizeof(double), xy.size(), f) != xy.size() ||
      fread(G0.data(), sizeof(double), G0.size(), f) != G0.size() ||
      (hdr[3] && fread(words.data(), sizeof(uint64_t), words.size(), f) != words.size())) {
    fprintf(stderr, "%s: truncated\n", argv[1]);
    return 1;
  }
  fclose(f);
  const int noiter = atoi(argv[2]);
  const double minres = strtod(argv[3], nullptr);
  try {
    BundleClass ba(N, F, S);
    ba.SetPoints(X.data());
    ba.SetObservations(xy.data());
    ba.SetCamera(par, par + 2);
    ba.SetOffset(par + 4);
    ba.SetMask(hdr[3] ? words.data() : nullptr);
    ba.Run(G0.data(), noiter, 2.0, 10.0, minres);
    std::vector<double> G((size_t)(12 * F)), Xo((size_t)(3 * N));
    double cost = 0, damp = 0;
    int32_t iters = 0, status = 0;
    int64_t n = 0;
    ba.Wait(G.data(), Xo.data(), &cost, &damp, &iters, &status, &n);
    printf("status %d iters %d n %lld cost %a damp %a\n", status, iters, (long long)n, cost, damp);
    for (int64_t k = 0; k < F; ++k) {
      printf("G %lld:", (long long)k);
      for (int q = 0; q < 12; ++q) printf(" %a", G[(size_t)(12 * k + q)]);
      printf("\n");
    }
    for (int64_t m = 0; m < N; ++m)
      printf("X %lld: %a %a %a\n", (long long)m, Xo[(size_t)m], Xo[(size_t)(N + m)], Xo[(size_t)(2 * N + m)]);
  } catch (const std::exception &e) {
    fprintf(stderr, "%s\n", e.what());
    return 1;
  }
  return 0;
}
