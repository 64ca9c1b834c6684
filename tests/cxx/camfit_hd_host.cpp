// Host caller of csrc/ictr_camfit_hd.h (cf_pass_host, cf_solve, cf_update, cf_fit_host) as plain C++. Used by
// tests/test_camfit_cpu.py, built with -ffp-contract=off and the address / undefined-behaviour sanitizers.
//   camfit_hd_host in.bin out.bin
// in.bin:  int64 N, F, has_mask, noiter; f64 fx, fy, cx, cy, damp_init, damp_fct, minres, maxdamp; f64 X[3][N],
//          xy[F][2][N], G0[F][12]; uint64 words[ceil(N / 64)] when has_mask
// out.bin: per frame 68 f64: the pass at G0 (32 slots); cf_solve of its H, b at damp_init (ok, x[6]); cf_update of G0 by
//          that x (12); the whole fit: G[12], cost, damp, iters, status, n
#include <cstdint>
#include <cstdio>
#include <vector>

#include "ictr_camfit_hd.h"

using namespace ictr;

int main(int argc, char **argv) {
  if (argc != 3) return 2;
  FILE *f = fopen(argv[1], "rb"), *o = fopen(argv[2], "wb");
  if (!f || !o) return 1;
  int64_t hdr[4];
  double par[8];
  if (fread(hdr, sizeof(int64_t), 4, f) != 4 || fread(par, sizeof(double), 8, f) != 8) return 1;
  const int64_t N = hdr[0], F = hdr[1];
  if (N < 1 || F < 1) return 1;
  std::vector<double> X((size_t)(3 * N)), xy((size_t)(2 * F * N)), G0((size_t)(12 * F));
  std::vector<unsigned long long> words((size_t)((N + 63) / 64));
  if (fread(X.data(), sizeof(double), X.size(), f) != X.size()) return 1;
  if (fread(xy.data(), sizeof(double), xy.size(), f) != xy.size()) return 1;
  if (fread(G0.data(), sizeof(double), G0.size(), f) != G0.size()) return 1;
  if (hdr[2] && fread(words.data(), sizeof(unsigned long long), words.size(), f) != words.size()) return 1;
  const unsigned long long *w = hdr[2] ? words.data() : nullptr;
  const CfCam cam = {par[0], par[1], par[2], par[3]};
  const CfParams prm = {(int)hdr[3], par[4], par[5], par[6], par[7]};
  for (int64_t fr = 0; fr < F; ++fr) {
    double r[68];
    const double *g0 = G0.data() + 12 * fr, *obs = xy.data() + 2 * N * fr;
    cf_pass_host(g0, nullptr, cam, X.data(), obs, w, N, r);
    r[32] = cf_solve(r, r + 21, prm.damp_init, r + 33) ? 1.0 : 0.0;
    cf_update(g0, r + 33, r + 39);
    CfState s;
    cf_fit_host(g0, cam, prm, X.data(), obs, w, N, s);
    for (int q = 0; q < 12; ++q) r[51 + q] = s.G[q];
    r[63] = s.c;
    r[64] = s.damp;
    r[65] = (double)s.it;
    r[66] = (double)s.status;
    r[67] = (double)s.n;
    fwrite(r, sizeof(double), 68, o);
  }
  fclose(f);
  fclose(o);
  return 0;
}
