// Host caller of csrc/ictr_ba_hd.h (BaHost) as plain C++. Used by tests/test_bundle_cpu.py, built with -ffp-contract=off
// and the address / undefined-behaviour sanitizers.
//   bundle_hd_host in.bin out.bin
// in.bin:  int64 N, F, S, has_mask, noiter; f64 fx, fy, cx, cy, damp_init, damp_fct, minres, maxdamp, offset[3];
//          f64 X[3][N], xy[S][F][2][N], G0[F][12]; uint64 words[ceil(N / 64)] when has_mask
// out.bin: f64, with dim = 6 (F - 1): the system at G0 and damp_init: n, cost, nfail, A[dim (dim + 1) / 2], rhs[dim],
//          V[6][N], gp[3][N]; its solve: ok, dc[dim]; the update by that step: Gt[F][12], Xt[3][N] (zeros when the solve
//          failed); the whole run: G[F][12], X[3][N], cost, damp, iters, status, n
#include <cstdint>
#include <cstdio>
#include <vector>

#include "ictr_ba_hd.h"

using namespace ictr;

static void put(FILE *o, const std::vector<double> &v) { fwrite(v.data(), sizeof(double), v.size(), o); }
static void put(FILE *o, double v) { fwrite(&v, sizeof(double), 1, o); }

int main(int argc, char **argv) {
  if (argc != 3) return 2;
  FILE *f = fopen(argv[1], "rb"), *o = fopen(argv[2], "wb");
  if (!f || !o) return 1;
  int64_t hdr[5];
  double par[11];
  if (fread(hdr, sizeof(int64_t), 5, f) != 5 || fread(par, sizeof(double), 11, f) != 11) return 1;
  const int64_t N = hdr[0];
  const int F = (int)hdr[1], S = (int)hdr[2];
  if (N < 1 || F < 2 || F > kBaMaxFrames || S < 1 || S > 2) return 1;
  std::vector<double> X((size_t)(3 * N)), xy((size_t)(2 * S * F * N)), G0((size_t)(12 * F));
  std::vector<unsigned long long> words((size_t)((N + 63) / 64));
  if (fread(X.data(), sizeof(double), X.size(), f) != X.size()) return 1;
  if (fread(xy.data(), sizeof(double), xy.size(), f) != xy.size()) return 1;
  if (fread(G0.data(), sizeof(double), G0.size(), f) != G0.size()) return 1;
  if (hdr[3] && fread(words.data(), sizeof(unsigned long long), words.size(), f) != words.size()) return 1;
  const CfCam cam = {par[0], par[1], par[2], par[3]};
  const CfParams prm = {(int)hdr[4], par[4], par[5], par[6], par[7]};
  const int dim = 6 * (F - 1);

  BaHost h;
  h.setup(X.data(), xy.data(), hdr[3] ? words.data() : nullptr, N, F, S, cam, par + 8);
  ba_init(h.st, G0.data(), F, prm);
  h.point_pass(h.st.Gt, 0);
  h.frame_pass(h.st.Gt, 0);
  ba_decide(h.st, h.fsums.data(), F, S, prm);
  put(o, (double)h.st.n);
  put(o, h.st.c);
  // the system whatever ba_decide made of the start
  std::vector<double> U((size_t)(21 * F)), gc((size_t)(6 * F));
  for (int fr = 0; fr < F; ++fr) {
    for (int q = 0; q < 21; ++q) U[(size_t)(21 * fr + q)] = h.fsums[(size_t)(kCfSlots * fr + q)];
    for (int q = 0; q < 6; ++q) gc[(size_t)(6 * fr + q)] = h.fsums[(size_t)(kCfSlots * fr + 21 + q)];
  }
  h.schur_pass(G0.data(), 0, prm.damp_init);
  h.assemble(U.data(), gc.data(), prm.damp_init);
  put(o, (double)h.nfail);
  put(o, h.A);
  put(o, h.rhs);
  put(o, h.V[0]);
  put(o, h.gp[0]);
  std::vector<double> dc((size_t)dim, 0.0), Gt((size_t)(12 * F), 0.0), Xt((size_t)(3 * N), 0.0);
  const bool ok = h.reduced_solve(dc.data());
  put(o, ok ? 1.0 : 0.0);
  if (!ok) dc.assign((size_t)dim, 0.0);
  put(o, dc);
  if (ok) {
    for (int q = 0; q < 12; ++q) Gt[(size_t)q] = G0[(size_t)q];
    for (int fr = 1; fr < F; ++fr) cf_update(G0.data() + 12 * fr, dc.data() + 6 * (fr - 1), Gt.data() + 12 * fr);
    h.back_pass(G0.data(), 0, 1, prm.damp_init, dc.data());
    Xt = h.X[1];
  }
  put(o, Gt);
  put(o, Xt);

  BaHost r;
  r.setup(X.data(), xy.data(), hdr[3] ? words.data() : nullptr, N, F, S, cam, par + 8);
  r.run(G0.data(), prm);
  put(o, std::vector<double>(r.st.G, r.st.G + 12 * F));
  put(o, r.X[r.st.cur]);
  put(o, r.st.c);
  put(o, r.st.damp);
  put(o, (double)r.st.it);
  put(o, (double)r.st.status);
  put(o, (double)r.st.n);
  fclose(f);
  fclose(o);
  return 0;
}
