// Host caller of csrc/ictr_camransac_hd.h (cr_counts, cr_trial_host) and csrc/ictr_p3p_hd.h (p3p_lambda_twist) as plain
// C++. Used by tests/test_camransac_cpu.py, built with -ffp-contract=off and the address / undefined-behaviour sanitizers.
//   camransac_hd_host run in.bin out.bin
// in.bin:  int64 N, F, S, has_mask, ntrials, seed; f64 fx, fy, cx, cy, off[3], thresh; f64 X[3][N], xy[S][F][2][N];
//          uint64 words[ceil(N / 64)] when has_mask
// out.bin: per trial int64 status, draws[4], cnt; f64 G[F][12], dd[N]; uint64 words[ceil(N / 64)]. Then int64 best_trial,
//          best_count (the largest count among the successful trials, the lowest trial on ties; -1, 0 without one).
//   camransac_hd_host p3p in.bin out.bin
// in.bin:  int64 ncases; per case f64 y[3][3] (unit bearings), x[3][3] (world points)
// out.bin: per case int64 nsol; f64 [4][12]: R (9), T (3) of every solution in the order found, zeros beyond nsol
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "ictr_camransac_hd.h"

using namespace ictr;

static int run(FILE *f, FILE *o) {
  int64_t hdr[6];
  double par[8];
  if (fread(hdr, sizeof(int64_t), 6, f) != 6 || fread(par, sizeof(double), 8, f) != 8) return 1;
  const int64_t N = hdr[0], F = hdr[1], S = hdr[2], W = (N + 63) / 64, T = hdr[4];
  if (N < 4 || F < 1 || F > kCrMaxFrames || S < 1 || S > 2 || T < 1) return 1;
  std::vector<double> X((size_t)(3 * N)), xy((size_t)(2 * S * F * N));
  std::vector<unsigned long long> mask((size_t)W), cw((size_t)W, 0ull), words((size_t)W);
  if (fread(X.data(), sizeof(double), X.size(), f) != X.size()) return 1;
  if (fread(xy.data(), sizeof(double), xy.size(), f) != xy.size()) return 1;
  if (hdr[3] && fread(mask.data(), sizeof(unsigned long long), mask.size(), f) != mask.size()) return 1;
  const CfCam cam = {par[0], par[1], par[2], par[3]};
  for (int64_t m = 0; m < N; ++m) {
    const bool bit = hdr[3] ? cr_bit(mask.data(), m) : true;
    if (cr_counts(bit, X.data(), xy.data(), N, (int)F, (int)S, m)) cw[(size_t)(m >> 6)] |= 1ull << (m & 63);
  }
  const unsigned long long seedmix = ran_seed((unsigned long long)hdr[5]);
  std::vector<double> G((size_t)(12 * F)), dd((size_t)N);
  int64_t best[2] = {-1, 0};
  for (int64_t g = 0; g < T; ++g) {
    int idx[4];
    long long cnt = 0;
    const int st = cr_trial_host(seedmix, g, X.data(), xy.data(), cw.data(), N, (int)F, (int)S, cam, par + 4, par[7], idx,
                                 G.data(), &cnt, dd.data(), words.data());
    const int64_t rec[6] = {st, idx[0], idx[1], idx[2], idx[3], cnt};
    fwrite(rec, sizeof(int64_t), 6, o);
    fwrite(G.data(), sizeof(double), G.size(), o);
    fwrite(dd.data(), sizeof(double), dd.size(), o);
    fwrite(words.data(), sizeof(unsigned long long), words.size(), o);
    if (st && (best[0] < 0 || cnt > best[1])) {
      best[0] = g;
      best[1] = cnt;
    }
  }
  fwrite(best, sizeof(int64_t), 2, o);
  return 0;
}

static int p3p(FILE *f, FILE *o) {
  int64_t ncases;
  if (fread(&ncases, sizeof(int64_t), 1, f) != 1 || ncases < 0) return 1;
  for (int64_t c = 0; c < ncases; ++c) {
    double y[3][3], x[3][3], out[4][12];
    if (fread(y, sizeof(double), 9, f) != 9 || fread(x, sizeof(double), 9, f) != 9) return 1;
    memset(out, 0, sizeof(out));
    int64_t nsol = 0;
    p3p_lambda_twist(y, x, [&](const double *R, const double *T) {
      if (nsol < 4) {
        for (int k = 0; k < 9; ++k) out[nsol][k] = R[k];
        for (int k = 0; k < 3; ++k) out[nsol][9 + k] = T[k];
      }
      ++nsol;
    });
    fwrite(&nsol, sizeof(int64_t), 1, o);
    fwrite(out, sizeof(double), 48, o);
  }
  return 0;
}

int main(int argc, char **argv) {
  if (argc != 4) return 2;
  FILE *f = fopen(argv[2], "rb"), *o = fopen(argv[3], "wb");
  if (!f || !o) return 1;
  const int rc = strcmp(argv[1], "p3p") == 0 ? p3p(f, o) : run(f, o);
  fclose(f);
  fclose(o);
  return rc;
}
