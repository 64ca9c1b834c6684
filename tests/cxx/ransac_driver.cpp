// C++ caller of CTR::RansacClass (include/ctr_shim.hpp), file-compatible with python -m invcompcamtrack_amd.run_ransac
// (without --track). Used by the tests.
//   ransac_driver in.txt out.txt nsamples maxtrials inlthresh kc seed
// Reads a run_track_nposes input file (its sample section is ignored), draws the pose samples on the GPU and writes the
// same file with them filled in.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "ctr_shim.hpp"

using namespace CTR;

int main(int argc, char **argv) {
  if (argc != 8) {
    fprintf(stderr, "usage: %s in.txt out.txt nsamples maxtrials inlthresh kc seed\n", argv[0]);
    return 2;
  }
  std::ifstream in(argv[1]);
  std::vector<std::string> lines;
  for (std::string ln; std::getline(in, ln);)
    if (ln.find_first_not_of(" \t\r") != std::string::npos) lines.push_back(ln);
  size_t li = 0;
  auto next = [&]() -> std::istringstream {
    if (li >= lines.size()) {
      fprintf(stderr, "%s: truncated\n", argv[1]);
      exit(1);
    }
    return std::istringstream(lines[li++]);
  };
  int lv_f, lv_l, psz, maxiter, donorm, dopatchnorm, maxpt, verbosity;
  double ratio;
  next() >> lv_f >> lv_l >> psz >> maxiter >> ratio >> donorm >> dopatchnorm >> maxpt >> verbosity;
  float fcf[2], ccf[2];
  int wh[2];
  next() >> fcf[0] >> fcf[1] >> ccf[0] >> ccf[1] >> wh[0] >> wh[1];
  int nback, nfwd;
  next() >> nback >> nfwd;
  std::vector<std::string> files;
  for (int i = 0; i < nback + nfwd + 1; ++i) {
    std::string f;
    next() >> f;
    files.push_back(f);
  }
  long long n = 0;
  next() >> n;
  std::vector<double> pt2d(2 * n), pt3d(3 * n);  // SoA
  for (long long i = 0; i < n; ++i) {
    std::istringstream s = next();
    std::string tok[5];
    for (auto &t : tok) s >> t;
    pt2d[i] = strtod(tok[0].c_str(), nullptr);
    pt2d[n + i] = strtod(tok[1].c_str(), nullptr);
    for (int k = 0; k < 3; ++k) pt3d[k * n + i] = strtod(tok[2 + k].c_str(), nullptr);
  }
  const long long nsamples = atoll(argv[3]), maxtrials = atoll(argv[4]);
  const double thr = strtod(argv[5], nullptr), kc = strtod(argv[6], nullptr);
  const uint64_t seed = strtoull(argv[7], nullptr, 10);
  const double fc[2] = {fcf[0], fcf[1]}, cc[2] = {ccf[0], ccf[1]};
  try {
    RansacClass r(n, nsamples);
    r.SetPoints(pt2d.data(), pt3d.data());
    r.Run(fc, cc, kc, nsamples, maxtrials, thr, seed);
    const int64_t W = r.WordsPerSample();
    int64_t counts[4];
    std::vector<double> R(9 * nsamples), t(3 * nsamples), p(6 * nsamples);
    std::vector<uint64_t> words(W * nsamples);
    std::vector<int32_t> cnt(n);
    r.Wait(counts, R.data(), t.data(), p.data(), words.data(), cnt.data());
    FILE *f = fopen(argv[2], "w");
    if (!f) return 1;
    fprintf(f, "%d %d %d %d %g %d %d %d %d\n", lv_f, lv_l, psz, maxiter, ratio, donorm, dopatchnorm, maxpt, verbosity);
    fprintf(f, "%.9g %.9g %.9g %.9g %d %d\n", fcf[0], fcf[1], ccf[0], ccf[1], wh[0], wh[1]);
    fprintf(f, "%d %d\n", nback, nfwd);
    for (auto &s : files) fprintf(f, "%s\n", s.c_str());
    fprintf(f, "%lld\n", n);
    for (long long i = 0; i < n; ++i)
      fprintf(f, "%.17g %.17g %.17g %.17g %.17g\n", pt2d[i], pt2d[n + i], pt3d[i], pt3d[n + i], pt3d[2 * n + i]);
    fprintf(f, "%lld\n", (long long)counts[0]);
    for (int64_t s = 0; s < counts[0]; ++s) {
      std::vector<long long> ids;
      for (long long j = 0; j < n; ++j)
        if ((words[s * W + j / 64] >> (j % 64)) & 1ull) ids.push_back(j + 1);
      for (int k = 0; k < 6; ++k) fprintf(f, k ? " %.17g" : "%.17g", p[s * 6 + k]);
      fprintf(f, " %zu ", ids.size());
      for (size_t k = 0; k < ids.size(); ++k) fprintf(f, k ? " %lld" : "%lld", ids[k]);
      fprintf(f, "\n");
    }
    fclose(f);
  } catch (const std::exception &e) {
    fprintf(stderr, "%s\n", e.what());
    return 1;
  }
  return 0;
}
