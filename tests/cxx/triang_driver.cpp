// C++ caller of CTR::TriangClass (include/ctr_shim.hpp), file-compatible with python -m invcompcamtrack_amd.run_triangulate.
// Used by the tests.
//   triang_driver in.txt out.txt mode        mode: dlt | gn | lm | depth
// Reads the track file (format: invcompcamtrack_amd/run_triangulate.py), triangulates on the GPU and writes one line per
// point: X Y Z, the covariance (9 numbers; depth: 1), the iteration count, the status word.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "ctr_shim.hpp"

using namespace CTR;

static std::string fmt(float v) {
  if (std::isnan(v)) return "nan";
  char b[64];
  snprintf(b, sizeof(b), "%.9g", (double)v);
  return b;
}

int main(int argc, char **argv) {
  if (argc != 4) {
    fprintf(stderr, "usage: %s in.txt out.txt dlt|gn|lm|depth\n", argv[0]);
    return 2;
  }
  const char *names[4] = {"dlt", "gn", "lm", "depth"};
  int mode = -1;
  for (int k = 0; k < 4; ++k)
    if (!strcmp(argv[3], names[k])) mode = k;
  if (mode < 0) {
    fprintf(stderr, "unknown mode %s\n", argv[3]);
    return 2;
  }
  std::ifstream in(argv[1]);
  std::vector<std::vector<std::string>> lines;
  for (std::string ln; std::getline(in, ln);) {
    std::istringstream s(ln);
    std::vector<std::string> tok;
    for (std::string t; s >> t;) tok.push_back(t);
    if (!tok.empty()) lines.push_back(tok);
  }
  size_t li = 0;
  auto next = [&](size_t need) -> const std::vector<std::string> & {
    if (li >= lines.size() || lines[li].size() < need) {
      fprintf(stderr, "%s: truncated\n", argv[1]);
      exit(1);
    }
    return lines[li++];
  };
  auto num = [](const std::string &s) { return (float)strtod(s.c_str(), nullptr); };  // as Python: f64, then narrowed
  const long long F = atoll(next(1)[0].c_str());
  std::vector<float> P(12 * F);
  for (long long i = 0; i < F; ++i) {
    const auto &t = next(12);
    for (int k = 0; k < 12; ++k) P[12 * i + k] = num(t[k]);
  }
  const long long n = atoll(next(1)[0].c_str());
  std::vector<int64_t> off(1, 0);
  std::vector<int32_t> view;
  std::vector<float> x, y;
  for (long long i = 0; i < n; ++i) {
    const auto &t0 = next(1);
    const long long L = atoll(t0[0].c_str());
    if (L < 0 || t0.size() < (size_t)(1 + 3 * L)) {
      fprintf(stderr, "%s: a track line announces %lld observations and holds fewer\n", argv[1], L);
      return 1;
    }
    for (long long k = 0; k < L; ++k) {
      view.push_back((int32_t)atoll(t0[1 + 3 * k].c_str()));
      x.push_back(num(t0[2 + 3 * k]));
      y.push_back(num(t0[3 + 3 * k]));
    }
    off.push_back((int64_t)view.size());
  }
  ictr_triang_params prm;
  {
    const auto &t = next(5);
    prm.noiter = atoi(t[0].c_str());
    prm.minres = num(t[1]);
    prm.damp_init = num(t[2]);
    prm.damp_fct = num(t[3]);
    prm.maxdamp = num(t[4]);
  }
  int has_init, has_rays;
  {
    const auto &t = next(2);
    has_init = atoi(t[0].c_str());
    has_rays = atoi(t[1].c_str());
  }
  std::vector<float> init, campos, ptdir;
  if (has_init)
    for (long long i = 0; i < n; ++i) {
      const auto &t = next(3);
      for (int k = 0; k < 3; ++k) init.push_back(num(t[k]));
    }
  if (has_rays)
    for (long long i = 0; i < n; ++i) {
      const auto &t = next(6);
      for (int k = 0; k < 3; ++k) campos.push_back(num(t[k]));
      for (int k = 0; k < 3; ++k) ptdir.push_back(num(t[3 + k]));
    }
  if (mode == ICTR_TRIANG_DEPTH && !has_rays) {
    fprintf(stderr, "the depth-only mode needs the rays section of the input\n");
    return 2;
  }
  try {
    TriangClass tr(n > 0 ? n : 1, std::max<long long>(2 * n, (long long)view.size()), F);
    tr.SetCameras(P.data(), F);
    tr.SetTracks(n, off.data(), view.data(), x.data(), y.data());
    std::vector<float> pts(3 * n), cov(9 * n);
    std::vector<int32_t> iters(n), status(n);
    if (mode != ICTR_TRIANG_DLT && !has_init) {  // an iterative mode without start points: from the DLT points
      tr.Run(ICTR_TRIANG_DLT);
      tr.Wait(pts.data(), nullptr);
      init = pts;
    }
    tr.Run(mode, &prm, mode == ICTR_TRIANG_DLT ? nullptr : init.data(), has_rays ? campos.data() : nullptr,
           has_rays ? ptdir.data() : nullptr);
    tr.Wait(pts.data(), cov.data(), iters.data(), status.data());
    FILE *f = fopen(argv[2], "w");
    if (!f) return 1;
    const int ncov = mode == ICTR_TRIANG_DEPTH ? 1 : 9;
    for (long long i = 0; i < n; ++i) {
      std::string s = fmt(pts[3 * i]) + " " + fmt(pts[3 * i + 1]) + " " + fmt(pts[3 * i + 2]);
      for (int k = 0; k < ncov; ++k) s += " " + fmt(cov[9 * i + k]);
      fprintf(f, "%s %d %d\n", s.c_str(), (int)iters[i], (int)status[i]);
    }
    fclose(f);
  } catch (const std::exception &e) {
    fprintf(stderr, "%s\n", e.what());
    return 1;
  }
  return 0;
}
