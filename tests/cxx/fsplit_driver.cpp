// C++ caller of CTR::StaticSplitClass (include/ctr_shim.hpp). Used by the tests.
//   fsplit_driver in.bin out.bin ntrials thresh seed
// in.bin:  int64 P, int64 N, f64 [P][4][N] (per pair the rows xa, ya, xb, yb)
// out.bin: int64 best_trial, int64 best_count, int32 draws[8], f64 F[P][9], uint64 words[ceil(N / 64)], f64 dd[N]
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "ctr_shim.hpp"

using namespace CTR;

int main(int argc, char **argv) {
  if (argc != 6) {
    fprintf(stderr, "usage: %s in.bin out.bin ntrials thresh seed\n", argv[0]);
    return 2;
  }
  FILE *f = fopen(argv[1], "rb");
  int64_t hdr[2];
  if (!f || fread(hdr, sizeof(int64_t), 2, f) != 2 || hdr[0] < 1 || hdr[0] > 64 || hdr[1] < 8 || hdr[1] > (1 << 22)) {
    fprintf(stderr, "%s: cannot read the header\n", argv[1]);
    return 1;
  }
  const int64_t P = hdr[0], N = hdr[1];
  std::vector<double> xy((size_t)(4 * P * N));
  if (fread(xy.data(), sizeof(double), xy.size(), f) != xy.size()) {
    fprintf(stderr, "%s: truncated\n", argv[1]);
    return 1;
  }
  fclose(f);
  const long long ntrials = atoll(argv[3]);
  const double thresh = strtod(argv[4], nullptr);
  const uint64_t seed = strtoull(argv[5], nullptr, 10);
  try {
    StaticSplitClass sp(N, P);
    sp.SetPairs(xy.data());
    sp.Run(ntrials, thresh, seed);
    int64_t best[2];
    int32_t draws[8];
    std::vector<double> F((size_t)(9 * P)), dd((size_t)N);
    std::vector<uint64_t> words((size_t)sp.Words());
    sp.Wait(&best[0], &best[1], draws, F.data(), words.data(), dd.data());
    FILE *o = fopen(argv[2], "wb");
    if (!o) return 1;
    fwrite(best, sizeof(int64_t), 2, o);
    fwrite(draws, sizeof(int32_t), 8, o);
    fwrite(F.data(), sizeof(double), F.size(), o);
    fwrite(words.data(), sizeof(uint64_t), words.size(), o);
    fwrite(dd.data(), sizeof(double), dd.size(), o);
    fclose(o);
  } catch (const std::exception &e) {
    fprintf(stderr, "%s\n", e.what());
    return 1;
  }
  return 0;
}
