// ictr_draw_hd.h -- the counter-based draw stream of the RANSAC stages, stated once: the mixer, the seed as the kernels
// take it and the distinct indices of one trial. The same text compiles for the device (k_ransac_hyp and k_cr_hyp: 4 matches,
// k_fsplit_fit: 8 points), for the host code that fills the kernels' seed and, as plain C++ under sanitizers, for
// tests/cxx/draw_hd_host.cpp (tests/test_fsplit_cpu.py); invcompcamtrack_amd/_hostmath.py restates it. Integers only.
#pragma once

#include "se3_math.h"

namespace ictr {

constexpr int kRanMaxDraws = 1024;  // draws per trial before it counts as failed (N >= K: never reached in practice)

ICTR_HD unsigned long long ran_mix(unsigned long long z) {  // splitmix64
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// the caller's seed as the kernels take it (RansacArgs::seedmix, FsplitArgs::seedmix)
ICTR_HD unsigned long long ran_seed(unsigned long long seed) { return ran_mix(seed); }

// Trial g over n items: draw k is u_k = ran_mix(seedmix ^ (g << 32 | k)), its index (u_k >> 32) * n >> 32; repeats are
// skipped. idx gets the first K distinct indices in draw order, -1 where kRanMaxDraws draws gave none; returns how many
// were drawn. idx is indexed by constants of fully unrolled loops only, so that it stays in registers.
template <int K>
ICTR_HD int ran_draw(unsigned long long seedmix, long long g, int n, int *idx) {
#pragma unroll
  for (int q = 0; q < K; ++q) idx[q] = -1;
  int nd = 0;
  for (int k = 0; k < kRanMaxDraws && nd < K; ++k) {
    const unsigned long long u = ran_mix(seedmix ^ (((unsigned long long)g << 32) | (unsigned long long)k));
    const int id = (int)(((u >> 32) * (unsigned long long)n) >> 32);
    bool dup = false;
#pragma unroll
    for (int q = 0; q < K; ++q) dup = dup || idx[q] == id;
    if (dup) continue;
#pragma unroll
    for (int q = 0; q < K; ++q) idx[q] = nd == q ? id : idx[q];
    ++nd;
  }
  return nd;
}

}  // namespace ictr
