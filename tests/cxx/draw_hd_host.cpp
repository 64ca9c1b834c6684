// Host caller of csrc/ictr_draw_hd.h (ran_seed, ran_draw<4>, ran_draw<8>) as plain C++. Used by tests/test_fsplit_cpu.py,
// built with the address / undefined-behaviour sanitizers.
//   draw_hd_host in.bin out.bin
// in.bin:  records of 4 x 64 bits: seed (u64), trial, n, K (i64; K = 4 or 8)
// out.bin: per record 10 x 64 bits: ran_seed(seed), ran_draw's return value, idx[8] (-1 beyond K)
#include <cstdint>
#include <cstdio>

#include "ictr_draw_hd.h"

int main(int argc, char **argv) {
  if (argc != 3) return 2;
  FILE *f = fopen(argv[1], "rb"), *o = fopen(argv[2], "wb");
  if (!f || !o) return 1;
  int64_t s[4];
  while (fread(s, sizeof(int64_t), 4, f) == 4) {
    const unsigned long long sm = ictr::ran_seed((unsigned long long)s[0]);
    int idx[8] = {-1, -1, -1, -1, -1, -1, -1, -1};
    int64_t r[10];
    if (s[3] == 4) r[1] = ictr::ran_draw<4>(sm, s[1], (int)s[2], idx);
    else if (s[3] == 8) r[1] = ictr::ran_draw<8>(sm, s[1], (int)s[2], idx);
    else return 3;
    r[0] = (int64_t)sm;
    for (int q = 0; q < 8; ++q) r[2 + q] = idx[q];
    fwrite(r, sizeof(int64_t), 10, o);
  }
  fclose(f);
  fclose(o);
  return 0;
}
