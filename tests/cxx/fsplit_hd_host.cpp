// Host caller of csrc/ictr_fsplit_hd.h (fs_fit8, fs_dist) as plain C++. Used by tests/test_fsplit_cpu.py, built with
// -ffp-contract=off and the address / undefined-behaviour sanitizers.
//   fsplit_hd_host in.bin out.bin
// in.bin:  records of 32 f64: xa[8] ya[8] xb[8] yb[8]
// out.bin: per record 11 f64: F[9], the fit's return value (0 / 1), fs_dist of the record's first correspondence
#include <cstdio>

#include "ictr_fsplit_hd.h"

int main(int argc, char **argv) {
  if (argc != 3) return 2;
  FILE *f = fopen(argv[1], "rb"), *o = fopen(argv[2], "wb");
  if (!f || !o) return 1;
  double s[32];
  while (fread(s, sizeof(double), 32, f) == 32) {
    double r[11];
    r[9] = ictr::fs_fit8(s, s + 8, s + 16, s + 24, r) ? 1.0 : 0.0;
    r[10] = ictr::fs_dist(r, s[0], s[8], s[16], s[24]);
    fwrite(r, sizeof(double), 11, o);
  }
  fclose(f);
  fclose(o);
  return 0;
}
