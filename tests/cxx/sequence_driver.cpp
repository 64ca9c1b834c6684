// C++ caller of CTR::SequenceClass (include/ctr_shim.hpp), argv- and file-compatible with
// python -m invcompcamtrack_amd.run_track_sequence. Used by the tests.
//   sequence_driver listfile infile outfile lv_f lv_l psz maxiter normdp_ratio donorm dopatchnorm maxpttrack stride
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "ctr_shim.hpp"

using namespace CTR;

// binary 8-bit PGM (P5) -> f32 grey levels
static bool read_pgm(const char *fn, std::vector<float> &out, int &w, int &h) {
  FILE *f = fopen(fn, "rb");
  if (!f) return false;
  char magic[3] = {0, 0, 0};
  int maxv = 0;
  bool ok = fscanf(f, "%2s", magic) == 1 && strcmp(magic, "P5") == 0;
  int vals[3], got = 0;
  while (ok && got < 3) {
    int c = fgetc(f);
    if (c == '#') {
      while (c != '\n' && c != EOF) c = fgetc(f);
    } else if (c >= '0' && c <= '9') {
      ungetc(c, f);
      ok = fscanf(f, "%d", &vals[got++]) == 1;
    } else if (c == EOF) {
      ok = false;
    }
  }
  if (ok) fgetc(f);  // the single whitespace after maxval
  w = vals[0];
  h = vals[1];
  maxv = vals[2];
  ok = ok && maxv > 0 && maxv < 256;
  std::vector<unsigned char> px(ok ? (size_t)w * h : 0);
  ok = ok && fread(px.data(), 1, px.size(), f) == px.size();
  fclose(f);
  if (!ok) return false;
  out.resize(px.size());
  for (size_t i = 0; i < px.size(); ++i) out[i] = (float)px[i];
  return true;
}

int main(int argc, char **argv) {
  if (argc != 13) {
    fprintf(stderr, "usage: see source\n");
    return 2;
  }
  optparam op;
  ictr_optparam_init(&op, atoi(argv[4]), atoi(argv[5]), atoi(argv[6]), atoi(argv[7]), (float)atof(argv[8]),
                     atoi(argv[9]), atoi(argv[10]), atoi(argv[11]), 0);
  const int stride = atoi(argv[12]);
  // frames, in list order
  std::vector<float> frames;
  int64_t n = 0;
  int w = 0, h = 0;
  {
    FILE *lf = fopen(argv[1], "r");
    if (!lf) return 2;
    char line[4096];
    while (fgets(line, sizeof(line), lf)) {
      std::string s(line);
      while (!s.empty() && (s.back() == '\n' || s.back() == '\r' || s.back() == ' ')) s.pop_back();
      if (s.empty()) continue;
      std::vector<float> img;
      int wi, hi;
      if (!read_pgm(s.c_str(), img, wi, hi) || (n > 0 && (wi != w || hi != h))) {
        fprintf(stderr, "cannot read %s\n", s.c_str());
        return 2;
      }
      w = wi;
      h = hi;
      frames.insert(frames.end(), img.begin(), img.end());
      ++n;
    }
    fclose(lf);
  }
  // the point/cam file of run_io_reprojection_test (run_io_reprojection_test.cpp:54-79), without its point cap
  FILE *f = fopen(argv[2], "rb");
  if (!f) return 2;
  double p0[6];
  float fc[2], cc[2];
  uint32_t whu[2];
  uint64_t nw;
  if (fread(p0, 8, 6, f) != 6 || fread(fc, 4, 2, f) != 2 || fread(cc, 4, 2, f) != 2 || fread(whu, 4, 2, f) != 2 ||
      fread(&nw, 8, 1, f) != 1)
    return 2;
  std::vector<double> pt3d(3 * nw);
  if (fread(pt3d.data(), 8, 3 * nw, f) != 3 * nw) return 2;
  fclose(f);
  const int wh[2] = {(int)whu[0], (int)whu[1]};
  try {
    CamClass cam(op.lv_f + 1, fc, cc, wh, op.psz);
    SequenceClass seq(&cam, &op, (int64_t)nw, stride);
    seq.SetPoints(pt3d.data());
    seq.SetFrames(frames.data(), n, w, h);
    seq.TrackAsync(p0);
    std::vector<double> poses(6 * n);
    seq.Wait(poses.data());
    FILE *o = fopen(argv[3], "wb");
    if (!o || fwrite(poses.data(), 8, poses.size(), o) != poses.size()) return 2;
    fclose(o);
  } catch (const std::exception &e) {
    fprintf(stderr, "%s\n", e.what());
    return 1;
  }
  return 0;
}
