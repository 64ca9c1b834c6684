// ictr_flowgrid_dev.h -- the flow grid as a kernel reads it: the node table of an ictr_flowgrid (FgDev), dense_flow's field
// at an integer pixel (fg_value) and func_get_transf_position on that field (fg_gather), which is never formed. Stated once
// for the kernels of ictr_frontend.hip (k_fg_gather, k_fg_dense, k_pt_advance) and of ictr_stereotrack.hip (the grid kind
// of a field descriptor).
#pragma once

#include <hip/hip_runtime.h>

struct ictr_flowgrid;

namespace ictr {

struct FgDev {
  const float *d;  // [ny][nx][2] node displacements after the fill
  int nx, ny, step, w, h;
};

// dense_flow's field at the integer pixel (X, Y), component c: the bilinear blend of the four surrounding nodes
__device__ __forceinline__ void fg_value(const FgDev &g, int X, int Y, float *u, float *v) {
  const int half = g.step / 2;
  const double fx = fmin(fmax((double)(X - half) / (double)g.step, 0.0), (double)(g.nx - 1));
  const double fy = fmin(fmax((double)(Y - half) / (double)g.step, 0.0), (double)(g.ny - 1));
  const double flx = floor(fx), fly = floor(fy);
  const int x0 = (int)flx, y0 = (int)fly;
  const int x1 = min(x0 + 1, g.nx - 1), y1 = min(y0 + 1, g.ny - 1);
  const double ax = fx - flx, ay = fy - fly;
  const float2 *d = reinterpret_cast<const float2 *>(g.d);
  const float2 a = d[y0 * g.nx + x0], b = d[y0 * g.nx + x1], c = d[y1 * g.nx + x0], e = d[y1 * g.nx + x1];
  const double topu = (double)a.x * (1 - ax) + (double)b.x * ax, botu = (double)c.x * (1 - ax) + (double)e.x * ax;
  const double topv = (double)a.y * (1 - ax) + (double)b.y * ax, botv = (double)c.y * (1 - ax) + (double)e.y * ax;
  *u = (float)(topu * (1 - ay) + botu * ay);
  *v = (float)(topv * (1 - ay) + botv * ay);
}

// func_get_transf_position(xy, F[:, :, 0], F[:, :, 1]) with F = the dense field of the grid, never formed
__device__ __forceinline__ void fg_gather(const FgDev &g, double x, double y, double *ox, double *oy) {
  const double flx = floor(x), fly = floor(y);
  const double nan = __builtin_nan("");
  *ox = nan;
  *oy = nan;
  // NaN / out-of-range coordinates fail the range test (written positively), like the INT_MIN cast in NumPy
  if (flx >= 0.0 && fly >= 0.0 && flx + 1.0 < (double)g.w && fly + 1.0 < (double)g.h) {
    const int x0 = (int)flx, y0 = (int)fly;
    const double fx = x - flx, fy = y - fly;
    const double w0 = fx * fy, w1 = (1 - fx) * fy, w2 = fx * (1 - fy), w3 = (1 - fx) * (1 - fy);
    float u11, v11, u01, v01, u10, v10, u00, v00;
    fg_value(g, x0 + 1, y0 + 1, &u11, &v11);
    fg_value(g, x0, y0 + 1, &u01, &v01);
    fg_value(g, x0 + 1, y0, &u10, &v10);
    fg_value(g, x0, y0, &u00, &v00);
    *ox = x + ((double)u11 * w0 + (double)u01 * w1 + (double)u10 * w2 + (double)u00 * w3);
    *oy = y + ((double)v11 * w0 + (double)v01 * w1 + (double)v10 * w2 + (double)v00 * w3);
  }
}

}  // namespace ictr

// the node table of a grid that holds a field; non-zero (with its message): NULL, or no field yet (ictr_frontend.hip)
extern "C" int ictr_flowgrid_view_(const ictr_flowgrid *g, ictr::FgDev *v);
// the same with the lost mask [ny][nx] (1: the node was lost and v->d holds its filled value), for k_densify
extern "C" int ictr_flowgrid_view_lost_(const ictr_flowgrid *g, ictr::FgDev *v, const unsigned char **lost);
// the dense field of a grid, interleaved [h][w][2], into device memory: k_fg_dense on s (ictr_frontend.hip)
namespace ictr {
void launch_fg_dense(const FgDev &g, float2 *out, hipStream_t s);
}
