// ictr_c2fflow.hip -- coarse-to-fine dense flow (DESIGN.md §4 "Coarse-to-fine dense flow"): per pyramid level a patch
// search on a grid of the level's own size, started from the coarser level's dense field, then the flow grid's fill, the
// densification and (optionally) the variational refinement on the level's planes. The rule is build-defined; its
// statement of record is patchflow.c2f_flow_host (NumPy, f64). This file is the same rule in f32 with one fixed operation
// order, restated in NumPy f32 by tests/c2fflow_f32.py.
//
// k_c2f_level<NPL, WPP>, one launch per level: a wave (two for patches of more than 4 pixels per lane) per node, in
// k_patchflow's forms and two-wave exchange. What FlowGrid.compute spends three launches on is one here: the node position
// follows from the node index, the start is ONE 8-byte load of the coarser field (times 2: exact), the search at this
// level alone is k_patchflow's (pf_level_search of ictr_patchflow_dev.h: a node's step is the same f32 value as a
// k_patchflow step at the same position), then the hold rules, and the node's displacement, lost byte and status byte
// written directly. f32 throughout, plain vector loads and stores, no atomics.
//
// MEAN is patch-mean normalisation (DESIGN.md "Patch-mean normalisation"): the search removes the patch means
// (pf_level_search<.., MEAN>), and the kernel's tail takes every voting node's brightness offset, beta = mean(B at the
// node's final position) - mean(T), with one more window pass (pf_window_sum), into the level's bias table; a node that is
// lost or whose final position is out of view gets +0.0. restated by tests/patnorm_f32.py.
//
// XONLY is the 1-D form for rectified stereo pairs (DESIGN.md "The 1-D form"): the start is the x component of the coarser
// field alone (ONE 4-byte load), the search is pf_level_search's XONLY rule at this level (min_det then carries min_hx),
// the rejection is scalar, the MEAN tail stays in the node's row, and a node's y displacement is +0.0 to the bit.
// Restated by tests/c2fdisp_f32.py.
//
// NCH = 3 is the colour form (DESIGN.md "Colour"): a frame is three pyramids of one geometry, the search is
// pf_level_search_ch over three channel planes (H and b summed over the channels, one decision and one step per node), the
// MEAN tail writes three betas per node, and a level's densifier and refiner runs take the three pyramids per frame
// (k_densify<BIAS, 3>, k_fr_warp<3>, k_fr_coef_rgb). Restated by tests/c2frgb_f32.py.
//
// ROBUST is the Huber patch cost (DESIGN.md "Robust patch cost"): pf_level_search_ch's ROBUST forms, every residual clipped
// to [-huber_k, +huber_k]; nothing else of the kernel changes. k_c2f_level, its arguments and its launcher live in
// ictr_c2fflow_dev.h; this file instantiates the L2 forms and ictr_c2fflow_robust.hip the ROBUST ones, which
// launch_c2f_level_robust reaches. Restated by tests/c2fcost_f32.py.
//
// k_flow_upsample<XONLY> finishes a run whose finest level is above 0 (DESIGN.md "A finest level above 0"): the field of
// level lv to the w x h frame, bilinear with half-pixel centres at the fixed factor 2^-lv, the vectors times 2^lv. One lane
// per output pixel, a wave per 64 consecutive columns of a row and kWaves rows per workgroup, so that a workgroup's source
// taps are two or three rows' worth of at most 34 records; one whole float2 store per lane, 512 contiguous bytes per wave.
// No LDS, no atomics. Restated by tests/c2fup_f32.py; the definition is patchflow.upsample_flow_host.
#include <math.h>
#include <string.h>

#include <memory>
#include <type_traits>
#include <vector>

#include "ictr_dev.h"
#include "ictr_launch.h"
#include "ictr_devfn.h"
#include "ictr_patchflow_dev.h"
#include "ictr_c2fflow_dev.h"

namespace ictr {

// s = 2^lv, inv_s = 2^-lv. Everything before the taps is exact in f32 (x + 0.5, the product with 2^-lv, - 0.5, rx,
// 1 - rx); the six products and three sums are taken in the order written, each rounded (no contraction), then s * val.
template <bool XONLY>
__global__ __launch_bounds__(kBlock) void k_flow_upsample(const float2 *__restrict__ src, int wl, int hl, float inv_s,
                                                          float s, float2 *__restrict__ out, int w, int h) {
  const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * kWaves + (threadIdx.x >> 6);
  if (x >= w || y >= h) return;
  const float fx = fminf(fmaxf(((float)x + 0.5f) * inv_s - 0.5f, 0.0f), (float)(wl - 1));
  const float fy = fminf(fmaxf(((float)y + 0.5f) * inv_s - 0.5f, 0.0f), (float)(hl - 1));
  const int x0 = (int)fx, y0 = (int)fy;  // fx, fy >= 0: the cast is the floor
  const int x1 = min(x0 + 1, wl - 1), y1 = min(y0 + 1, hl - 1);
  const float rx = fx - (float)x0, ry = fy - (float)y0;
  const float qx = 1.0f - rx, qy = 1.0f - ry;
  const size_t r0 = (size_t)y0 * wl, r1 = (size_t)y1 * wl;
  float2 o;
  if constexpr (XONLY) {  // y is not read and is +0.0
    const float *f = reinterpret_cast<const float *>(src);
    const float top = qx * f[2 * (r0 + x0)] + rx * f[2 * (r0 + x1)];
    const float bot = qx * f[2 * (r1 + x0)] + rx * f[2 * (r1 + x1)];
    o.x = s * (qy * top + ry * bot);
    o.y = 0.0f;
  } else {
    const float2 a = src[r0 + x0], b = src[r0 + x1], c = src[r1 + x0], d = src[r1 + x1];
    const float tx = qx * a.x + rx * b.x, bx = qx * c.x + rx * d.x;
    const float ty = qx * a.y + rx * b.y, by = qx * c.y + rx * d.y;
    o.x = s * (qy * tx + ry * bx);
    o.y = s * (qy * ty + ry * by);
  }
  out[(size_t)y * w + x] = o;
}

// src [hl][wl][2] and out [h][w][2] on the device; the caller has checked the sizes
static void launch_flow_upsample(const float *src, int wl, int hl, int lv, float *out, int w, int h, int x_only,
                                 hipStream_t s) {
  const float sc = (float)(1 << lv), inv = 1.0f / sc;
  const dim3 g = pixel_rows_grid(w, h), blk(kBlock);
  if (x_only)
    hipLaunchKernelGGL((k_flow_upsample<true>), g, blk, 0, s, reinterpret_cast<const float2 *>(src), wl, hl, inv, sc,
                       reinterpret_cast<float2 *>(out), w, h);
  else
    hipLaunchKernelGGL((k_flow_upsample<false>), g, blk, 0, s, reinterpret_cast<const float2 *>(src), wl, hl, inv, sc,
                       reinterpret_cast<float2 *>(out), w, h);
}

}  // namespace ictr

using namespace ictr;

// ---------------------------------------------------------------- C-ABI
namespace {
struct GridDel {
  void operator()(ictr_flowgrid *p) const { ictr_flowgrid_destroy(p); }
};
struct DensDel {
  void operator()(ictr_flowdensify *p) const { ictr_flowdensify_destroy(p); }
};
struct RefDel {
  void operator()(ictr_flowrefine *p) const { ictr_flowrefine_destroy(p); }
};
struct C2fLevel {
  int w = 0, h = 0, nx = 0, ny = 0;
  unsigned char *status = nullptr;  // [ny][nx], in the object's status block
  float *bias = nullptr;            // [ny][nx][channels], in the object's bias block
  std::unique_ptr<ictr_flowgrid, GridDel> grid;
  std::unique_ptr<ictr_flowdensify, DensDel> dens;
  std::unique_ptr<ictr_flowrefine, RefDel> ref;  // made when the refinement is switched on
  Event ev[4];                                    // before the search, after the fill, the densifier, the refiner
};
}  // namespace

struct ictr_c2fflow {
  int w = 0, h = 0, lv_f = 0, lv_l = 0, step = 0, psz = 0;
  int maxiter = 10;
  float eps = 0.01f;
  int refine = 0;  // refiners exist for every level and hold their parameters
  int patnorm = 0;
  int x_only = 0;  // the 1-D form: the XONLY kernels and the refinement along x
  int channels = 1;  // 3: colour frames, three pyramids per frame (ictr_c2fflow_run_rgb)
  int cost = ICTR_C2F_COST_L2;  // ICTR_C2F_COST_HUBER: the ROBUST kernels with huber_k
  float huber_k = 5.0f;
  int timing = 0, timed = 0, ran = 0, ran_refined = 0, ran_patnorm = 0;
  std::vector<C2fLevel> lv;  // [lv_f + 1]; the levels below lv_l hold their size and nothing else
  DevBuf<unsigned char> status;
  DevBuf<float> bias;  // next to it: the node bias of a run with patch-mean normalisation
  DevBuf<float> bw12;  // two planes of the finest level's size, the refinement's Bw of channels 1 and 2: made by the first
                       // refined run of a 3-channel object
  DevBuf<float> up;    // lv_l > 0: the result plane [h][w][2], level lv_l's field up-sampled
  Event up_done;       // behind k_flow_upsample in a timed run (it starts at level lv_l's last event)
  Event done;  // behind the last run
};

// the field a level hands on: the refiner's when the run refined, else the densifier's
static const float *c2f_field(const C2fLevel &L, int refined) {
  return refined ? ictr_flowrefine_device_ptr(L.ref.get()) : ictr_flowdensify_device_ptr(L.dens.get());
}

// the w x h result: level 0's field, or the result plane of an object whose finest level is above 0
static const float *c2f_result(const ictr_c2fflow *c, int refined) {
  return c->lv_l > 0 ? c->up.get() : c2f_field(c->lv[0], refined);
}

// the bias block for `channels` channels: per level [ny][nx][channels] floats, the levels one behind the other from 0. The
// new block is allocated first; on failure the object keeps its block, its rows and its channel count.
static int c2f_place_bias(ictr_c2fflow *c, int channels) {
  size_t nodes = 0;
  for (const C2fLevel &L : c->lv) nodes += (size_t)L.nx * L.ny;
  DevBuf<float> block;
  if (int rc = block.alloc(sizeof(float) * nodes * (size_t)channels, true)) return rc;
  c->bias = std::move(block);
  float *cur = c->bias.get();
  for (C2fLevel &L : c->lv) {
    L.bias = cur;
    cur += (size_t)L.nx * L.ny * (size_t)channels;
  }
  c->channels = channels;
  return ICTR_OK;
}

extern "C" void ictr_c2fflow_destroy(ictr_c2fflow *c) {
  if (c && c->ran) (void)hipEventSynchronize(c->done.get());  // before any buffer of a run in flight is released
  delete c;
}
extern "C" int ictr_c2fflow_create(ictr_c2fflow **out, int w, int h, int lv_f, int step, int psz) {
  return ictr_c2fflow_create_lvl(out, w, h, lv_f, 0, step, psz);
}
extern "C" int ictr_c2fflow_create_lvl(ictr_c2fflow **out, int w, int h, int lv_f, int lv_l, int step, int psz) {
  if (!out || w < 1 || h < 1 || lv_f < 0 || lv_f > 15 || step < 1)
    return fail(ICTR_ERR_INVALID, "c2fflow: bad arguments (w, h, step >= 1, 0 <= lv_f <= 15)");
  if (psz < 1 || psz > 32) return fail(ICTR_ERR_INVALID, "c2fflow: psz is %d (1 .. 32)", psz);
  if (lv_l < 0 || lv_l > lv_f) return fail(ICTR_ERR_INVALID, "c2fflow: lv_l is %d (0 .. lv_f = %d)", lv_l, lv_f);
  if (int rc = need_device()) return rc;
  auto c = std::make_unique<ictr_c2fflow>();
  c->w = w;
  c->h = h;
  c->lv_f = lv_f;
  c->lv_l = lv_l;
  c->step = step;
  c->psz = psz;
  c->lv.resize((size_t)lv_f + 1);
  size_t nodes = 0;
  for (int l = 0; l <= lv_f; ++l) {
    C2fLevel &L = c->lv[l];
    pyramid_level_size(w, h, l, &L.w, &L.h);
    if (l < lv_l) continue;
    if (L.w < 2 || L.h < 2) return fail(ICTR_ERR_INVALID, "c2fflow: level %d is %d x %d, smaller than 2 px", l, L.w, L.h);
    if (step / 2 >= L.w || step / 2 >= L.h)
      return fail(ICTR_ERR_INVALID, "c2fflow: level %d (%d x %d) has no node at step %d", l, L.w, L.h, step);
    ictr_flowgrid *g = nullptr;
    if (int rc = ictr_flowgrid_create(&g, L.w, L.h, step)) return rc;
    L.grid.reset(g);
    if (int rc = ictr_flowgrid_dims(g, &L.nx, &L.ny)) return rc;
    ictr_flowdensify *z = nullptr;
    if (int rc = ictr_flowdensify_create(&z, L.w, L.h)) return rc;
    L.dens.reset(z);
    for (Event &e : L.ev)
      if (int rc = e.create()) return rc;
    nodes += (size_t)L.nx * L.ny;
  }
  if (int rc = c->status.alloc(nodes, true)) return rc;
  unsigned char *cur = c->status.get();
  for (C2fLevel &L : c->lv) {  // (a level below lv_l has no nodes)
    L.status = cur;
    cur += (size_t)L.nx * L.ny;
  }
  if (int rc = c2f_place_bias(c.get(), 1)) return rc;
  if (lv_l > 0) {
    if (int rc = c->up.alloc(sizeof(float) * 2 * (size_t)w * h, true)) return rc;
    if (int rc = c->up_done.create()) return rc;
  }
  if (int rc = c->done.create(hipEventDisableTiming)) return rc;
  *out = c.release();
  return ICTR_OK;
}
extern "C" int ictr_c2fflow_set_params(ictr_c2fflow *c, int maxiter, float eps, float minerr, int power) {
  if (!c) return fail(ICTR_ERR_INVALID, "c2fflow is NULL");
  if (maxiter < 0 || !isfinite(eps) || eps < 0.0f)
    return fail(ICTR_ERR_INVALID, "c2fflow_set_params: maxiter >= 0, finite eps >= 0");
  for (int l = c->lv_l; l <= c->lv_f; ++l)
    if (int rc = ictr_flowdensify_set_params(c->lv[l].dens.get(), minerr, power)) return rc;
  c->maxiter = maxiter;
  c->eps = eps;
  return ICTR_OK;
}
extern "C" int ictr_c2fflow_set_refine(ictr_c2fflow *c, int on, float alpha, float gamma, float delta, int n_outer,
                                       int n_sor, float omega) {
  if (!c) return fail(ICTR_ERR_INVALID, "c2fflow is NULL");
  if (!on) {
    c->refine = 0;
    return ICTR_OK;
  }
  for (size_t l = (size_t)c->lv_l; l < c->lv.size(); ++l)
    if (c->lv[l].w < 4 || c->lv[l].h < 4)
      return fail(ICTR_ERR_INVALID, "c2fflow_set_refine: level %d is %d x %d, the refinement needs 4 x 4", (int)l, c->lv[l].w,
                  c->lv[l].h);
  for (int l = c->lv_l; l <= c->lv_f; ++l) {
    C2fLevel &L = c->lv[l];
    if (!L.ref) {
      ictr_flowrefine *r = nullptr;
      if (int rc = ictr_flowrefine_create(&r, L.w, L.h)) return rc;
      L.ref.reset(r);
    }
    if (int rc = ictr_flowrefine_set_params(L.ref.get(), alpha, gamma, delta, n_outer, n_sor, omega)) return rc;
  }
  c->refine = 1;
  return ICTR_OK;
}
extern "C" int ictr_c2fflow_set_patnorm(ictr_c2fflow *c, int on) {
  if (!c) return fail(ICTR_ERR_INVALID, "c2fflow is NULL");
  c->patnorm = on ? 1 : 0;
  return ICTR_OK;
}
extern "C" int ictr_c2fflow_set_x_only(ictr_c2fflow *c, int on) {
  if (!c) return fail(ICTR_ERR_INVALID, "c2fflow is NULL");
  c->x_only = on ? 1 : 0;
  return ICTR_OK;
}
extern "C" int ictr_c2fflow_get_x_only(const ictr_c2fflow *c, int *on) {
  if (!c || !on) return fail(ICTR_ERR_INVALID, "c2fflow_get_x_only: c2fflow or on is NULL");
  *on = c->x_only;
  return ICTR_OK;
}
extern "C" int ictr_c2fflow_set_cost(ictr_c2fflow *c, int cost, float huber_k) {
  if (!c) return fail(ICTR_ERR_INVALID, "c2fflow is NULL");
  if (cost == 1)
    return fail(ICTR_ERR_INVALID,
                "c2fflow_set_cost: cost 1 (L1) is not built: with H fixed its influence sign(r) has no scale; use "
                "ICTR_C2F_COST_HUBER (2) with a small huber_k");
  if (cost != ICTR_C2F_COST_L2 && cost != ICTR_C2F_COST_HUBER)
    return fail(ICTR_ERR_INVALID, "c2fflow_set_cost: cost is %d (0: L2, or 2: Huber)", cost);
  if (!(huber_k > 0.0f) || !isfinite(huber_k))
    return fail(ICTR_ERR_INVALID, "c2fflow_set_cost: huber_k must be finite and > 0");
  c->cost = cost;
  c->huber_k = huber_k;
  return ICTR_OK;
}
extern "C" int ictr_c2fflow_get_cost(const ictr_c2fflow *c, int *cost, float *huber_k) {
  if (!c || !cost || !huber_k) return fail(ICTR_ERR_INVALID, "c2fflow_get_cost: c2fflow, cost or huber_k is NULL");
  *cost = c->cost;
  *huber_k = c->huber_k;
  return ICTR_OK;
}
extern "C" int ictr_c2fflow_set_timing(ictr_c2fflow *c, int on) {
  if (!c) return fail(ICTR_ERR_INVALID, "c2fflow is NULL");
  c->timing = on ? 1 : 0;
  return ICTR_OK;
}

// level l's search of a run: pfc[ch] the level tables of the channels' pyramids, which agree in geometry
template <bool MEAN, bool XONLY, int NCH, bool ROBUST>
static int c2f_search(const ictr_c2fflow *c, const PFArgs *pfc, int l, int refined, hipStream_t s) {
  const C2fLevel &L = c->lv[l];
  const PFArgs &pf = pfc[0];
  C2fArgsOf<MEAN, NCH, ROBUST> a;
  memset(&a, 0, sizeof(a));
  for (int ch = 0; ch < NCH; ++ch)
    a.a[ch] = pfc[ch].lv[l].a, a.ax[ch] = pfc[ch].lv[l].ax, a.ay[ch] = pfc[ch].lv[l].ay, a.b[ch] = pfc[ch].lv[l].b;
  a.sw = pf.lv[l].sw;
  a.shift = pf.lv[l].shift;
  a.swo = pf.lv[l].swo;
  a.sho = pf.lv[l].sho;
  a.nx = L.nx;
  a.K = L.nx * L.ny;
  a.step = c->step;
  if (l < c->lv_f) {
    a.coarse = reinterpret_cast<const float2 *>(c2f_field(c->lv[l + 1], refined));
    a.cw = c->lv[l + 1].w;
    a.ch = c->lv[l + 1].h;
  }
  a.P = c->psz;
  a.maxiter = c->maxiter;
  a.eps2 = pf.eps2;
  a.min_det = XONLY ? pf.min_hx : pf.min_det;
  a.far2 = (float)(c->psz * c->psz);
  if (int rc = ictr_flowgrid_node_buffers_(L.grid.get(), &a.d, &a.lost)) return rc;
  a.status = L.status;
  if constexpr (MEAN) a.bias = L.bias;
  if constexpr (ROBUST) a.huber_k = c->huber_k;
  if (c->timed) HIPCHK(hipEventRecord(L.ev[0].get(), s));
  if constexpr (ROBUST)
    launch_c2f_level_robust(a, XONLY, s);  // (instantiated in ictr_c2fflow_robust.hip)
  else
    launch_c2f_level<MEAN, XONLY, NCH, false>(a, s);
  return ICTR_OK;
}
// the search's form by [cost == Huber][patnorm][x_only][channels == 3]
using C2fSearch = int (*)(const ictr_c2fflow *, const PFArgs *, int, int, hipStream_t);
#define ICTR_C2F_FORMS(R)                                                                                                  \
  {                                                                                                                        \
    {{c2f_search<false, false, 1, R>, c2f_search<false, false, 3, R>},                                                     \
     {c2f_search<false, true, 1, R>, c2f_search<false, true, 3, R>}},                                                      \
    {{c2f_search<true, false, 1, R>, c2f_search<true, false, 3, R>},                                                       \
     {c2f_search<true, true, 1, R>, c2f_search<true, true, 3, R>}}                                                         \
  }
static const C2fSearch kC2fSearch[2][2][2][2] = {ICTR_C2F_FORMS(false), ICTR_C2F_FORMS(true)};
#undef ICTR_C2F_FORMS

// a run on c->channels pyramids per frame (pyr_a[ch], pyr_b[ch]); `who` opens the messages
static int c2f_run(ictr_c2fflow *c, const ictr_pyramid *const *pyr_a, const ictr_pyramid *const *pyr_b, const char *who,
                   void *hip_stream) {
  const int nch = c->channels;
  PFArgs pfc[3];  // the argument checks and the level table of a patch search: pads, gradient planes, equal sizes
  for (int ch = 0; ch < nch; ++ch)
    if (int rc = patchflow_args(pyr_a[ch], pyr_b[ch], c->psz, c->lv_f, 0, c->maxiter, c->eps, &pfc[ch])) return rc;
  const PFArgs &pf = pfc[0];
  for (int ch = 1; ch < nch; ++ch)
    for (int l = 0; l <= c->lv_f; ++l)
      if (pfc[ch].lv[l].sw != pf.lv[l].sw || pfc[ch].lv[l].shift != pf.lv[l].shift || pfc[ch].lv[l].swo != pf.lv[l].swo ||
          pfc[ch].lv[l].sho != pf.lv[l].sho)
        return fail(ICTR_ERR_INVALID, "%s: the three pyramids of a frame differ in geometry at level %d (channel %d)", who, l,
                    ch);
  for (int l = 0; l <= c->lv_f; ++l)
    if ((int)pf.lv[l].swo != c->lv[l].w || (int)pf.lv[l].sho != c->lv[l].h)
      return fail(ICTR_ERR_INVALID, "c2fflow_run: level %d of the pyramids is %d x %d, of the object %d x %d", l,
                  (int)pf.lv[l].swo, (int)pf.lv[l].sho, c->lv[l].w, c->lv[l].h);
  hipStream_t s = (hipStream_t)hip_stream;
  const int refined = c->refine, patnorm = c->patnorm, x_only = c->x_only;
  const int robust = c->cost == ICTR_C2F_COST_HUBER;
  if (nch == 3 && refined && !c->bw12) {  // the first refined colour run: Bw of channels 1 and 2, the finest level's size
    const C2fLevel &L = c->lv[c->lv_l];
    if (int rc = c->bw12.alloc(sizeof(float) * 2 * (size_t)L.w * L.h, true)) return rc;
  }
  c->timed = c->timing;
  for (int l = c->lv_f; l >= c->lv_l; --l) {
    C2fLevel &L = c->lv[l];
    if (int rc = kC2fSearch[robust][patnorm][x_only][nch == 3](c, pfc, l, refined, s)) return rc;
    if (int rc = ictr_flowgrid_fill_(L.grid.get(), s)) return rc;
    if (c->timed) HIPCHK(hipEventRecord(L.ev[1].get(), s));
    if (int rc = ictr_flowdensify_run_level_(L.dens.get(), L.grid.get(), pyr_a, pyr_b, nch, c->psz, l,
                                             patnorm ? L.bias : nullptr, s))
      return rc;
    if (c->timed) HIPCHK(hipEventRecord(L.ev[2].get(), s));
    if (refined)
      if (int rc = ictr_flowrefine_run_level_(L.ref.get(), pyr_a, pyr_b, nch, ictr_flowdensify_device_ptr(L.dens.get()),
                                              x_only, l, c->bw12.get(), s))
        return rc;
    if (c->timed) HIPCHK(hipEventRecord(L.ev[3].get(), s));
  }
  if (c->lv_l > 0) {  // the finest level's field to the frame's size
    const C2fLevel &L = c->lv[c->lv_l];
    launch_flow_upsample(c2f_field(L, refined), L.w, L.h, c->lv_l, c->up.get(), c->w, c->h, x_only, s);
    if (c->timed) HIPCHK(hipEventRecord(c->up_done.get(), s));
  }
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(c->done.get(), s));
  c->ran = 1;
  c->ran_refined = refined;
  c->ran_patnorm = patnorm;
  return ICTR_OK;
}
extern "C" int ictr_c2fflow_run(ictr_c2fflow *c, const ictr_pyramid *pyr_a, const ictr_pyramid *pyr_b, void *hip_stream) {
  if (!c) return fail(ICTR_ERR_INVALID, "c2fflow is NULL");
  if (c->channels != 1)
    return fail(ICTR_ERR_INVALID, "c2fflow_run: the object has %d channels; a colour run is ictr_c2fflow_run_rgb", c->channels);
  return c2f_run(c, &pyr_a, &pyr_b, "c2fflow_run", hip_stream);
}
extern "C" int ictr_c2fflow_run_rgb(ictr_c2fflow *c, const ictr_pyramid *const pyr_a[3], const ictr_pyramid *const pyr_b[3],
                                    void *hip_stream) {
  if (!c) return fail(ICTR_ERR_INVALID, "c2fflow is NULL");
  if (c->channels != 3)
    return fail(ICTR_ERR_INVALID, "c2fflow_run_rgb: the object has %d channel; set 3 with ictr_c2fflow_set_channels",
                c->channels);
  if (!pyr_a || !pyr_b) return fail(ICTR_ERR_INVALID, "c2fflow_run_rgb: a pyramid triple is NULL");
  return c2f_run(c, pyr_a, pyr_b, "c2fflow_run_rgb", hip_stream);
}
extern "C" int ictr_c2fflow_set_channels(ictr_c2fflow *c, int n) {
  if (!c) return fail(ICTR_ERR_INVALID, "c2fflow is NULL");
  if (n != 1 && n != 3) return fail(ICTR_ERR_INVALID, "c2fflow_set_channels: n is %d (1: grey, or 3: colour)", n);
  if (c->ran) return fail(ICTR_ERR_STATE, "c2fflow_set_channels: the object has run; set the channels before the first run");
  if (n == c->channels) return ICTR_OK;
  return c2f_place_bias(c, n);  // (sets c->channels once the block is there)
}
extern "C" int ictr_c2fflow_get_channels(const ictr_c2fflow *c, int *n) {
  if (!c || !n) return fail(ICTR_ERR_INVALID, "c2fflow_get_channels: c2fflow or n is NULL");
  *n = c->channels;
  return ICTR_OK;
}

static int c2f_wait(ictr_c2fflow *c, const char *what) {
  if (!c) return fail(ICTR_ERR_INVALID, "c2fflow is NULL");
  if (!c->ran) return fail(ICTR_ERR_STATE, "%s: no run yet", what);
  HIPCHK(hipEventSynchronize(c->done.get()));
  return ICTR_OK;
}
extern "C" int ictr_c2fflow_result(ictr_c2fflow *c, float *out, int on_device) {
  if (int rc = c2f_wait(c, "c2fflow_result")) return rc;
  if (!out) return fail(ICTR_ERR_INVALID, "c2fflow_result: out is NULL");
  HIPCHK(hipMemcpy(out, c2f_result(c, c->ran_refined), sizeof(float) * 2 * (size_t)c->w * c->h,
                   on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost));
  return ICTR_OK;
}
extern "C" const float *ictr_c2fflow_device_ptr(const ictr_c2fflow *c) {
  if (!c) return nullptr;
  return c2f_result(c, c->ran ? c->ran_refined : c->refine);
}
extern "C" int ictr_c2fflow_level_dims(const ictr_c2fflow *c, int level, int *w, int *h, int *nx, int *ny) {
  if (!c) return fail(ICTR_ERR_INVALID, "c2fflow is NULL");
  if (level < c->lv_l || level > c->lv_f)
    return fail(ICTR_ERR_INVALID, "c2fflow_level_dims: level is %d (%d .. %d)", level, c->lv_l, c->lv_f);
  const C2fLevel &L = c->lv[level];
  if (w) *w = L.w;
  if (h) *h = L.h;
  if (nx) *nx = L.nx;
  if (ny) *ny = L.ny;
  return ICTR_OK;
}
extern "C" int ictr_c2fflow_read_level(ictr_c2fflow *c, int level, float *field, float *d, unsigned char *status) {
  if (int rc = c2f_wait(c, "c2fflow_read_level")) return rc;
  if (level < c->lv_l || level > c->lv_f)
    return fail(ICTR_ERR_INVALID, "c2fflow_read_level: level is %d (%d .. %d)", level, c->lv_l, c->lv_f);
  const C2fLevel &L = c->lv[level];
  const size_t K = (size_t)L.nx * L.ny;
  if (field)
    HIPCHK(hipMemcpy(field, c2f_field(L, c->ran_refined), sizeof(float) * 2 * (size_t)L.w * L.h, hipMemcpyDeviceToHost));
  if (d)
    if (int rc = ictr_flowgrid_nodes(L.grid.get(), d, nullptr)) return rc;
  if (status) HIPCHK(hipMemcpy(status, L.status, K, hipMemcpyDeviceToHost));
  return ICTR_OK;
}
// the two bias readers: `who` names the caller; wrong_channels: its refusal of an object of the other channel count
static int c2f_read_bias(ictr_c2fflow *c, int level, float *bias, const char *who, int channels, const char *wrong_channels) {
  if (int rc = c2f_wait(c, who)) return rc;
  if (level < c->lv_l || level > c->lv_f)
    return fail(ICTR_ERR_INVALID, "%s: level is %d (%d .. %d)", who, level, c->lv_l, c->lv_f);
  if (!bias) return fail(ICTR_ERR_INVALID, "%s: bias is NULL", who);
  if (!c->ran_patnorm) return fail(ICTR_ERR_STATE, "%s: the last run had patnorm off", who);
  if (c->channels != channels) return fail(ICTR_ERR_INVALID, wrong_channels, who, c->channels);
  const C2fLevel &L = c->lv[level];
  HIPCHK(hipMemcpy(bias, L.bias, sizeof(float) * (size_t)channels * L.nx * L.ny, hipMemcpyDeviceToHost));
  return ICTR_OK;
}
extern "C" int ictr_c2fflow_read_level_bias(ictr_c2fflow *c, int level, float *bias) {
  return c2f_read_bias(c, level, bias, "c2fflow_read_level_bias", 1,
                       "%s: the object has %d channels; use ictr_c2fflow_read_level_bias_rgb");
}
extern "C" int ictr_c2fflow_read_level_bias_rgb(ictr_c2fflow *c, int level, float *bias) {
  return c2f_read_bias(c, level, bias, "c2fflow_read_level_bias_rgb", 3, "%s: the object has %d channel");
}
extern "C" int ictr_c2fflow_get_kernel_ms(ictr_c2fflow *c, float *ms) {
  if (int rc = c2f_wait(c, "c2fflow_get_kernel_ms")) return rc;
  if (!ms) return fail(ICTR_ERR_INVALID, "c2fflow_get_kernel_ms: ms is NULL");
  for (int l = 0; l <= c->lv_f; ++l)
    for (int k = 0; k < 3; ++k) {
      ms[3 * l + k] = 0.0f;
      if (c->timed && l >= c->lv_l)  // (a level below lv_l has no events)
        HIPCHK(hipEventElapsedTime(&ms[3 * l + k], c->lv[l].ev[k].get(), c->lv[l].ev[k + 1].get()));
    }
  return ICTR_OK;
}
extern "C" int ictr_c2fflow_get_lv_l(const ictr_c2fflow *c, int *lv_l) {
  if (!c || !lv_l) return fail(ICTR_ERR_INVALID, "c2fflow_get_lv_l: c2fflow or lv_l is NULL");
  *lv_l = c->lv_l;
  return ICTR_OK;
}
extern "C" int ictr_c2fflow_get_upsample_ms(ictr_c2fflow *c, float *ms) {
  if (int rc = c2f_wait(c, "c2fflow_get_upsample_ms")) return rc;
  if (!ms) return fail(ICTR_ERR_INVALID, "c2fflow_get_upsample_ms: ms is NULL");
  *ms = 0.0f;
  if (c->timed && c->lv_l > 0) HIPCHK(hipEventElapsedTime(ms, c->lv[c->lv_l].ev[3].get(), c->up_done.get()));
  return ICTR_OK;
}
extern "C" int ictr_flow_upsample(const float *src, int w_l, int h_l, int lv, float *out, int w, int h, int x_only,
                                  int on_device, void *hip_stream) {
  if (!src || !out) return fail(ICTR_ERR_INVALID, "flow_upsample: src or out is NULL");
  if (w < 1 || h < 1 || lv < 1 || lv > 15) return fail(ICTR_ERR_INVALID, "flow_upsample: w, h >= 1, lv is 1 .. 15");
  int ew = 0, eh = 0;
  pyramid_level_size(w, h, lv, &ew, &eh);
  if (ew < 1 || eh < 1) return fail(ICTR_ERR_INVALID, "flow_upsample: level %d of %d x %d is empty", lv, w, h);
  if (w_l != ew || h_l != eh)
    return fail(ICTR_ERR_INVALID, "flow_upsample: the field is %d x %d, level %d of %d x %d is %d x %d", w_l, h_l, lv, w, h,
                ew, eh);
  if (int rc = need_device()) return rc;
  hipStream_t s = (hipStream_t)hip_stream;
  if (on_device) {
    launch_flow_upsample(src, w_l, h_l, lv, out, w, h, x_only, s);
    HIPCHK(hipGetLastError());
    return ICTR_OK;
  }
  const size_t nsrc = sizeof(float) * 2 * (size_t)w_l * h_l, nout = sizeof(float) * 2 * (size_t)w * h;
  DevBuf<float> dsrc, dout;
  if (int rc = dsrc.alloc(nsrc)) return rc;
  if (int rc = dout.alloc(nout)) return rc;
  HIPCHK(hipMemcpyAsync(dsrc.get(), src, nsrc, hipMemcpyHostToDevice, s));
  launch_flow_upsample(dsrc.get(), w_l, h_l, lv, dout.get(), w, h, x_only, s);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(out, dout.get(), nout, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  return ICTR_OK;
}
