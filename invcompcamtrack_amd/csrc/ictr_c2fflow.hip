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
// ictr_c2fflow_dev.h; this file instantiates the L2 forms and ictr_c2fflow_robust.hip the ROBUST ones. Restated by
// tests/c2fcost_f32.py.
//
// Every kernel of a run takes the arguments of 1 .. kSetMax flows of one shape and runs a member's workgroups on the
// member its block index names (DESIGN.md "Lockstep sets"); an object's own run is a set of one, and ictr_c2fset_run the
// same walk over the levels (c2f_walk) on several.
//
// k_flow_upsample<XONLY> finishes a run whose finest level is above 0 (DESIGN.md "A finest level above 0"): the field of
// level lv to the w x h frame, bilinear with half-pixel centres at the fixed factor 2^-lv, the vectors times 2^lv. One lane
// per output pixel, a wave per 64 consecutive columns of a row and kWaves rows per workgroup, so that a workgroup's source
// taps are two or three rows' worth of at most 34 records; one whole float2 store per lane, 512 contiguous bytes per wave.
// No LDS, no atomics. Restated by tests/c2fup_f32.py; the definition is patchflow.upsample_flow_host.
#include <math.h>
#include <string.h>

#include <memory>
#include <string>
#include <type_traits>
#include <vector>

#include "ictr_dev.h"
#include "ictr_launch.h"
#include "ictr_devfn.h"
#include "ictr_patchflow_dev.h"
#include "ictr_c2fflow_dev.h"

namespace ictr {

// the fields k_flow_upsample reads and writes, per member
struct UpArgs {
  const float2 *src[kSetMax];
  float2 *out[kSetMax];
};
// s = 2^lv, inv_s = 2^-lv; member blockIdx.z's field. Everything before the taps is exact in f32 (x + 0.5, the product
// with 2^-lv, - 0.5, rx, 1 - rx); the six products and three sums are taken in the order written, each rounded (no
// contraction), then s * val.
template <bool XONLY>
__global__ __launch_bounds__(kBlock) void k_flow_upsample(UpArgs io, int wl, int hl, float inv_s, float s, int w, int h) {
  const float2 *__restrict__ src = io.src[blockIdx.z];
  float2 *__restrict__ out = io.out[blockIdx.z];
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

// n fields src[m] [hl][wl][2] to out[m] [h][w][2], all on the device; the caller has checked the sizes
static void launch_flow_upsample(const UpArgs &a, int n, int wl, int hl, int lv, int w, int h, int x_only, hipStream_t s) {
  const float sc = (float)(1 << lv), inv = 1.0f / sc;
  dim3 g = pixel_rows_grid(w, h);
  g.z = n;
  if (x_only)
    hipLaunchKernelGGL((k_flow_upsample<true>), g, dim3(kBlock), 0, s, a, wl, hl, inv, sc, w, h);
  else
    hipLaunchKernelGGL((k_flow_upsample<false>), g, dim3(kBlock), 0, s, a, wl, hl, inv, sc, w, h);
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
};
}  // namespace

constexpr int kC2fMaxLevels = 16;  // levels 0 .. 15: the level table of a patch search (PFArgs) holds as many
static_assert(kC2fMaxLevels == sizeof(PFArgs::lv) / sizeof(PFLevel), "the levels of a coarse-to-fine flow are PFArgs' levels");

// The stage events of a timed run over the levels lv_l .. lv_f, an object's own or a set's.
struct C2fEvents {
  int timing = 0, timed = 0;    // asked for; recorded by the last run
  Event lv[kC2fMaxLevels][4];   // per level: before the search, after the fill, the densifier, the refiner
  Event up_done;                // lv_l > 0: behind k_flow_upsample (it starts at level lv_l's last event)
  int create(int lv_l, int lv_f) {
    for (int l = lv_l; l <= lv_f; ++l)
      for (Event &e : lv[l])
        if (int rc = e.create()) return rc;
    return lv_l > 0 ? up_done.create() : ICTR_OK;
  }
  // ms [3 (lv_f + 1)]: search + fill, densifier, refiner per level; *up_ms: the up-sampling. Either may be NULL; zeros
  // behind an untimed run and at the levels below lv_l
  int read(int lv_l, int lv_f, float *ms, float *up_ms) const {
    for (int l = 0; ms && l <= lv_f; ++l)
      for (int k = 0; k < 3; ++k) {
        ms[3 * l + k] = 0.0f;
        if (timed && l >= lv_l) HIPCHK(hipEventElapsedTime(&ms[3 * l + k], lv[l][k].get(), lv[l][k + 1].get()));
      }
    if (up_ms) {
      *up_ms = 0.0f;
      if (timed && lv_l > 0) HIPCHK(hipEventElapsedTime(up_ms, lv[lv_l][3].get(), up_done.get()));
    }
    return ICTR_OK;
  }
};

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
  int ran = 0, ran_refined = 0, ran_patnorm = 0;
  std::vector<C2fLevel> lv;  // [lv_f + 1]; the levels below lv_l hold their size and nothing else
  DevBuf<unsigned char> status;
  DevBuf<float> bias;  // next to it: the node bias of a run with patch-mean normalisation
  DevBuf<float> bw12;  // two planes of the finest level's size, the refinement's Bw of channels 1 and 2: made by the first
                       // refined run of a 3-channel object
  DevBuf<float> up;    // lv_l > 0: the result plane [h][w][2], level lv_l's field up-sampled
  C2fEvents ev;        // of the object's own timed run
  Event done;  // behind the last run, its own or a set's
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
  if (!out || w < 1 || h < 1 || lv_f < 0 || lv_f >= kC2fMaxLevels || step < 1)
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
    nodes += (size_t)L.nx * L.ny;
  }
  if (int rc = c->status.alloc(nodes, true)) return rc;
  unsigned char *cur = c->status.get();
  for (C2fLevel &L : c->lv) {  // (a level below lv_l has no nodes)
    L.status = cur;
    cur += (size_t)L.nx * L.ny;
  }
  if (int rc = c2f_place_bias(c.get(), 1)) return rc;
  if (lv_l > 0)
    if (int rc = c->up.alloc(sizeof(float) * 2 * (size_t)w * h, true)) return rc;
  if (int rc = c->ev.create(lv_l, lv_f)) return rc;
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
  c->ev.timing = on ? 1 : 0;
  return ICTR_OK;
}

// the kernel arguments of level l's search of a run: pfc[ch] the level tables of the channels' pyramids, which agree in
// geometry
template <bool MEAN, int NCH, bool ROBUST>
static int c2f_search_args(const ictr_c2fflow *c, const PFArgs *pfc, int l, int refined, C2fArgsOf<MEAN, NCH, ROBUST> *out) {
  const C2fLevel &L = c->lv[l];
  const PFArgs &pf = pfc[0];
  C2fArgsOf<MEAN, NCH, ROBUST> &a = *out;
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
  a.min_det = c->x_only ? pf.min_hx : pf.min_det;
  a.far2 = (float)(c->psz * c->psz);
  if (int rc = ictr_flowgrid_node_buffers_(L.grid.get(), &a.d, &a.lost)) return rc;
  a.status = L.status;
  if constexpr (MEAN) a.bias = L.bias;
  if constexpr (ROBUST) a.huber_k = c->huber_k;
  return ICTR_OK;
}
// level l's search of n members: pfc[m] the level tables of member m's channels
template <bool MEAN, int NCH, bool ROBUST>
static int c2f_search(ictr_c2fflow *const *m, int n, const PFArgs (*pfc)[3], int l, int refined, hipStream_t s) {
  SetArgs<C2fArgsOf<MEAN, NCH, ROBUST>> a;
  memset(&a, 0, sizeof(a));
  for (int i = 0; i < n; ++i)
    if (int rc = c2f_search_args<MEAN, NCH, ROBUST>(m[i], pfc[i], l, refined, &a.m[i])) return rc;
  launch_c2f_level<MEAN, NCH, ROBUST>(a, n, m[0]->x_only, s);
  return ICTR_OK;
}
// the search's form by [cost == Huber][patnorm][channels == 3]
using C2fSearch = int (*)(ictr_c2fflow *const *, int, const PFArgs (*)[3], int, int, hipStream_t);
#define ICTR_C2F_FORMS(R) \
  {{c2f_search<false, 1, R>, c2f_search<false, 3, R>}, {c2f_search<true, 1, R>, c2f_search<true, 3, R>}}
static const C2fSearch kC2fSearch[2][2][2] = {ICTR_C2F_FORMS(false), ICTR_C2F_FORMS(true)};
#undef ICTR_C2F_FORMS

// the argument checks of a run and pfc[ch], the level tables of a patch search on the channels' pyramids: pads, gradient
// planes, equal sizes; `who` opens the messages
static int c2f_run_args(const ictr_c2fflow *c, const ictr_pyramid *const *pyr_a, const ictr_pyramid *const *pyr_b,
                        const char *who, PFArgs *pfc) {
  const int nch = c->channels;
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
      return fail(ICTR_ERR_INVALID, "%s: level %d of the pyramids is %d x %d, of the object %d x %d", who, l,
                  (int)pf.lv[l].swo, (int)pf.lv[l].sho, c->lv[l].w, c->lv[l].h);
  return ICTR_OK;
}
// The walk over the levels lv_f .. lv_l for the n members m[] (1 .. kSetMax, which agree in shape and parameters: member
// 0's stand for all), every stage enqueued once. pfc[i]: member i's level tables (c2f_run_args); member i's pyramids are
// pyr_a[i * channels + ch], pyr_b[i * channels + ch]. ev: the stage events, recorded when ev.timing is on; rowhas: the
// fill's block for n members (NULL: the one grid's own). *ops takes the launches and memsets enqueued. Behind the run every
// member is as behind its own: `done` recorded, the stage events not its own unless ev is.
static int c2f_walk(ictr_c2fflow *const *m, int n, const PFArgs (*pfc)[3], const ictr_pyramid *const *pyr_a,
                    const ictr_pyramid *const *pyr_b, C2fEvents &ev, int *rowhas, int *ops, hipStream_t s) {
  ictr_c2fflow *const c0 = m[0];
  const int nch = c0->channels, refined = c0->refine, patnorm = c0->patnorm, x_only = c0->x_only;
  const int robust = c0->cost == ICTR_C2F_COST_HUBER;
  if (nch == 3 && refined)  // the first refined colour run: Bw of channels 1 and 2, the finest level's size, per member
    for (int i = 0; i < n; ++i) {
      const C2fLevel &L = m[i]->lv[c0->lv_l];
      if (!m[i]->bw12)
        if (int rc = m[i]->bw12.alloc(sizeof(float) * 2 * (size_t)L.w * L.h, true)) return rc;
    }
  for (int i = 0; i < n; ++i) m[i]->ev.timed = 0;
  const int timed = ev.timed = ev.timing;
  int count = 0;
  ictr_flowgrid *grid[kSetMax] = {};
  ictr_flowdensify *dens[kSetMax] = {};
  ictr_flowrefine *ref[kSetMax] = {};
  const float *bias[kSetMax] = {}, *field[kSetMax] = {};
  float *bw12[kSetMax] = {};
  for (int l = c0->lv_f; l >= c0->lv_l; --l) {
    for (int i = 0; i < n; ++i) {
      C2fLevel &L = m[i]->lv[l];
      grid[i] = L.grid.get(), dens[i] = L.dens.get(), ref[i] = L.ref.get();
      bias[i] = patnorm ? L.bias : nullptr;
      field[i] = ictr_flowdensify_device_ptr(L.dens.get());
      bw12[i] = m[i]->bw12.get();
    }
    if (timed) HIPCHK(hipEventRecord(ev.lv[l][0].get(), s));
    if (int rc = kC2fSearch[robust][patnorm][nch == 3](m, n, pfc, l, refined, s)) return rc;
    if (int rc = ictr_flowgrid_fill_(grid, n, rowhas, s)) return rc;
    count += 4;  // the search, the memset of rowhas and the fill's two launches
    if (timed) HIPCHK(hipEventRecord(ev.lv[l][1].get(), s));
    if (int rc = ictr_flowdensify_run_level_(dens, grid, pyr_a, pyr_b, n, nch, c0->psz, l, bias, s)) return rc;
    count += 1;
    if (timed) HIPCHK(hipEventRecord(ev.lv[l][2].get(), s));
    if (refined) {
      int k = 0;
      if (int rc = ictr_flowrefine_run_level_(ref, pyr_a, pyr_b, n, nch, field, x_only, l, bw12, &k, s)) return rc;
      count += k;
    }
    if (timed) HIPCHK(hipEventRecord(ev.lv[l][3].get(), s));
  }
  if (c0->lv_l > 0) {  // the finest level's fields to the frame's size
    UpArgs u;
    memset(&u, 0, sizeof(u));
    for (int i = 0; i < n; ++i) {
      u.src[i] = reinterpret_cast<const float2 *>(c2f_field(m[i]->lv[c0->lv_l], refined));
      u.out[i] = reinterpret_cast<float2 *>(m[i]->up.get());
    }
    const C2fLevel &L = c0->lv[c0->lv_l];
    launch_flow_upsample(u, n, L.w, L.h, c0->lv_l, c0->w, c0->h, x_only, s);
    count += 1;
    if (timed) HIPCHK(hipEventRecord(ev.up_done.get(), s));
  }
  HIPCHK(hipGetLastError());
  for (int i = 0; i < n; ++i) {
    ictr_c2fflow *c = m[i];
    HIPCHK(hipEventRecord(c->done.get(), s));
    c->ran = 1;
    c->ran_refined = refined;
    c->ran_patnorm = patnorm;
  }
  if (ops) *ops = count;
  return ICTR_OK;
}
// an object's own run on c->channels pyramids per frame (pyr_a[ch], pyr_b[ch]): the walk on a set of one; `who` opens
// the messages
static int c2f_run(ictr_c2fflow *c, const ictr_pyramid *const *pyr_a, const ictr_pyramid *const *pyr_b, const char *who,
                   void *hip_stream) {
  PFArgs pfc[1][3];
  if (int rc = c2f_run_args(c, pyr_a, pyr_b, who, pfc[0])) return rc;
  return c2f_walk(&c, 1, pfc, pyr_a, pyr_b, c->ev, nullptr, nullptr, (hipStream_t)hip_stream);
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
  return c->ev.read(c->lv_l, c->lv_f, ms, nullptr);
}
extern "C" int ictr_c2fflow_get_lv_l(const ictr_c2fflow *c, int *lv_l) {
  if (!c || !lv_l) return fail(ICTR_ERR_INVALID, "c2fflow_get_lv_l: c2fflow or lv_l is NULL");
  *lv_l = c->lv_l;
  return ICTR_OK;
}
extern "C" int ictr_c2fflow_get_upsample_ms(ictr_c2fflow *c, float *ms) {
  if (int rc = c2f_wait(c, "c2fflow_get_upsample_ms")) return rc;
  if (!ms) return fail(ICTR_ERR_INVALID, "c2fflow_get_upsample_ms: ms is NULL");
  return c->ev.read(c->lv_l, c->lv_f, nullptr, ms);
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
  const size_t nsrc = sizeof(float) * 2 * (size_t)w_l * h_l, nout = sizeof(float) * 2 * (size_t)w * h;
  DevBuf<float> dsrc, dout;
  if (!on_device) {
    if (int rc = dsrc.alloc(nsrc)) return rc;
    if (int rc = dout.alloc(nout)) return rc;
    HIPCHK(hipMemcpyAsync(dsrc.get(), src, nsrc, hipMemcpyHostToDevice, s));
  }
  UpArgs u;  // a set of one
  memset(&u, 0, sizeof(u));
  u.src[0] = reinterpret_cast<const float2 *>(on_device ? src : dsrc.get());
  u.out[0] = reinterpret_cast<float2 *>(on_device ? out : dout.get());
  launch_flow_upsample(u, 1, w_l, h_l, lv, w, h, x_only, s);
  HIPCHK(hipGetLastError());
  if (on_device) return ICTR_OK;
  HIPCHK(hipMemcpyAsync(out, dout.get(), nout, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  return ICTR_OK;
}

// ---------------------------------------------------------------- lockstep sets (include/ictr_c2f_set.h)
// A set of coarse-to-fine flows of equal shape and parameters, run in lockstep (DESIGN.md §4 "Lockstep sets"): c2f_walk
// on all of them, every stage enqueued once. The set holds its members' addresses and owns what no member can: the rowhas
// block of the fill for all members, the events of a timed run, and the event behind the last run.
static_assert(ICTR_C2FSET_MAX == kSetMax, "ictr_c2f_set.h and ictr_dev.h disagree on the members of a set");
struct ictr_c2fset {
  int n = 0;
  ictr_c2fflow *m[kSetMax] = {};
  int ran = 0, ops = 0;
  DevBuf<int> rowhas;  // [n][the most node rows of a level]
  C2fEvents ev;
  Event done;
};

// the refusals of members that are missing, doubled or differ from member 0; `who` opens the message
static int c2fset_compare(ictr_c2fflow *const *m, int n, const char *who) {
  if (!m) return fail(ICTR_ERR_INVALID, "%s: members is NULL", who);
  if (n < 1 || n > kSetMax) return fail(ICTR_ERR_INVALID, "%s: n is %d (1 .. %d)", who, n, kSetMax);
  for (int i = 0; i < n; ++i) {
    if (!m[i]) return fail(ICTR_ERR_INVALID, "%s: member %d is NULL", who, i);
    for (int j = 0; j < i; ++j)
      if (m[j] == m[i]) return fail(ICTR_ERR_INVALID, "%s: member %d is the same object as member %d", who, i, j);
  }
  const ictr_c2fflow *a = m[0];
  for (int i = 1; i < n; ++i) {
    const ictr_c2fflow *b = m[i];
    const struct {
      const char *name;
      double vb, va;
    } f[] = {{"w", (double)b->w, (double)a->w},
             {"h", (double)b->h, (double)a->h},
             {"lv_f", (double)b->lv_f, (double)a->lv_f},
             {"lv_l", (double)b->lv_l, (double)a->lv_l},
             {"step", (double)b->step, (double)a->step},
             {"psz", (double)b->psz, (double)a->psz},
             {"maxiter", (double)b->maxiter, (double)a->maxiter},
             {"eps", (double)b->eps, (double)a->eps},
             {"refine", (double)b->refine, (double)a->refine},
             {"patnorm", (double)b->patnorm, (double)a->patnorm},
             {"x_only", (double)b->x_only, (double)a->x_only},
             {"channels", (double)b->channels, (double)a->channels},
             {"cost", (double)b->cost, (double)a->cost},
             {"huber_k", (double)b->huber_k, (double)a->huber_k}};
    for (const auto &e : f)
      if (!(e.vb == e.va))
        return fail(ICTR_ERR_INVALID, "%s: member %d differs from member 0 in %s (%g, member 0 has %g)", who, i, e.name, e.vb,
                    e.va);
    // the stages' parameters are those of every level of an object: the finest stands for all
    float ea = 0.0f, eb = 0.0f;
    int pa = 0, pb = 0;
    if (int rc = ictr_flowdensify_get_params_(a->lv[a->lv_l].dens.get(), &ea, &pa)) return rc;
    if (int rc = ictr_flowdensify_get_params_(b->lv[b->lv_l].dens.get(), &eb, &pb)) return rc;
    if (!(ea == eb))
      return fail(ICTR_ERR_INVALID, "%s: member %d differs from member 0 in the densifier's minerr (%g, member 0 has %g)", who,
                  i, (double)eb, (double)ea);
    if (pa != pb)
      return fail(ICTR_ERR_INVALID, "%s: member %d differs from member 0 in the densifier's power (%d, member 0 has %d)", who,
                  i, pb, pa);
    if (a->refine) {
      static const char *const fname[4] = {"alpha", "gamma", "delta", "omega"}, *const iname[2] = {"n_outer", "n_sor"};
      float fa[4], fb[4];
      int ia[2], ib[2];
      if (int rc = ictr_flowrefine_get_params_(a->lv[a->lv_l].ref.get(), fa, ia)) return rc;
      if (int rc = ictr_flowrefine_get_params_(b->lv[b->lv_l].ref.get(), fb, ib)) return rc;
      for (int k = 0; k < 4; ++k)
        if (!(fa[k] == fb[k]))
          return fail(ICTR_ERR_INVALID, "%s: member %d differs from member 0 in the refinement's %s (%g, member 0 has %g)", who,
                      i, fname[k], (double)fb[k], (double)fa[k]);
      for (int k = 0; k < 2; ++k)
        if (ia[k] != ib[k])
          return fail(ICTR_ERR_INVALID, "%s: member %d differs from member 0 in the refinement's %s (%d, member 0 has %d)", who,
                      i, iname[k], ib[k], ia[k]);
    }
  }
  return ICTR_OK;
}

extern "C" void ictr_c2fset_destroy(ictr_c2fset *s) {
  if (s && s->ran) (void)hipEventSynchronize(s->done.get());  // before the rowhas block of a run in flight is released
  delete s;
}
extern "C" int ictr_c2fset_create(ictr_c2fset **out, ictr_c2fflow *const *members, int n) {
  if (!out) return fail(ICTR_ERR_INVALID, "c2fset_create: out is NULL");
  if (int rc = c2fset_compare(members, n, "c2fset_create")) return rc;
  if (int rc = need_device()) return rc;
  auto s = std::make_unique<ictr_c2fset>();
  s->n = n;
  const ictr_c2fflow *c = members[0];
  int ny = 1;
  for (int l = c->lv_l; l <= c->lv_f; ++l) ny = c->lv[l].ny > ny ? c->lv[l].ny : ny;
  for (int i = 0; i < n; ++i) s->m[i] = members[i];
  if (int rc = s->rowhas.alloc(sizeof(int) * (size_t)n * ny, true)) return rc;
  if (int rc = s->ev.create(c->lv_l, c->lv_f)) return rc;
  if (int rc = s->done.create(hipEventDisableTiming)) return rc;
  *out = s.release();
  return ICTR_OK;
}
extern "C" int ictr_c2fset_size(const ictr_c2fset *s, int *n) {
  if (!s || !n) return fail(ICTR_ERR_INVALID, "c2fset_size: the set or n is NULL");
  *n = s->n;
  return ICTR_OK;
}
extern "C" int ictr_c2fset_last_operations(const ictr_c2fset *s, int *ops) {
  if (!s || !ops) return fail(ICTR_ERR_INVALID, "c2fset_last_operations: the set or ops is NULL");
  *ops = s->ops;
  return ICTR_OK;
}
extern "C" int ictr_c2fset_set_timing(ictr_c2fset *s, int on) {
  if (!s) return fail(ICTR_ERR_INVALID, "c2fset is NULL");
  s->ev.timing = on ? 1 : 0;
  return ICTR_OK;
}

// a lockstep run on `nch` pyramids per member and frame; everything that can be refused is checked before anything is
// enqueued or any member touched
static int c2fset_run(ictr_c2fset *set, const ictr_pyramid *const *pyr_a, const ictr_pyramid *const *pyr_b, int nch,
                      const char *who, void *hip_stream) {
  if (!set) return fail(ICTR_ERR_INVALID, "%s: the set is NULL", who);
  if (!pyr_a || !pyr_b) return fail(ICTR_ERR_INVALID, "%s: a pyramid table is NULL", who);
  const int n = set->n;
  if (int rc = c2fset_compare(set->m, n, who)) return rc;
  ictr_c2fflow *const c0 = set->m[0];
  if (c0->channels != nch)
    return fail(ICTR_ERR_INVALID, "%s: the members have %d channel%s; %s", who, c0->channels, c0->channels == 1 ? "" : "s",
                nch == 1 ? "a colour run is ictr_c2fset_run_rgb" : "a grey run is ictr_c2fset_run");
  std::vector<PFArgs> store((size_t)n * 3);
  PFArgs(*pfc)[3] = reinterpret_cast<PFArgs(*)[3]>(store.data());
  for (int m = 0; m < n; ++m)
    if (int rc = c2f_run_args(set->m[m], pyr_a + m * nch, pyr_b + m * nch, who, pfc[m])) {
      std::string why = ictr_last_error();  // the member's number goes behind the call's name, where the reason opens with it
      const std::string head = std::string(who) + ": ";
      if (why.compare(0, head.size(), head) == 0) why.erase(0, head.size());
      return fail(rc, "%s: member %d: %s", who, m, why.c_str());
    }
  hipStream_t s = (hipStream_t)hip_stream;
  if (int rc = c2f_walk(set->m, n, pfc, pyr_a, pyr_b, set->ev, set->rowhas.get(), &set->ops, s)) return rc;
  HIPCHK(hipEventRecord(set->done.get(), s));
  set->ran = 1;
  return ICTR_OK;
}
extern "C" int ictr_c2fset_run(ictr_c2fset *s, const ictr_pyramid *const *pyr_a, const ictr_pyramid *const *pyr_b,
                               void *hip_stream) {
  return c2fset_run(s, pyr_a, pyr_b, 1, "c2fset_run", hip_stream);
}
extern "C" int ictr_c2fset_run_rgb(ictr_c2fset *s, const ictr_pyramid *const *pyr_a, const ictr_pyramid *const *pyr_b,
                                   void *hip_stream) {
  return c2fset_run(s, pyr_a, pyr_b, 3, "c2fset_run_rgb", hip_stream);
}
extern "C" int ictr_c2fset_get_kernel_ms(ictr_c2fset *s, float *ms, float *upsample_ms) {
  if (!s) return fail(ICTR_ERR_INVALID, "c2fset is NULL");
  if (!s->ran) return fail(ICTR_ERR_STATE, "c2fset_get_kernel_ms: no run yet");
  if (!ms) return fail(ICTR_ERR_INVALID, "c2fset_get_kernel_ms: ms is NULL");
  HIPCHK(hipEventSynchronize(s->done.get()));
  return s->ev.read(s->m[0]->lv_l, s->m[0]->lv_f, ms, upsample_ms);
}
