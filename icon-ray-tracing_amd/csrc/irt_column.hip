// irt_column.hip -- column products (include/icon_rt_hip.h, "column products"): a reduction over the
// vertical of the field sampled on a column's levels -- the weighted sum, the maximum and minimum
// with their levels, the number of levels found -- on a lat x lon grid (irt_column_latlon) and on
// the globe as the camera sees it (irt_render_column).  One pass: a wave walks its 64 columns up the
// levels with the running values (irt_column.h ColumnAcc) in registers, and writes the results
// alone; the numLevels values per column irt_sample_latlon would write never reach memory.  Each
// level's points go through the point location of irt_sample_points (irt_sample_dev.h
// wave_locate); the host side (irt_column_reduce, the argument checks) is host/irt_column.cpp.
//
// The guard argument of irt_sample_dev.h covers the column points unchanged: whatever float triple
// a level's point comes to, it reaches a locator only through admit().

#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>

#include "irt_build.h"
#include "irt_column.h"
#include "irt_context.h"
#include "irt_raygen.h"
#include "irt_sample_dev.h"

namespace irt {

// What the kernels need beyond RenderArgs (which stays the kernels' FIRST argument: Tracer's late
// reads go through fresh_args(), the kernarg segment read as a RenderArgs)
struct ColumnArgs {
  const float *latCS;   // k_column_latlon: {cosf lat, sinf lat} per row ...
  const float *lonCS;   // ... and {cosf lon, sinf lon} per column
  const float *radius;  // the levels' radii
  const float *weight;  // ... and weights; null: every weight 1.0f
  int numLat, numLon, numLevels;
  uint32_t patchesLon;     // k_column_latlon: 8 x 8 patches per patch row
  unsigned long long n;    // ... and patches in the grid
  irt_column_out out;      // k_column_latlon's outputs, each may be null
  uint32_t packetsX;       // k_render_column: 8 x 8 pixel packets per packet row ...
  uint32_t numPackets;     // ... and in the frame
  float surfaceRadius;     // ... the sphere the product is drawn on
  int product;             // ... IRT_COLUMN_WSUM / _MAX / _MIN
  float *value;            // ... may be null
  float missValue;
  float rLo, rHi;          // the scene's sphericalBounds.lower.x / upper.x (cell sampler's cut)
};

namespace {

// A wave's 64 columns up the levels.  point(k, r, x, y, z) makes a lane's point of level k from
// the radius; `live`: the lane has a column.  The loop's bounds, the table reads at k and the skip
// of a level no lane is admitted at are wave-uniform, as Tracer::locate_wave needs every lane to
// call it; a lane the guard turns away is a miss of wave_locate in any case, so the skip changes
// no result.
template <int O, typename Point>
__device__ __forceinline__ void walk_columns(const RenderArgs &A, const ColumnArgs &S, bool live, ColumnAcc &a,
                                             SampleLds<(O & OPT_WEDGE) == 0> &L, Point point) {
  column_init(a);
#pragma nounroll
  for (int k = 0; k < S.numLevels; ++k) {
    const float r = S.radius[k];
    const float w = S.weight ? S.weight[k] : 1.f;
    float x, y, z;
    point(r, x, y, z);
    if (__ballot(live && admit<(O & OPT_WEDGE) == 0>(S.rLo, S.rHi, x, y, z)) == 0ull) continue;
    float v = 0.f;
    if (wave_locate<O>(A, S.rLo, S.rHi, live, x, y, z, v, L)) column_step(a, k, w, v);  // per lane
  }
  column_finish(a, S.missValue);
}

template <typename T>
__device__ __forceinline__ void put(T *out, unsigned long long i, T v) {
  if (out) __builtin_nontemporal_store(v, &out[i]);  // streaming: nobody re-reads it in this kernel
}

// The lat x lon grid: a wave takes an 8 x 8 lat x lon patch (lane = 8 * dlat + dlon), the patch of
// k_sample_latlon, and every level of it.  Point (k, j, i) is made from the tables exactly as
// k_sample_latlon makes it (to_cartesian_trig); a lane's four trig values are read once.
template <int O>
__global__ void __launch_bounds__(64) k_column_latlon(RenderArgs A, ColumnArgs S) {
  __shared__ SampleLds<(O & OPT_WEDGE) == 0> L;
  const unsigned long long w = workgroup_index();
  if (w >= S.n) return;  // wave-uniform (the last grid row's tail)
  const unsigned long long j = (w / S.patchesLon) * 8ull + (threadIdx.x >> 3);
  const unsigned long long i = (w % S.patchesLon) * 8ull + (threadIdx.x & 7u);
  // live lanes index the tables inside their sizes: j < numLat, i < numLon
  const bool live = j < (unsigned long long)S.numLat && i < (unsigned long long)S.numLon;
  float t[4] = {0.f, 0.f, 0.f, 0.f};
  if (live) {
    t[0] = S.latCS[2 * j];
    t[1] = S.latCS[2 * j + 1];
    t[2] = S.lonCS[2 * i];
    t[3] = S.lonCS[2 * i + 1];
  }
  ColumnAcc a;
  walk_columns<O>(A, S, live, a, L, [&](float r, float &x, float &y, float &z) { to_cartesian_trig(r, t, x, y, z); });
  if (!live) return;
  const unsigned long long c = j * (unsigned long long)S.numLon + i;
  put(S.out.wsum, c, a.wsum);
  put(S.out.vmax, c, a.mx);
  put(S.out.vmin, c, a.mn);
  put(S.out.kmax, c, a.kmax);
  put(S.out.kmin, c, a.kmin);
  put(S.out.count, c, a.count);
}

// The globe: one 8 x 8 pixel packet per wave (lane = 8 dy + dx, the raygen's packet).  The pixel's
// ray meets the sphere of surfaceRadius at P (the one hit slot of k_render_levels with that level and
// no flags: the near hit in front of the camera, else the far hit); the column under P is P scaled
// to each level's radius.  Lanes outside the frame, and lanes whose ray has no hit, stay in the
// wave and never want a point.
template <int O>
__global__ void __launch_bounds__(64) k_render_column(RenderArgs A, ColumnArgs S) {
  __shared__ SampleLds<(O & OPT_WEDGE) == 0> L;
  const uint32_t w = (uint32_t)workgroup_index();  // packets < 2^27
  if (w >= S.numPackets) return;                   // wave-uniform (the last grid row's tail)
  const uint32_t py = w / S.packetsX, px = w - py * S.packetsX;
  const int x = (int)(px * 8u + (threadIdx.x & 7u)), y = (int)(py * 8u + (threadIdx.x >> 3));
  const bool inFrame = x < A.W && y < A.H;
  uint32_t st = 0;
  float dx = 1.f, dy = 1.f, dz = 1.f;
  if (inFrame) gen_ray(A, A.accumID, x, y, st, dx, dy, dz);
  const Ray ray = {A.org.x, A.org.y, A.org.z, 0.f, dx, dy, dz, 1e10f};
  float tn = 0.f, tf = 0.f;
  const bool hit = inFrame && intersect_sphere(ray, S.surfaceRadius, tn, tf);
  const bool near = tn > 0.f;
  const bool live = hit && (near || tf > 0.f);
  const float t = near ? tn : tf;
  const float X = ray.ox + ray.dx * t, Y = ray.oy + ray.dy * t, Z = ray.oz + ray.dz * t;
  const float len = sqrtf(X * X + Y * Y + Z * Z);
  ColumnAcc a;
  walk_columns<O>(A, S, live, a, L, [&](float r, float &cx, float &cy, float &cz) {
    const float s = r / len;
    cx = X * s;
    cy = Y * s;
    cz = Z * s;
  });
  if (!inFrame) return;
  float cr = 0.f, cg = 0.f, cb = 0.f, alpha = 0.f;
  const float v = column_product(a, S.product);  // missValue where no level was found
  if (a.count > 0) {
    Tracer<O> T{{}, A, nullptr, A.sphBits, L.cnt, {0, 0, 0, 0, 0, 0, 0}};  // post_classify
    const float4 c = T.post_classify(v);
    alpha = c.w < 0.f ? 0.f : (c.w > 1.f ? 1.f : c.w);
    cr = alpha * (c.x * A.amb.x * A.ambRad);  // the raygen's products (deviceCode.cu:318)
    cg = alpha * (c.y * A.amb.y * A.ambRad);
    cb = alpha * (c.z * A.amb.z * A.ambRad);
  }
  const size_t p = (size_t)x + (size_t)A.W * (size_t)y;
  write_pixel<true>(A, p, cr, cg, cb, alpha, A.srgbTh, A.accum[p]);
  if (S.value) __builtin_nontemporal_store(v, &S.value[p]);
}

template <int O>
void launch_column(const RenderArgs &A, const ColumnArgs &S, bool render, hipStream_t s) {
  if (render)
    hipLaunchKernelGGL(k_render_column<O>, sample_grid(S.numPackets), dim3(64), 0, s, A, S);
  else
    hipLaunchKernelGGL(k_column_latlon<O>, sample_grid(S.n), dim3(64), 0, s, A, S);
}

// the three instantiations irt_sample.hip's launch_sample chooses between
void launch_column(int mode, const RenderArgs &A, const ColumnArgs &S, bool render, hipStream_t s) {
  if (mode != IRT_MODE_USER_GEOM)
    launch_column<kSamplerVariant>(A, S, render, s);
  else if (A.slots)
    launch_column<kCellVariant | OPT_SLOT>(A, S, render, s);
  else
    launch_column<kCellVariant>(A, S, render, s);
}

}  // namespace
}  // namespace irt

using namespace irt;

extern "C" {

int irt_column_latlon(irt_context *c, int mode, const float *lat, int numLat, const float *lon, int numLon,
                      const float *radius, const float *weight, int numLevels, irt_column_out d_out,
                      float missValue, void *stream) {
  const char *what = "irt_column_latlon";
  int rc = sample_check(c, mode, what);
  if (rc) return rc;
  size_t total = 0;
  if ((rc = latlon_args(what, lat, numLat, lon, numLon, radius, numLevels, &total))) return rc;
  if ((rc = column_weights(what, weight, numLevels))) return rc;
  if (total == 0) return IRT_OK;
  if (!d_out.wsum && !d_out.vmax && !d_out.vmin && !d_out.kmax && !d_out.kmin && !d_out.count) return IRT_OK;
  hipStream_t s = (hipStream_t)stream;
  if ((rc = sample_begin(c, s))) return rc;
  // the tables: through the context's pinned staging into its device copy
  const size_t nLat = 2 * (size_t)numLat, nLon = 2 * (size_t)numLon, nLev = (size_t)numLevels;
  const size_t need = nLat + nLon + nLev + (weight ? nLev : 0);
  if ((rc = sample_tab_reserve(c, need))) return rc;
  float *h = c->h_sampleTab;
  latlon_trig(lat, numLat, lon, numLon, h, h + nLat);
  memcpy(h + nLat + nLon, radius, nLev * sizeof(float));
  if (weight) memcpy(h + nLat + nLon + nLev, weight, nLev * sizeof(float));
  if ((rc = sample_tab_upload(c, need, s))) return rc;

  RenderArgs A;
  scene_args(c, mode, A);
  ColumnArgs S;
  memset(&S, 0, sizeof(S));
  S.latCS = c->d_sampleTab;
  S.lonCS = S.latCS + nLat;
  S.radius = S.lonCS + nLon;
  S.weight = weight ? S.radius + nLev : nullptr;
  S.numLat = numLat;
  S.numLon = numLon;
  S.numLevels = numLevels;
  S.patchesLon = ((uint32_t)numLon + 7u) / 8u;
  S.n = (unsigned long long)(((uint32_t)numLat + 7u) / 8u) * S.patchesLon;  // < 2^56
  S.out = d_out;
  S.missValue = missValue;
  S.rLo = c->info.sphericalBounds.lower.x;
  S.rHi = c->info.sphericalBounds.upper.x;
  launch_column(mode, A, S, false, s);
  return sample_end(c, s);
}

int irt_render_column(irt_context *c, const irt_launch_params *lp, int width, int height, float surfaceRadius,
                      const float *radius, const float *weight, int numLevels, int product, uint32_t *d_fb,
                      irt_vec4f *d_accum, float *d_value, float missValue, void *stream) {
  const char *what = "irt_render_column";
  if (c && !c->building && !lp) {
    set_error("%s: null lp", what);
    return IRT_E_INVALID;
  }
  int rc = sample_check(c, lp ? lp->mode : IRT_MODE_USER_GEOM, what);
  if (rc) return rc;
  if (!c->tfSet) {
    set_error("%s: no transfer function set (irt_set_transfunc)", what);
    return IRT_E_INVALID;
  }
  if (!(isfinite(surfaceRadius) && surfaceRadius > 0.f)) {
    set_error("%s: surfaceRadius = %g is not finite and positive", what, (double)surfaceRadius);
    return IRT_E_INVALID;
  }
  if ((rc = column_levels_args(what, radius, weight, numLevels))) return rc;
  if (product != IRT_COLUMN_WSUM && product != IRT_COLUMN_MAX && product != IRT_COLUMN_MIN) {
    set_error("%s: product %d is none of IRT_COLUMN_WSUM, IRT_COLUMN_MAX, IRT_COLUMN_MIN", what, product);
    return IRT_E_INVALID;
  }
  // (write_pixel's size_t indices would hold more; 2^27 is where irt_render's chained frames stop)
  if (width < 1 || height < 1 || (uint64_t)width * (uint64_t)height >= (uint64_t(1) << 27)) {
    set_error("%s: a frame of %d x %d pixels (at least 1 x 1, fewer than 2^27 pixels)", what, width, height);
    return IRT_E_INVALID;
  }
  if (!d_fb || !d_accum) {
    set_error("%s: null d_fb or d_accum", what);
    return IRT_E_INVALID;
  }
  hipStream_t s = (hipStream_t)stream;
  if ((rc = sample_begin(c, s))) return rc;
  // the radii and the weights: too many for by-value arguments, so through the device table
  const size_t nLev = (size_t)numLevels, need = nLev + (weight ? nLev : 0);
  if ((rc = sample_tab_reserve(c, need))) return rc;
  memcpy(c->h_sampleTab, radius, nLev * sizeof(float));
  if (weight) memcpy(c->h_sampleTab + nLev, weight, nLev * sizeof(float));
  if ((rc = sample_tab_upload(c, need, s))) return rc;

  RenderArgs A;
  scene_args(c, lp->mode, A);
  frame_args(c, lp, d_fb, d_accum, A);
  A.W = width;
  A.H = height;
  ColumnArgs S;
  memset(&S, 0, sizeof(S));
  S.radius = c->d_sampleTab;
  S.weight = weight ? S.radius + nLev : nullptr;
  S.numLevels = numLevels;
  S.packetsX = ((uint32_t)width + 7u) / 8u;
  S.numPackets = S.packetsX * (((uint32_t)height + 7u) / 8u);  // <= width * height < 2^27
  S.surfaceRadius = surfaceRadius;
  S.product = product;
  S.value = d_value;
  S.missValue = missValue;
  S.rLo = c->info.sphericalBounds.lower.x;
  S.rHi = c->info.sphericalBounds.upper.x;
  launch_column(lp->mode, A, S, true, s);
  return sample_end(c, s);
}

}  // extern "C"
