// irt_levels.hip -- level surfaces (include/icon_rt_hip.h, "level surfaces"): per pixel the raygen's
// own ray (irt_raygen.h gen_ray), its hits with the levels' spheres (irt_device.h intersect_sphere),
// the field's value at each hit through the point location of irt_sample_points (irt_sample_dev.h
// wave_locate), classified (Tracer::post_classify), composited front to back and written as the
// raygen writes a pixel (irt_raygen.h write_pixel).  The kernel and the context entry point; the
// host side (the check and the order of the radii) is host/irt_level_order.cpp.
//
// The guard argument of irt_sample_dev.h covers the hit points unchanged: whatever float triple
// org + dir * t comes to, it reaches a locator only through admit().

#include <hip/hip_runtime.h>
#include <string.h>

#include "irt_context.h"
#include "irt_raygen.h"
#include "irt_sample_dev.h"

namespace irt {

// What the kernel needs beyond RenderArgs (which stays the kernel's FIRST argument: Tracer's late
// reads go through fresh_args(), the kernarg segment read as a RenderArgs).  The levels are in
// near order (host/irt_level_order.cpp levels_order): slot h < numLevels is the near hit of radius[h],
// slot numLevels + h the far hit of radius[numLevels - 1 - h].
struct LevelArgs {
  float radius[IRT_MAX_LEVELS];   // descending, ties by ascending caller index
  int32_t index[IRT_MAX_LEVELS];  // the caller's index of each
  int numLevels;
  int flags;
  uint32_t packetsX;    // 8 x 8 pixel packets per packet row
  uint32_t numPackets;  // ... and in the frame
  float *value;         // may be null
  int32_t *level;       // may be null
  float missValue;
  float rLo, rHi;       // the scene's sphericalBounds.lower.x / upper.x (cell sampler's cut)
};

namespace {

// One wave per workgroup, one 8 x 8 pixel packet per wave (lane = 8 dy + dx, the raygen's packet:
// neighbouring lanes share header lines, fat entries and height/value blocks).  Lanes outside the
// frame stay in the wave and never want a point; the slot loop's bounds and its skip of a slot no
// lane has a hit in are wave-uniform, as Tracer::locate_wave needs every lane to call it.
template <int O>
__global__ void __launch_bounds__(64) k_render_levels(RenderArgs A, LevelArgs S) {
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
  Tracer<O> T{{}, A, nullptr, A.sphBits, L.cnt, {0, 0, 0, 0, 0, 0, 0}};  // post_classify
  float cr = 0.f, cg = 0.f, cb = 0.f, alpha = 0.f;
  float first = S.missValue;
  int32_t firstLevel = -1;
  const int n = S.numLevels;
  const bool back = (S.flags & IRT_LEVELS_BACK) != 0;
#pragma nounroll
  for (int s = 0; s < 2 * n; ++s) {
    const bool far = s >= n;
    const int k = far ? 2 * n - 1 - s : s;
    float tn = 0.f, tf = 0.f;
    const bool hit = inFrame && intersect_sphere(ray, S.radius[k], tn, tf);
    // the far slot of a sphere whose near slot is live (the camera is outside it): IRT_LEVELS_BACK only
    const bool live = hit && (far ? tf > 0.f && (back || !(tn > 0.f)) : tn > 0.f);
    if (__ballot(live) == 0ull) continue;
    const float t = far ? tf : tn;
    const float X = ray.ox + ray.dx * t, Y = ray.oy + ray.dy * t, Z = ray.oz + ray.dz * t;
    float v = 0.f;
    if (wave_locate<O>(A, S.rLo, S.rHi, live, X, Y, Z, v, L)) {  // per lane from here
      if (firstLevel < 0) {
        first = v;
        firstLevel = S.index[k];
      }
      const float4 c = T.post_classify(v);
      const float a = c.w < 0.f ? 0.f : (c.w > 1.f ? 1.f : c.w);
      const float wgt = (1.f - alpha) * a;
      cr = cr + wgt * (c.x * A.amb.x * A.ambRad);  // the raygen's products (deviceCode.cu:318)
      cg = cg + wgt * (c.y * A.amb.y * A.ambRad);
      cb = cb + wgt * (c.z * A.amb.z * A.ambRad);
      alpha = alpha + wgt;
    }
  }
  if (!inFrame) return;
  const size_t p = (size_t)x + (size_t)A.W * (size_t)y;
  write_pixel<true>(A, p, cr, cg, cb, alpha, A.srgbTh, A.accum[p]);
  if (S.value) __builtin_nontemporal_store(first, &S.value[p]);
  if (S.level) __builtin_nontemporal_store(firstLevel, &S.level[p]);
}

template <int O>
void launch_levels(const RenderArgs &A, const LevelArgs &S, hipStream_t s) {
  hipLaunchKernelGGL(k_render_levels<O>, sample_grid(S.numPackets), dim3(64), 0, s, A, S);
}

}  // namespace
}  // namespace irt

using namespace irt;

extern "C" int irt_render_levels(irt_context *c, const irt_launch_params *lp, int width, int height,
                                 const float *radius, int numLevels, int flags, uint32_t *d_fb, irt_vec4f *d_accum,
                                 float *d_value, int32_t *d_level, float missValue, void *stream) {
  const char *what = "irt_render_levels";
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
  if ((rc = levels_args(what, radius, numLevels))) return rc;
  if (flags & ~IRT_LEVELS_BACK) {
    set_error("%s: unknown flag bits 0x%x", what, (unsigned)(flags & ~IRT_LEVELS_BACK));
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
  RenderArgs A;
  scene_args(c, lp->mode, A);
  frame_args(c, lp, d_fb, d_accum, A);
  A.W = width;
  A.H = height;
  LevelArgs S;
  memset(&S, 0, sizeof(S));
  levels_order(radius, numLevels, S.radius, S.index);
  S.numLevels = numLevels;
  S.flags = flags;
  S.packetsX = ((uint32_t)width + 7u) / 8u;
  S.numPackets = S.packetsX * (((uint32_t)height + 7u) / 8u);  // <= width * height < 2^27
  S.value = d_value;
  S.level = d_level;
  S.missValue = missValue;
  S.rLo = c->info.sphericalBounds.lower.x;
  S.rHi = c->info.sphericalBounds.upper.x;
  if (lp->mode != IRT_MODE_USER_GEOM)
    launch_levels<kSamplerVariant>(A, S, s);
  else if (A.slots)
    launch_levels<kCellVariant | OPT_SLOT>(A, S, s);
  else
    launch_levels<kCellVariant>(A, S, s);
  return sample_end(c, s);
}
