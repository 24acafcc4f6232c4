// irt_section.hip -- vertical cross-sections and station columns (include/icon_rt_hip.h, "sections"):
// the field on the levels of columns at arbitrary (lat, lon) pairs -- a great-circle track, a station
// list -- as values, as a classified RGBA8 curtain and as the column products of irt_column.h, in one
// pass.  A wave keeps its 64 consecutive pairs for all levels, as k_column_latlon keeps its patch;
// each level's points go through the point location of irt_sample_points (irt_sample_dev.h
// wave_locate).  The host side (the argument checks, irt_section_points, irt_great_circle) is
// host/irt_section.cpp.
//
// The guard argument of irt_sample_dev.h covers the section points unchanged: whatever float triple
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

// What the kernel needs beyond RenderArgs (which stays the kernel's FIRST argument: Tracer's late
// reads go through fresh_args(), the kernarg segment read as a RenderArgs)
struct SectionArgs {
  const float4 *trig;    // {cosf lat, sinf lat, cosf lon, sinf lon} per column
  const float *radius;   // the levels' radii
  const float *weight;   // ... and weights; null: every weight 1.0f
  unsigned long long numColumns;
  unsigned long long numWaves;  // (numColumns + 63) / 64
  int numLevels;
  float *value;          // [k * numColumns + c], may be null
  uint8_t *found;        // ... may be null
  uint32_t *rgba;        // ... may be null
  irt_column_out column; // [c], each may be null
  float missValue;
  float rLo, rHi;        // the scene's sphericalBounds.lower.x / upper.x (cell sampler's cut)
};

namespace {

template <typename T>
__device__ __forceinline__ void put(T *out, unsigned long long i, T v) {
  if (out) __builtin_nontemporal_store(v, &out[i]);  // streaming: nobody re-reads it in this kernel
}

// Wave w takes columns 64 w .. 64 w + 63 (a shift and an add: consecutive track points are
// neighbours on the globe and share header lines) and walks them up the levels as irt_column.hip's
// walk_columns does -- wave-uniform bounds, scalar reads of the level's radius and weight, every
// lane calling wave_locate -- with one difference: a level no lane is admitted at is not left with
// `continue`, because its per-point outputs are still due (missValue, 0, 0).  Only the locator is
// skipped there.  A lane's four trig values are read once; the per-point stores at
// [k * numColumns + c] are consecutive across the wave.
template <int O>
__global__ void __launch_bounds__(64) k_section(RenderArgs A, SectionArgs S) {
  constexpr bool kCell = (O & OPT_WEDGE) == 0;
  __shared__ SampleLds<kCell> L;
  const unsigned long long w = workgroup_index();
  if (w >= S.numWaves) return;  // wave-uniform (the last grid row's tail)
  const unsigned long long c = (w << 6) + threadIdx.x;
  const bool live = c < S.numColumns;  // live lanes index the trig table inside its size
  float t[4] = {0.f, 0.f, 0.f, 0.f};
  if (live) {
    const float4 q = S.trig[c];
    t[0] = q.x;
    t[1] = q.y;
    t[2] = q.z;
    t[3] = q.w;
  }
  const irt_column_out &co = S.column;
  const bool wantColumn = co.wsum || co.vmax || co.vmin || co.kmax || co.kmin || co.count;
  Tracer<O> T{{}, A, nullptr, A.sphBits, L.cnt, {0, 0, 0, 0, 0, 0, 0}};  // post_classify
  ColumnAcc a;
  column_init(a);
#pragma nounroll
  for (int k = 0; k < S.numLevels; ++k) {
    const float r = S.radius[k];
    const float wgt = S.weight ? S.weight[k] : 1.f;
    float x, y, z;
    to_cartesian_trig(r, t, x, y, z);
    float v = 0.f;
    bool hit = false;
    // a lane the guard turns away is a miss of wave_locate in any case, so the skip changes no result
    if (__ballot(live && admit<kCell>(S.rLo, S.rHi, x, y, z)) != 0ull)
      hit = wave_locate<O>(A, S.rLo, S.rHi, live, x, y, z, v, L);  // per lane from here
    if (hit && wantColumn) column_step(a, k, wgt, v);
    if (!live) continue;
    const unsigned long long p = (unsigned long long)k * S.numColumns + c;  // < 2^36
    put(S.value, p, hit ? v : S.missValue);
    put(S.found, p, (uint8_t)(hit ? 1 : 0));
    if (S.rgba) {
      uint32_t px = 0u;
      if (hit) {
        // what write_pixel (irt_raygen.h) stores for (C, alpha) at accumID 0, without its accum
        const float4 s = T.post_classify(v);
        const float alpha = s.w < 0.f ? 0.f : (s.w > 1.f ? 1.f : s.w);
        const float cr = alpha * (s.x * A.amb.x * A.ambRad);  // the raygen's products (deviceCode.cu:318)
        const float cg = alpha * (s.y * A.amb.y * A.ambRad);
        const float cb = alpha * (s.z * A.amb.z * A.ambRad);
        px = srgb_byte(A.srgbTh, cr) + (srgb_byte(A.srgbTh, cg) << 8) + (srgb_byte(A.srgbTh, cb) << 16) +
             (make_8bit(alpha) << 24);
      }
      __builtin_nontemporal_store(px, &S.rgba[p]);
    }
  }
  if (!live || !wantColumn) return;
  column_finish(a, S.missValue);
  put(co.wsum, c, a.wsum);
  put(co.vmax, c, a.mx);
  put(co.vmin, c, a.mn);
  put(co.kmax, c, a.kmax);
  put(co.kmin, c, a.kmin);
  put(co.count, c, a.count);
}

template <int O>
void launch_section(const RenderArgs &A, const SectionArgs &S, hipStream_t s) {
  hipLaunchKernelGGL(k_section<O>, sample_grid(S.numWaves), dim3(64), 0, s, A, S);
}

}  // namespace
}  // namespace irt

using namespace irt;

extern "C" int irt_section(irt_context *c, int mode, const float *lat, const float *lon, int numColumns,
                           const float *radius, const float *weight, int numLevels, irt_vec3f ambientColor,
                           float ambientRadiance, irt_section_out d_out, float missValue, void *stream) {
  const char *what = "irt_section";
  int rc = sample_check(c, mode, what);
  if (rc) return rc;
  size_t total = 0;
  if ((rc = section_args(what, lat, lon, numColumns, radius, numLevels, &total))) return rc;
  if ((rc = column_weights(what, weight, numLevels))) return rc;
  if (d_out.rgba) {
    if (!c->tfSet) {
      set_error("%s: rgba asked for with no transfer function set (irt_set_transfunc)", what);
      return IRT_E_INVALID;
    }
    if (!(isfinite(ambientColor.x) && isfinite(ambientColor.y) && isfinite(ambientColor.z) &&
          isfinite(ambientRadiance))) {
      set_error("%s: rgba asked for with a non-finite ambientColor or ambientRadiance", what);
      return IRT_E_INVALID;
    }
  }
  if (total == 0) return IRT_OK;
  const irt_column_out &co = d_out.column;
  if (!d_out.value && !d_out.found && !d_out.rgba && !co.wsum && !co.vmax && !co.vmin && !co.kmax && !co.kmin &&
      !co.count)
    return IRT_OK;
  hipStream_t s = (hipStream_t)stream;
  if ((rc = sample_begin(c, s))) return rc;
  // the tables: through the context's pinned staging into its device copy.  The trig table first:
  // the device copy's start is aligned for its 16-byte reads
  const size_t nCol = (size_t)numColumns, nLev = (size_t)numLevels;
  const size_t need = 4 * nCol + nLev + (weight ? nLev : 0);
  if ((rc = sample_tab_reserve(c, need))) return rc;
  float *h = c->h_sampleTab;
  section_trig(lat, lon, numColumns, h);
  memcpy(h + 4 * nCol, radius, nLev * sizeof(float));
  if (weight) memcpy(h + 4 * nCol + nLev, weight, nLev * sizeof(float));
  if ((rc = sample_tab_upload(c, need, s))) return rc;

  RenderArgs A;
  scene_args(c, mode, A);
  if (d_out.rgba) {  // the classification and the pixel conversion, as a frame of accumID 0 takes them
    irt_launch_params lp;
    memset(&lp, 0, sizeof(lp));
    lp.ambientColor = ambientColor;
    lp.ambientRadiance = ambientRadiance;
    frame_args(c, &lp, nullptr, nullptr, A);
  }
  SectionArgs S;
  memset(&S, 0, sizeof(S));
  S.trig = reinterpret_cast<const float4 *>(c->d_sampleTab);
  S.radius = c->d_sampleTab + 4 * nCol;
  S.weight = weight ? S.radius + nLev : nullptr;
  S.numColumns = nCol;
  S.numWaves = (nCol + 63) / 64;  // <= 2^25: one grid row
  S.numLevels = numLevels;
  S.value = d_out.value;
  S.found = d_out.found;
  S.rgba = d_out.rgba;
  S.column = d_out.column;
  S.missValue = missValue;
  S.rLo = c->info.sphericalBounds.lower.x;
  S.rHi = c->info.sphericalBounds.upper.x;
  // the three instantiations irt_sample.hip's launch_sample chooses between
  if (mode != IRT_MODE_USER_GEOM)
    launch_section<kSamplerVariant>(A, S, s);
  else if (A.slots)
    launch_section<kCellVariant | OPT_SLOT>(A, S, s);
  else
    launch_section<kCellVariant>(A, S, s);
  return sample_end(c, s);
}
