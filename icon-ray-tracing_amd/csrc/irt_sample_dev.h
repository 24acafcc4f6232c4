// irt_sample_dev.h -- the device half the sampling translation units share (irt_sample.hip: points
// and lat/lon grids; irt_levels.hip: level surfaces; irt_column.hip: column products): the guard in front of the locator, a one-wave
// workgroup's LDS, sampleVolume of one wave's 64 points, and the sampling grids' workgroup index.
// Their host half (scene_args, sample_check, sample_begin, sample_end) is declared in irt_context.h.
//
// The raygen only ever hands the locator points inside the shell; the sampling entry points hand
// it anything.  admit() below is the guard, and says why every point it lets through indexes every
// table in bounds.
#pragma once

#include <algorithm>

#include "irt_tracer.h"

namespace irt {

// The guard.  Returns whether the point goes to the locator.  rLo, rHi: the scene's
// sphericalBounds.lower.x / upper.x (the cell sampler's cut).
//
// (1) sample_admits (irt_common.h): the squared length is finite and positive.  So the
//     coordinates are finite, the largest magnitude `den` is a normal float in [2^-76, 2^64),
//     and r = sqrtf(r2) is finite and positive.  From that, table by table:
//  - cube-map cell and sub-cell (cubemap_cell_fast, for G and for the wedge locator's wG):
//    rcpf(den) is finite and normal, |num| <= den, so (num * inv + 1) * fg is finite, in
//    [0, GS (1 + 2^-22)]; the int conversion is then clamped to [0, GS - 1] in any case, so
//    cell < 6 G^2 and sub < kSubCells^2 for every float input.  binHdr holds 6 G^2 headers of
//    kBinHdrWords; wOff holds 6 wG^2 + 1 offsets.
//  - radial bin (bin_of): three compares, b in [0, 3]; the header's cumulative ends give
//    [beg, end) inside the cell's own entries by construction of the build.  The second pass
//    (b + 1, mask shift 8 (b + 1)) runs only when b < kMaxEdges, so the shift is at most 24.
//  - slot bin (OPT_SLOT): bin_of against slotEdge, whose unused edges are +inf.  r is finite,
//    so +inf < r is false: b <= the number of finite edges = slotBins - 1.  The slot index is
//    (cell * units + unit) * slotBins + b with unit < units: inside the table.
//  - sphere hash: sph_hash(r) >> 18 < 2^14 = 32 kSphBitWords bits, for every float; sphere_at
//    bisects [0, numSph) and reads sphOff[lo] with lo < numSph.
//  - candidates, height/value blocks, wedge CSR, boxes and trig: indexed by entry positions and
//    record numbers the build stored, never by anything computed from the point.
//  - getValue (record_value, find_value_literal): runs only for a record whose radial test
//    h0 <= r <= hN passed, as in the raygen; the literal search is bounded by numLayers <= 31.
//  - locate_tri divides by len = r > 0, finite.
// (2) the cell sampler's shell cut: r outside [sphericalBounds.lower.x, upper.x] = [min
//     height[0], max height[numLayers]] fails every record's radial test (ICONGrid.h:184), the
//     reference's own miss; nothing is read for it.  An empty scene's bounds are (+inf, -inf):
//     everything is cut.
template <bool kCell>
__device__ __forceinline__ bool admit(float rLo, float rHi, float x, float y, float z) {
  if (!sample_admits(x, y, z)) return false;
  if constexpr (kCell) {
    const float r = sqrtf(dot3(x, y, z, x, y, z));  // toSpherical(pos).x, as locate_wave takes it
    if (!(r >= rLo && r <= rHi)) return false;
  }
  return true;
}

// A one-wave workgroup's LDS: the wave-wide scan's records (cell sampler only) and the Tracer's
// count words (its serial forms add into them; the forms run here never do)
template <bool kCell>
struct SampleLds {
  CoopWave coop;
  ScanWave scan;
  uint32_t cnt[kCnt];
};
template <>
struct SampleLds<false> {
  uint32_t cnt[kCnt];
};

// sampleVolume of one wave's 64 points.  `live`: the lane has a point; every lane calls.
template <int O>
__device__ __forceinline__ bool wave_locate(const RenderArgs &A, float rLo, float rHi, bool live, float x, float y,
                                            float z, float &v, SampleLds<(O & OPT_WEDGE) == 0> &L) {
  constexpr bool kCell = (O & OPT_WEDGE) == 0;
  const bool want = live && admit<kCell>(rLo, rHi, x, y, z);
  // the sphere hash from global memory, as the raygen's lean kernels read it
  Tracer<O> T{{}, A, nullptr, A.sphBits, L.cnt, {0, 0, 0, 0, 0, 0, 0}};
  if constexpr (kCell) {
    static_assert(Tracer<O>::kWaveScan, "the cell sampler scans wave-wide");
    return T.locate_wave(want, x, y, z, v, L.coop, L.scan);
  } else {
    return want && T.locate(x, y, z, v);
  }
}

// Workgroup w of a sampling grid: one wave each, kGridRow to a grid row (64 kGridRow threads stay
// below the 2^32 threads a grid's x dimension may hold), the rows in grid y -- at most 32 of them
// for kSampleMaxPoints points.
constexpr unsigned long long kGridRow = 1ull << 25;
__device__ __forceinline__ unsigned long long workgroup_index() {
  return (unsigned long long)blockIdx.x + kGridRow * (unsigned long long)blockIdx.y;
}
inline dim3 sample_grid(unsigned long long wgs) {
  return dim3((unsigned)std::min(wgs, kGridRow), (unsigned)((wgs + kGridRow - 1) / kGridRow));
}

// the cell sampler's Tracer, as k_debug_locate_wave instantiates it: from headers (with the
// quad-bound miss test), or from the slot table where the context's frames start there
constexpr int kCellVariant = kDefaultVariant & ~OPT_MONO;

}  // namespace irt
