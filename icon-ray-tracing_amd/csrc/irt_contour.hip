// irt_contour.hip -- isolines of a value grid on the device (include/icon_rt_hip.h, "isolines"; the
// definition is irt_contour.h): three passes from a lat x lon value grid to a compact segment array
// in the definition's order -- count, scan, emit -- and the context entry points irt_contour_grid
// and irt_contour_latlon.  The host side (the argument check, the trig tables, irt_contour_cells) is
// host/irt_contour.cpp.
//
// No pass uses a global atomic: a segment's index is the scanned total of its (threshold, workgroup)
// plus its place among the workgroup's lanes, so every run writes the same bytes to the same places.
// The kernels read no scene array and run no Tracer.

#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>

#include <algorithm>

#include "irt_context.h"
#include "irt_contour.h"

namespace irt {
namespace {

constexpr int kCtrWG = 256;             // cells per workgroup of the count and emit passes: 4 waves
constexpr int kCtrWaves = kCtrWG / 64;
constexpr int kScanWG = 256;            // threads of the scan's one workgroup ...
constexpr int kScanPer = 4;             // ... and consecutive entries per thread and round
constexpr int kMaxT = IRT_CONTOUR_MAX_THRESHOLDS;

struct ContourArgs {
  const float *value;
  const uint8_t *found;        // may be null
  const double *latC, *latS, *lonC, *lonS;
  const float *threshold;      // T, device
  const int32_t *style;        // T, device
  int numLon, cellsLon, T;
  uint32_t numCells, numWG;
  uint32_t *packed;            // per cell: 2 bits per threshold, the kept segments
  uint32_t *totals;            // T x numWG: per-workgroup counts, after the scan their exclusive sums
  unsigned long long *counts;  // kMaxT per-threshold counts, then the total
  irt_overlay_segment *out;
  unsigned long long total;    // emit: the segments d_out holds
};

__device__ __forceinline__ uint32_t popc64(unsigned long long m) { return (uint32_t)__popcll(m); }

// the cell of this lane: false for a lane past the grid or a cell that emits nothing
__device__ __forceinline__ bool load_cell(const ContourArgs &A, uint32_t cell, ContourCell &K) {
  const int j = (int)(cell / (uint32_t)A.cellsLon), i = (int)(cell - (uint32_t)j * (uint32_t)A.cellsLon);
  const int i1 = i + 1 == A.numLon ? 0 : i + 1;  // rows j, j + 1 < numLat and columns i, i1 < numLon
  return ctr_load(A.value, A.found, A.latC, A.latS, A.lonC, A.lonS, A.numLon, j, i, i1, K);
}

// Pass 1.  One lane per cell: the kept segments of every threshold as a packed word, and the
// workgroup's total per threshold from wave ballots (a lane keeps 0, 1 or 2 segments: two ballots).
__global__ void __launch_bounds__(kCtrWG) k_contour_count(ContourArgs A) {
  __shared__ uint32_t waveTotal[kMaxT][kCtrWaves];
  const uint32_t cell = blockIdx.x * (uint32_t)kCtrWG + threadIdx.x;
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
  ContourCell K;
  const bool ok = cell < A.numCells && load_cell(A, cell, K);
  uint32_t packed = 0u;
  for (int t = 0; t < A.T; ++t) {  // T is launch-uniform: every lane takes every ballot
    uint32_t cnt = 0u;
    if (ok) {
      irt_overlay_segment s0, s1;
      const uint32_t kept = ctr_eval<false>(K, A.threshold[t], 0, s0, s1);
      cnt = (kept & 1u) + (kept >> 1);
    }
    packed |= cnt << (2 * t);
    const uint32_t total = popc64(__ballot(cnt & 1u)) + 2u * popc64(__ballot(cnt & 2u));
    if (lane == 0u) waveTotal[t][wave] = total;
  }
  if (cell < A.numCells) A.packed[cell] = packed;
  __syncthreads();
  if (threadIdx.x < (uint32_t)A.T) {
    uint32_t sum = 0u;
    for (int w = 0; w < kCtrWaves; ++w) sum += waveTotal[threadIdx.x][w];
    A.totals[(size_t)threadIdx.x * A.numWG + blockIdx.x] = sum;
  }
}

// Pass 2.  The exclusive scan of the T x numWG totals in (threshold, workgroup) order, in place, by
// one workgroup that takes kScanWG * kScanPer entries per round; then the counts per threshold and
// the total (64-bit: 2^27 cells x 2 segments x 16 thresholds reaches 2^32; the stored sums are its
// low words, exact whenever the total passes the 2^24 limit the call then applies).
__global__ void __launch_bounds__(kScanWG) k_contour_scan(ContourArgs A) {
  __shared__ uint32_t waveSum[kScanWG / 64];
  const uint32_t n = (uint32_t)A.T * A.numWG;  // < 16 * 2^19
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
  unsigned long long carry = 0ull;
  for (uint32_t base = 0u; base < n; base += (uint32_t)(kScanWG * kScanPer)) {
    const uint32_t at = base + (uint32_t)kScanPer * threadIdx.x;
    uint32_t x[kScanPer], sum = 0u;
    for (int k = 0; k < kScanPer; ++k) {
      x[k] = at + (uint32_t)k < n ? A.totals[at + (uint32_t)k] : 0u;
      sum += x[k];
    }
    uint32_t incl = sum;  // the wave's inclusive scan
    for (int d = 1; d < 64; d <<= 1) {
      const uint32_t y = __shfl_up(incl, d);
      if (lane >= (uint32_t)d) incl += y;
    }
    if (lane == 63u) waveSum[wave] = incl;
    __syncthreads();
    uint32_t before = 0u, all = 0u;
    for (uint32_t w = 0u; w < (uint32_t)(kScanWG / 64); ++w) {
      if (w < wave) before += waveSum[w];
      all += waveSum[w];
    }
    uint32_t run = (uint32_t)carry + before + (incl - sum);
    for (int k = 0; k < kScanPer; ++k) {
      if (at + (uint32_t)k < n) A.totals[at + (uint32_t)k] = run;
      run += x[k];
    }
    carry += all;  // (a round's entries sum to at most 1024 * 512: no wrap inside a round)
    __syncthreads();  // waveSum is rewritten next round; the stores above are visible to the block below
  }
  if (threadIdx.x < (uint32_t)A.T) {
    const uint32_t t = threadIdx.x;
    const uint32_t start = A.totals[(size_t)t * A.numWG];
    const uint32_t next = t + 1u < (uint32_t)A.T ? A.totals[(size_t)(t + 1u) * A.numWG] : (uint32_t)carry;
    A.counts[t] = (unsigned long long)(uint32_t)(next - start);  // one threshold: at most 2^28
  }
  if (threadIdx.x == 0u) A.counts[kMaxT] = carry;
}

__device__ __forceinline__ void store_segment(irt_overlay_segment *dst, const irt_overlay_segment &s) {
  typedef float f4v __attribute__((ext_vector_type(4)));
  f4v *p = reinterpret_cast<f4v *>(dst);  // 64-byte aligned (checked by the call)
  const f4v v0 = {s.a[0], s.a[1], s.a[2], s.b[0]}, v1 = {s.b[1], s.b[2], s.n[0], s.n[1]},
            v2 = {s.n[2], s.t[0], s.t[1], s.t[2]}, v3 = {s.sinHalf, u2f((uint32_t)s.style), 0.f, 0.f};
  __builtin_nontemporal_store(v0, p);
  __builtin_nontemporal_store(v1, p + 1);
  __builtin_nontemporal_store(v2, p + 2);
  __builtin_nontemporal_store(v3, p + 3);
}

// Pass 3.  The grid of pass 1.  A lane's first segment of threshold t goes to the scanned total of
// (t, workgroup) + the totals of the workgroup's earlier waves + the lanes before it in its wave,
// from the packed counts; the lane runs the definition again and writes each kept segment as one
// 64-byte line.
__global__ void __launch_bounds__(kCtrWG) k_contour_emit(ContourArgs A) {
  __shared__ uint32_t waveTotal[kMaxT][kCtrWaves];
  const uint32_t cell = blockIdx.x * (uint32_t)kCtrWG + threadIdx.x;
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
  const unsigned long long below = (1ull << lane) - 1ull;
  const uint32_t packed = cell < A.numCells ? A.packed[cell] : 0u;
  for (int t = 0; t < A.T; ++t) {
    const uint32_t cnt = (packed >> (2 * t)) & 3u;
    const uint32_t total = popc64(__ballot(cnt & 1u)) + 2u * popc64(__ballot(cnt & 2u));
    if (lane == 0u) waveTotal[t][wave] = total;
  }
  __syncthreads();
  ContourCell K;
  const bool ok = packed != 0u && load_cell(A, cell, K);  // (packed != 0: the cell is inside the grid)
  for (int t = 0; t < A.T; ++t) {
    const uint32_t cnt = (packed >> (2 * t)) & 3u;
    const uint32_t prefix = popc64(__ballot(cnt & 1u) & below) + 2u * popc64(__ballot(cnt & 2u) & below);
    if (ok && cnt != 0u) {  // (no ballot inside)
      uint32_t at = A.totals[(size_t)t * A.numWG + blockIdx.x] + prefix;
      for (uint32_t w = 0u; w < wave; ++w) at += waveTotal[t][w];
      irt_overlay_segment s0, s1;
      const uint32_t kept = ctr_eval<true>(K, A.threshold[t], A.style[t], s0, s1);
      // (kept has cnt bits, by the same code on the same input; the compare keeps a store inside
      // d_out whatever happens)
      if ((kept & 1u) && (unsigned long long)at < A.total) store_segment(A.out + at, s0);
      at += kept & 1u;
      if ((kept & 2u) && (unsigned long long)at < A.total) store_segment(A.out + at, s1);
    }
  }
}

// The context's contour scratch (irt_context.h): the device block -- tables, thresholds, styles,
// counts, packed words, totals -- and the pinned block (the tables' staging, the counts' landing),
// both grown on demand.  A larger block replaces the old one only once every sampling call issued
// so far has run.
struct Layout {
  size_t tab, thr, sty, counts, packed, totals, bytes;  // byte offsets into the device block
  size_t hostTab, hostCounts, hostBytes;                // ... and into the pinned block
};
size_t up(size_t x) { return (x + 255) & ~size_t(255); }
Layout layout(int numLat, int numLon, uint32_t numCells, uint32_t numWG) {
  Layout L;
  const size_t tabBytes = 2 * ((size_t)numLat + (size_t)numLon) * sizeof(double);
  L.tab = 0;
  L.thr = up(tabBytes);
  L.sty = L.thr + up(kMaxT * sizeof(float));
  L.counts = L.sty + up(kMaxT * sizeof(int32_t));
  L.packed = L.counts + up((kMaxT + 1) * sizeof(unsigned long long));
  L.totals = L.packed + up((size_t)numCells * sizeof(uint32_t));
  L.bytes = L.totals + up((size_t)kMaxT * numWG * sizeof(uint32_t));
  // the pinned block mirrors the first three device regions (one upload) and adds the counts
  L.hostTab = 0;
  L.hostCounts = L.counts;
  L.hostBytes = L.packed;
  return L;
}

int reserve(irt_context *c, const Layout &L) {
  if (L.bytes > c->contourCap || L.hostBytes > c->contourHostCap) {
    IRT_HIP(wait_samples(c));
    if (c->d_contour) {
      IRT_HIP(hipFree(c->d_contour));
      c->d_contour = nullptr;
      c->bytes -= std::min(c->bytes, c->contourCap);
    }
    if (c->h_contour) {
      IRT_HIP(hipHostFree(c->h_contour));
      c->h_contour = nullptr;
    }
    c->contourCap = c->contourHostCap = 0;
    c->info.deviceBytes = c->bytes;
    const size_t cap = L.bytes + L.bytes / 2, hostCap = L.hostBytes + L.hostBytes / 2;
    IRT_HIP(hipHostMalloc((void **)&c->h_contour, hostCap));
    c->contourHostCap = hostCap;
    IRT_HIP(hipMalloc((void **)&c->d_contour, cap));
    c->contourCap = cap;
    c->bytes += cap;
    c->info.deviceBytes = c->bytes;
  }
  return IRT_OK;
}

}  // namespace
}  // namespace irt

using namespace irt;

void free_contour_state(irt_context *c) {
  if (c->d_contour) (void)hipFree(c->d_contour);
  if (c->h_contour) (void)hipHostFree(c->h_contour);
  if (c->d_contourGrid) (void)hipFree(c->d_contourGrid);
  c->d_contour = c->h_contour = c->d_contourGrid = nullptr;
  c->contourCap = c->contourHostCap = c->contourGridCap = 0;
}

extern "C" {

int irt_contour_grid(irt_context *c, const float *d_value, const uint8_t *d_found, const float *lat, int numLat,
                     const float *lon, int numLon, const float *threshold, const int32_t *style, int numThresholds,
                     int flags, irt_overlay_segment *d_out, size_t capacity, size_t *count,
                     size_t *countPerThreshold, void *stream) {
  const char *what = "irt_contour_grid";
  int rc = sample_check(c, IRT_MODE_USER_GEOM, what);  // (no sampler is used: the cell mode asks for nothing)
  if (rc) return rc;
  if (!count) {
    set_error("%s: null count", what);
    return IRT_E_INVALID;
  }
  int cellsLon = 0;
  if ((rc = contour_args(what, lat, numLat, lon, numLon, threshold, style, numThresholds, flags, &cellsLon))) return rc;
  if (!d_value) {
    set_error("%s: null d_value", what);
    return IRT_E_INVALID;
  }
  if ((uintptr_t)d_out & 63u) {
    set_error("%s: d_out is not 64-byte aligned", what);
    return IRT_E_INVALID;
  }
  const uint32_t numCells = (uint32_t)(numLat - 1) * (uint32_t)cellsLon;  // < 2^27
  const uint32_t numWG = (numCells + (uint32_t)kCtrWG - 1u) / (uint32_t)kCtrWG;
  const Layout L = layout(numLat, numLon, numCells, numWG);
  hipStream_t s = (hipStream_t)stream;
  if ((rc = sample_begin(c, s))) return rc;
  if ((rc = reserve(c, L))) return rc;
  // the pinned block is free: every earlier call ended with its upload and its counts read
  char *h = (char *)c->h_contour, *d = (char *)c->d_contour;
  double *latC = (double *)(h + L.hostTab), *latS = latC + numLat, *lonC = latS + numLat, *lonS = lonC + numLon;
  contour_trig(lat, numLat, lon, numLon, latC, latS, lonC, lonS);
  memset(h + L.thr, 0, L.counts - L.thr);
  memcpy(h + L.thr, threshold, (size_t)numThresholds * sizeof(float));
  memcpy(h + L.sty, style, (size_t)numThresholds * sizeof(int32_t));
  IRT_HIP(hipMemcpyAsync(d, h, L.counts, hipMemcpyHostToDevice, s));

  ContourArgs A;
  memset(&A, 0, sizeof(A));
  A.value = d_value;
  A.found = d_found;
  A.latC = (const double *)(d + L.tab);
  A.latS = A.latC + numLat;
  A.lonC = A.latS + numLat;
  A.lonS = A.lonC + numLon;
  A.threshold = (const float *)(d + L.thr);
  A.style = (const int32_t *)(d + L.sty);
  A.numLon = numLon;
  A.cellsLon = cellsLon;
  A.T = numThresholds;
  A.numCells = numCells;
  A.numWG = numWG;
  A.packed = (uint32_t *)(d + L.packed);
  A.totals = (uint32_t *)(d + L.totals);
  A.counts = (unsigned long long *)(d + L.counts);
  A.out = d_out;
  hipLaunchKernelGGL(k_contour_count, dim3(numWG), dim3(kCtrWG), 0, s, A);
  hipLaunchKernelGGL(k_contour_scan, dim3(1), dim3(kScanWG), 0, s, A);
  IRT_HIP(hipGetLastError());
  unsigned long long *hc = (unsigned long long *)(h + L.hostCounts);
  IRT_HIP(hipMemcpyAsync(hc, A.counts, (kMaxT + 1) * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
  IRT_HIP(hipStreamSynchronize(s));  // the counts are the call's answer on the host
  const unsigned long long total = hc[kMaxT];
  if (total >= (unsigned long long)kContourMaxSegments) {
    set_error("%s: %llu segments (fewer than 2^24)", what, total);
    return IRT_E_INVALID;
  }
  *count = (size_t)total;
  if (countPerThreshold)
    for (int t = 0; t < numThresholds; ++t) countPerThreshold[t] = (size_t)hc[t];
  if (!d_out) return IRT_OK;  // size query
  if (capacity < (size_t)total) {
    set_error("%s: capacity %zu < %llu segments", what, capacity, total);
    return IRT_E_INVALID;
  }
  if (total == 0ull) return IRT_OK;
  A.total = total;
  hipLaunchKernelGGL(k_contour_emit, dim3(numWG), dim3(kCtrWG), 0, s, A);
  return sample_end(c, s);
}

int irt_contour_latlon(irt_context *c, int mode, const float *lat, int numLat, const float *lon, int numLon,
                       float radius, const float *threshold, const int32_t *style, int numThresholds, int flags,
                       irt_overlay_segment *d_out, size_t capacity, size_t *count, size_t *countPerThreshold,
                       void *stream) {
  const char *what = "irt_contour_latlon";
  int rc = sample_check(c, mode, what);
  if (rc) return rc;
  if (!count) {
    set_error("%s: null count", what);
    return IRT_E_INVALID;
  }
  // (before anything is sampled: what irt_contour_grid would refuse)
  int cellsLon = 0;
  if ((rc = contour_args(what, lat, numLat, lon, numLon, threshold, style, numThresholds, flags, &cellsLon))) return rc;
  if ((uintptr_t)d_out & 63u) {
    set_error("%s: d_out is not 64-byte aligned", what);
    return IRT_E_INVALID;
  }
  if (!(isfinite(radius) && radius > 0.f)) {
    set_error("%s: radius = %g is not finite and positive", what, (double)radius);
    return IRT_E_INVALID;
  }
  const size_t points = (size_t)numLat * (size_t)numLon;  // < 2^27
  const size_t need = ((points * sizeof(float) + 255) & ~size_t(255)) + points;
  if (need > c->contourGridCap) {
    IRT_HIP(hipSetDevice(c->device));
    IRT_HIP(wait_samples(c));  // an earlier call's kernels may still read the old grid
    if (c->d_contourGrid) {
      IRT_HIP(hipFree(c->d_contourGrid));
      c->d_contourGrid = nullptr;
      c->bytes -= std::min(c->bytes, c->contourGridCap);
    }
    c->contourGridCap = 0;
    c->info.deviceBytes = c->bytes;
    const size_t cap = need + need / 2;
    IRT_HIP(hipMalloc((void **)&c->d_contourGrid, cap));
    c->contourGridCap = cap;
    c->bytes += cap;
    c->info.deviceBytes = c->bytes;
  }
  float *d_value = (float *)c->d_contourGrid;
  uint8_t *d_found = (uint8_t *)c->d_contourGrid + ((points * sizeof(float) + 255) & ~size_t(255));
  if ((rc = irt_sample_latlon(c, mode, lat, numLat, lon, numLon, &radius, 1, d_value, d_found, NAN, stream))) return rc;
  return irt_contour_grid(c, d_value, d_found, lat, numLat, lon, numLon, threshold, style, numThresholds, flags, d_out,
                          capacity, count, countPerThreshold, stream);
}

}  // extern "C"
