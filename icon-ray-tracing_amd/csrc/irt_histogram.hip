// irt_histogram.hip -- the histogram of the field by value and altitude band (include/icon_rt_hip.h,
// "field statistics"; the definition is irt_histogram.h): one pass over the per-record height/value
// blocks and the meta words (numLayers), the only copy of the values a context keeps.  The host side
// (the argument check, irt_histogram_cells) is host/irt_histogram.cpp.
//
// The stream: 16 lanes per record, lane q loading float4 q of the record's 256-B block -- a wave's
// load is four consecutive records, 1 KiB contiguous -- and only the 64-B blocks numLayers reaches.
// In block b (lanes 4b .. 4b+3; irt_common.h kBlk4) lanes 0 and 1 hold height[8b .. 8b+7], lanes 2 and
// 3 value[8b-1 .. 8b+6].  A layer needs its value and two heights, which sit at most five lanes
// apart in the record's DPP row: six row shifts hand every lane two consecutive layers, so all 64
// lanes bin.  The accumulators are a private copy per workgroup in LDS (64-bit adds), flushed once
// at the end, the non-zero entries only, with 64-bit global integer atomics.

#include <hip/hip_runtime.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>

#include "irt_context.h"
#include "irt_histogram.h"

namespace irt {
namespace {

constexpr int kHistThreads = 256;
constexpr int kHistUnroll = 4;  // records per 16-lane group and pass: 4 KiB in flight per wave

struct HistArgs {
  const float4 *blocks;
  const uint32_t *meta;
  unsigned long long n;                        // records
  unsigned long long *bins, *tails, *outside;  // each may be null
  HistSpec S;
  float edges[kHistMaxBands + 1];
};

template <int CTRL>
__device__ __forceinline__ float row_shift(float v) {  // 0x11n: row_shr:n, 0x10n: row_shl:n; 0 past the row's end
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, false));
}

// MERGE: a lane adds a run of items that fall into the same accumulator as one LDS add -- its two
// layers, and the same two layers of the records it takes next; the run ends with the kernel.  Measured
// at C3 it is no faster than one LDS add per item with 300 bins (0-3 % slower) and 5 % slower with 64
// bands, on the smooth field and on noise alike: the product runs MERGE =
// false, IRT_HIST_MERGE=1 selects the other for measurement.
template <bool MERGE>
__global__ void __launch_bounds__(kHistThreads) k_histogram(HistArgs A) {
  extern __shared__ unsigned long long s_acc[];  // hist_slots(A.S) accumulators
  __shared__ float s_edges[kHistMaxBands + 1];
  const int slots = hist_slots(A.S);
  for (int k = threadIdx.x; k < slots; k += kHistThreads) s_acc[k] = 0ull;
  if (A.S.banded && (int)threadIdx.x <= A.S.numBands) s_edges[threadIdx.x] = A.edges[threadIdx.x];
  __syncthreads();

  const int q = (int)(threadIdx.x & 15u);  // float4 q of the record's block
  const bool valueLane = (q & 2) != 0;
  // the lane's two layers l0, l0 + 1: of the four values {value[c0 .. c0+3]} of its pair's value lane
  // (c0 = 8b - 1 or 8b + 3) the value lane takes the first two, the height lane two to its left the others
  const int l0 = 8 * (q >> 2) + ((q & 1) ? 3 : -1) + (valueLane ? 0 : 2);
  const unsigned long long groups = (unsigned long long)gridDim.x * (kHistThreads / 16);
  const unsigned long long g = (unsigned long long)blockIdx.x * (kHistThreads / 16) + (threadIdx.x >> 4);

  int run = -1;  // the accumulator of the lane's current run, and its sum
  unsigned long long sum = 0ull;
  auto add = [&](int slot, unsigned long long w) {
    if (slot < 0) return;
    if (!MERGE) {
      atomicAdd(&s_acc[slot], w);
    } else if (slot == run) {
      sum += w;
    } else {
      if (run >= 0) atomicAdd(&s_acc[run], sum);
      run = slot;
      sum = w;
    }
  };

  int nlNext[kHistUnroll];
#pragma unroll
  for (int u = 0; u < kHistUnroll; ++u) {
    const unsigned long long r = (unsigned long long)u * groups + g;
    nlNext[u] = r < A.n ? (int)(A.meta[r] & 31u) : 0;
  }
  for (unsigned long long base = 0; base < A.n; base += groups * kHistUnroll) {
    int nl[kHistUnroll];
    float4 x[kHistUnroll];
#pragma unroll
    for (int u = 0; u < kHistUnroll; ++u) {
      const unsigned long long r = base + (unsigned long long)u * groups + g;
      nl[u] = nlNext[u];
      x[u] = make_float4(0.f, 0.f, 0.f, 0.f);
      // nl > 0 only for r < n; block b holds a layer below nl, or height[nl], iff b <= nl / 8
      if (nl[u] > 0 && (q >> 2) <= (nl[u] >> 3)) x[u] = A.blocks[r * (unsigned long long)kBlk4 + (unsigned)q];
    }
#pragma unroll
    for (int u = 0; u < kHistUnroll; ++u) {  // the next pass's meta words, behind this pass's blocks
      const unsigned long long r = base + groups * kHistUnroll + (unsigned long long)u * groups + g;
      nlNext[u] = r < A.n ? (int)(A.meta[r] & 31u) : 0;
    }
#pragma unroll
    for (int u = 0; u < kHistUnroll; ++u) {
      // a value lane with {value[c0 .. c0+3]}: height[c0+1 .. c0+4] is two lanes down, height[c0] the .w
      // of the height lane before that one -- three lanes down for lane 3 of a block, five for lane 2
      // (the previous block's lane 1); the height lane two down has height[c0+1 .. c0+4] itself and
      // takes value[c0+2], value[c0+3] from two lanes up.  Every lane of the row runs the shifts (no
      // branch around them).
      const float hA3 = row_shift<0x113>(x[u].w), hA5 = row_shift<0x115>(x[u].w);
      const float hA = (q & 1) ? hA3 : hA5, hB = row_shift<0x112>(x[u].x), hC = row_shift<0x112>(x[u].y);
      const float vZ = row_shift<0x102>(x[u].z), vW = row_shift<0x102>(x[u].w);
      const float v0 = valueLane ? x[u].x : vZ, v1 = valueLane ? x[u].y : vW;
      const float h0 = valueLane ? hA : x[u].y, h1 = valueLane ? hB : x[u].z, h2 = valueLane ? hC : x[u].w;
      uint64_t w;
      if (l0 >= 0 && l0 < nl[u]) {
        const int slot = hist_item(A.S, s_edges, v0, h0, h1, w);
        add(slot, w);
      }
      if (l0 + 1 < nl[u]) {
        const int slot = hist_item(A.S, s_edges, v1, h1, h2, w);
        add(slot, w);
      }
    }
  }
  if (MERGE && run >= 0) atomicAdd(&s_acc[run], sum);
  __syncthreads();
  const int tailBase = hist_tail_base(A.S), outSlot = hist_outside_slot(A.S);
  for (int k = threadIdx.x; k < slots; k += kHistThreads) {
    const unsigned long long v = s_acc[k];
    if (v == 0ull) continue;
    unsigned long long *dst = k < tailBase ? (A.bins ? A.bins + k : nullptr)
                              : k < outSlot ? (A.tails ? A.tails + (k - tailBase) : nullptr)
                                            : A.outside;
    if (dst) atomicAdd(dst, v);
  }
}

}  // namespace
}  // namespace irt

using namespace irt;

extern "C" int irt_histogram(irt_context *c, irt_box1f valueRange, int numBins, int weighting,
                             const float *bandEdges, int numBands, irt_histogram_out d_out, void *stream) {
  const char *what = "irt_histogram";
  int rc = sample_check(c, IRT_MODE_USER_GEOM, what);  // (no sampler is used: the cell mode asks for nothing)
  if (rc) return rc;
  if ((rc = hist_args(what, valueRange, numBins, weighting, bandEdges, numBands))) return rc;
  if (!d_out.bins && !d_out.tails && !d_out.outside) return IRT_OK;
  hipStream_t s = (hipStream_t)stream;
  if ((rc = sample_begin(c, s))) return rc;
  HistArgs A;
  memset(&A, 0, sizeof(A));
  A.blocks = c->d_blocks;
  A.meta = c->d_meta;
  A.n = c->n;
  A.bins = reinterpret_cast<unsigned long long *>(d_out.bins);
  A.tails = reinterpret_cast<unsigned long long *>(d_out.tails);
  A.outside = reinterpret_cast<unsigned long long *>(d_out.outside);
  A.S = {valueRange.lower, valueRange.upper, numBins, numBands, weighting, bandEdges ? 1 : 0};
  if (bandEdges) memcpy(A.edges, bandEdges, (size_t)(numBands + 1) * sizeof(float));
  // the call overwrites: zeroes on the stream, then the workgroups' adds
  if (A.bins) IRT_HIP(hipMemsetAsync(A.bins, 0, (size_t)numBands * numBins * sizeof(uint64_t), s));
  if (A.tails) IRT_HIP(hipMemsetAsync(A.tails, 0, (size_t)numBands * 3 * sizeof(uint64_t), s));
  if (A.outside) IRT_HIP(hipMemsetAsync(A.outside, 0, sizeof(uint64_t), s));
  if (A.n) {
    // IRT_HIST_MERGE=1: the kernel with the in-lane merge (measurement only, profiles/hist_rate.py)
    const char *e = getenv("IRT_HIST_MERGE");
    auto kernel = e && atoi(e) == 1 ? k_histogram<true> : k_histogram<false>;
    const size_t lds = (size_t)hist_slots(A.S) * sizeof(unsigned long long);
    // the grid: every workgroup the device holds at once, each taking 16 x kHistUnroll records per
    // pass; fewer for a small scene.  IRT_HIST_WGS caps it (tests: more than one pass on a small scene)
    int perCU = 0;
    IRT_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&perCU, kernel, kHistThreads, lds));
    const unsigned long long perPass = (kHistThreads / 16) * kHistUnroll;
    unsigned long long wgs = std::min<unsigned long long>(
        (A.n + perPass - 1) / perPass, (unsigned long long)std::max(perCU, 1) * (unsigned)std::max(c->numCU, 1));
    if ((e = getenv("IRT_HIST_WGS")) && atoll(e) > 0) wgs = std::min<unsigned long long>(wgs, (unsigned long long)atoll(e));
    hipLaunchKernelGGL(kernel, dim3((unsigned)wgs), dim3(kHistThreads), lds, s, A);
  }
  return sample_end(c, s);
}
