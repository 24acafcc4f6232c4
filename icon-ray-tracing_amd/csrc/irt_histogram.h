// irt_histogram.h -- the histogram of the field by value and altitude band (include/icon_rt_hip.h,
// "field statistics"), defined once: the weight, the band and the bin of one (record, layer) item.
// The host helper (host/irt_histogram.cpp irt_histogram_cells) and the kernel (csrc/irt_histogram.hip)
// compile this text.  Everything is float (-ffp-contract=off, correctly rounded division) and every
// accumulator an unsigned 64-bit integer, so the result does not depend on the order of the
// additions: "equal" means equal integers.
//
// The items are every (record i, layer l) with 0 <= l < numLayers[i]; v = value[l], h0 = height[l],
// h1 = height[l + 1].  ICON cells have nearly equal area, so with IRT_HIST_THICKNESS a layer's
// thickness stands in for its volume: the unit of the weight is 1/64 m, and heights near 6.4e6 m
// are multiples of 0.5 m, so nothing is lost.
//
// With numBins == tf.size the bin k of a value is the LUT index clamp(idx, 0, size - 1) of
// postClassify (deviceCode.cu:129-132): t is its normalised value, k = min(int(t * size), size - 1),
// so the bins line up with the LUT entries (the tails hold what postClassify clamps from outside).
#pragma once

#include <stdint.h>

#include "irt_common.h"

namespace irt {

constexpr int kHistMaxBins = 4096;   // numBins, and numBins * numBands: 32 KB of 64-bit counters
constexpr int kHistMaxBands = 64;
constexpr float kHistMaxThickness = 1048576.0f;  // a thicker layer weighs nothing

struct HistSpec {
  float lower, upper;  // valueRange
  int numBins, numBands;
  int weighting;       // IRT_HIST_COUNT (0) / IRT_HIST_THICKNESS (1)
  int banded;          // bandEdges given (else one band that holds every item)
};

// The accumulators as one array: bins[numBands * numBins], tails[numBands * 3], outside[1]
IRT_HD int hist_tail_base(const HistSpec &S) { return S.numBands * S.numBins; }
IRT_HD int hist_outside_slot(const HistSpec &S) { return S.numBands * S.numBins + 3 * S.numBands; }
IRT_HD int hist_slots(const HistSpec &S) { return hist_outside_slot(S) + 1; }

// The weight of a layer.  Thickness: (uint64_t)(d * 64.0f), truncating, for 0 < d <= 2^20 m -- at
// most 2^26, so the conversion through 32 bits is the same integer; an inverted first layer of a
// convert_icon land column, a zero-thickness record and a non-finite d weigh nothing.
IRT_HD uint64_t hist_weight(int weighting, float h0, float h1) {
  if (weighting == 0) return 1u;
  const float d = h1 - h0;
  if (!(d > 0.f && d <= kHistMaxThickness)) return 0u;
  return (uint64_t)(uint32_t)(d * 64.0f);
}

// The band of mid-height m: b with edges[b] <= m && m < edges[b + 1].  The edges ascend strictly, so
// that is (the number of edges <= m) - 1 wherever it lies in [0, numBands); -1 (m below edges[0], or
// NaN) and numBands (m at or above the last edge) are "in no band".
IRT_HD int hist_band(const float *edges, int numBands, float m) {
  int first = 0, count = numBands + 1;
  while (count > 0) {
    const int step = count / 2;
    if (edges[first + step] <= m) {
      first += step + 1;
      count -= step + 1;
    } else {
      count = step;
    }
  }
  return first - 1;
}

// The accumulator slot of a value in band b: its bin, or one of the band's three tails
IRT_HD int hist_value_slot(const HistSpec &S, int b, float v) {
  const float t = (v - S.lower) / (S.upper - S.lower);  // postClassify's normalisation
  const bool finite = (f2u(v) & 0x7f800000u) != 0x7f800000u;
  const int tail = hist_tail_base(S) + 3 * b;
  if (!finite || t != t) return tail + 2;
  if (t < 0.f) return tail;
  if (t > 1.f) return tail + 1;
  const int k = (int)(t * (float)S.numBins);  // t in [0, 1]: at most 4096
  return b * S.numBins + (k < S.numBins - 1 ? k : S.numBins - 1);
}

// One item: its weight in w and the slot it is added to; -1 when w == 0 (the item is dropped)
IRT_HD int hist_item(const HistSpec &S, const float *edges, float v, float h0, float h1, uint64_t &w) {
  w = hist_weight(S.weighting, h0, h1);
  if (w == 0u) return -1;
  int b = 0;
  if (S.banded) {
    b = hist_band(edges, S.numBands, (h0 + h1) * 0.5f);
    if (b < 0 || b >= S.numBands) return hist_outside_slot(S);
  }
  return hist_value_slot(S, b, v);
}

}  // namespace irt
