// irt_histogram.cpp -- the host side of the field's histogram (include/icon_rt_hip.h, "field
// statistics"): the argument check irt_histogram and irt_histogram_cells share, and the histogram of
// a record array on the host (irt_histogram_cells, the definition the kernel is held to).  No GPU
// here; the kernel and the context entry point are in csrc/irt_histogram.hip.

#include <math.h>

#include <vector>

#include "irt_histogram.h"
#include "irt_internal.h"

namespace irt {

int hist_args(const char *what, irt_box1f valueRange, int numBins, int weighting, const float *bandEdges,
              int numBands) {
  if (numBins < 1 || numBins > kHistMaxBins) {
    set_error("%s: %d bins are outside [1, %d]", what, numBins, kHistMaxBins);
    return IRT_E_INVALID;
  }
  if (numBands < 1 || numBands > kHistMaxBands) {
    set_error("%s: %d bands are outside [1, %d]", what, numBands, kHistMaxBands);
    return IRT_E_INVALID;
  }
  if (numBins * numBands > kHistMaxBins) {
    set_error("%s: %d bins x %d bands are more than %d counters", what, numBins, numBands, kHistMaxBins);
    return IRT_E_INVALID;
  }
  if (!(isfinite(valueRange.lower) && isfinite(valueRange.upper) && valueRange.upper > valueRange.lower)) {
    set_error("%s: valueRange [%g, %g] is not finite with upper > lower", what, (double)valueRange.lower,
              (double)valueRange.upper);
    return IRT_E_INVALID;
  }
  if (weighting != IRT_HIST_COUNT && weighting != IRT_HIST_THICKNESS) {
    set_error("%s: weighting %d is neither IRT_HIST_COUNT nor IRT_HIST_THICKNESS", what, weighting);
    return IRT_E_INVALID;
  }
  if (!bandEdges) {
    if (numBands != 1) {
      set_error("%s: null bandEdges with %d bands (one band without edges)", what, numBands);
      return IRT_E_INVALID;
    }
    return IRT_OK;
  }
  for (int b = 0; b <= numBands; ++b)
    if (!isfinite(bandEdges[b]) || (b > 0 && !(bandEdges[b] > bandEdges[b - 1]))) {
      set_error("%s: bandEdges[%d] = %g is not finite and above bandEdges[%d]", what, b, (double)bandEdges[b],
                b > 0 ? b - 1 : 0);
      return IRT_E_INVALID;
    }
  return IRT_OK;
}

}  // namespace irt

using namespace irt;

extern "C" int irt_histogram_cells(const irt_icon_cell *cells, size_t n, irt_box1f valueRange, int numBins,
                                   int weighting, const float *bandEdges, int numBands, irt_histogram_out out) {
  const char *what = "irt_histogram_cells";
  const int rc = hist_args(what, valueRange, numBins, weighting, bandEdges, numBands);
  if (rc) return rc;
  if (n && !cells) {
    set_error("%s: null cells", what);
    return IRT_E_INVALID;
  }
  for (size_t i = 0; i < n; ++i)
    if (cells[i].numLayers < 0 || cells[i].numLayers > 31) {
      set_error("cell %zu: numLayers %d outside [0,31] (MAX_LAYERS 32, ICONGrid.h:57)", i, cells[i].numLayers);
      return IRT_E_DATA;
    }
  const HistSpec S = {valueRange.lower, valueRange.upper, numBins, numBands, weighting, bandEdges ? 1 : 0};
  std::vector<uint64_t> acc((size_t)hist_slots(S), 0u);
  for (size_t i = 0; i < n; ++i) {
    const irt_icon_cell &c = cells[i];
    for (int l = 0; l < c.numLayers; ++l) {
      uint64_t w;
      const int slot = hist_item(S, bandEdges, c.value[l], c.height[l], c.height[l + 1], w);
      if (slot >= 0) acc[(size_t)slot] += w;
    }
  }
  const uint64_t *a = acc.data();
  if (out.bins)
    for (int k = 0; k < numBands * numBins; ++k) out.bins[k] = a[k];
  if (out.tails)
    for (int k = 0; k < 3 * numBands; ++k) out.tails[k] = a[hist_tail_base(S) + k];
  if (out.outside) out.outside[0] = a[hist_outside_slot(S)];
  return IRT_OK;
}
