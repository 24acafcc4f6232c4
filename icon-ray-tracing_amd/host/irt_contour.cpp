// irt_contour.cpp -- the host side of the isolines (include/icon_rt_hip.h, "isolines"): the argument
// check and the trig tables the device call shares, and irt_contour_cells, the definition
// (csrc/irt_contour.h) applied cell by cell in output order -- what the kernels of
// csrc/irt_contour.hip are held to, bit for bit.  No GPU here.

#include <math.h>
#include <string.h>

#include <vector>

#include "irt_contour.h"
#include "irt_internal.h"

namespace irt {

int contour_args(const char *what, const float *lat, int numLat, const float *lon, int numLon, const float *threshold,
                 const int32_t *style, int numThresholds, int flags, int *cellsLon) {
  if (flags & ~IRT_CONTOUR_WRAP) {
    set_error("%s: unknown flag bits 0x%x", what, (unsigned)(flags & ~IRT_CONTOUR_WRAP));
    return IRT_E_INVALID;
  }
  if (numLat < 2 || numLon < 2 || (uint64_t)numLat * (uint64_t)numLon >= kContourMaxPoints) {
    set_error("%s: a grid of %d x %d points (at least 2 x 2, fewer than 2^27 points)", what, numLat, numLon);
    return IRT_E_INVALID;
  }
  if (numThresholds < 1 || numThresholds > IRT_CONTOUR_MAX_THRESHOLDS) {
    set_error("%s: %d thresholds are outside [1, %d]", what, numThresholds, IRT_CONTOUR_MAX_THRESHOLDS);
    return IRT_E_INVALID;
  }
  if (!lat || !lon || !threshold || !style) {
    set_error("%s: null lat, lon, threshold or style", what);
    return IRT_E_INVALID;
  }
  for (int k = 0; k < 2; ++k) {
    const float *x = k ? lon : lat;
    const int n = k ? numLon : numLat;
    for (int i = 0; i < n; ++i)
      if (!isfinite(x[i])) {
        set_error("%s: %s[%d] is not finite", what, k ? "lon" : "lat", i);
        return IRT_E_INVALID;
      }
    for (int i = 0; i + 1 < n; ++i)
      if (!(x[i + 1] > x[i] && x[i + 1] - x[i] <= kContourMaxStep)) {
        set_error("%s: %s[%d] = %g, %s[%d] = %g: steps must ascend by at most %g rad", what, k ? "lon" : "lat", i,
                  (double)x[i], k ? "lon" : "lat", i + 1, (double)x[i + 1], (double)kContourMaxStep);
        return IRT_E_INVALID;
      }
  }
  if (flags & IRT_CONTOUR_WRAP) {
    const double span = (double)lon[numLon - 1] - (double)lon[0], twoPi = 2.0 * M_PI;
    if (!(span < twoPi && twoPi - span <= (double)kContourMaxStep)) {
      set_error("%s: IRT_CONTOUR_WRAP: lon spans %.9g rad; the closing step must be in (0, %g] rad", what, span,
                (double)kContourMaxStep);
      return IRT_E_INVALID;
    }
  }
  for (int t = 0; t < numThresholds; ++t) {
    if (!isfinite(threshold[t])) {
      set_error("%s: threshold[%d] is not finite", what, t);
      return IRT_E_INVALID;
    }
    if (style[t] < 0 || style[t] >= IRT_OVERLAY_MAX_STYLES) {
      set_error("%s: style[%d] = %d is outside [0, %d)", what, t, style[t], IRT_OVERLAY_MAX_STYLES);
      return IRT_E_INVALID;
    }
  }
  *cellsLon = (flags & IRT_CONTOUR_WRAP) ? numLon : numLon - 1;
  return IRT_OK;
}

void contour_trig(const float *lat, int numLat, const float *lon, int numLon, double *latC, double *latS,
                  double *lonC, double *lonS) {
  for (int j = 0; j < numLat; ++j) {
    latC[j] = cos((double)lat[j]);
    latS[j] = sin((double)lat[j]);
  }
  for (int i = 0; i < numLon; ++i) {
    lonC[i] = cos((double)lon[i]);
    lonS[i] = sin((double)lon[i]);
  }
}

}  // namespace irt

using namespace irt;

extern "C" {

int irt_contour_cells(const float *value, const uint8_t *found, const float *lat, int numLat, const float *lon,
                      int numLon, const float *threshold, const int32_t *style, int numThresholds, int flags,
                      irt_overlay_segment *out, size_t capacity, size_t *count, size_t *countPerThreshold) {
  const char *what = "irt_contour_cells";
  if (!count) {
    set_error("%s: null count", what);
    return IRT_E_INVALID;
  }
  int cellsLon = 0;
  const int rc = contour_args(what, lat, numLat, lon, numLon, threshold, style, numThresholds, flags, &cellsLon);
  if (rc) return rc;
  if (!value) {
    set_error("%s: null value", what);
    return IRT_E_INVALID;
  }
  std::vector<double> tab(2 * ((size_t)numLat + (size_t)numLon));
  double *latC = tab.data(), *latS = latC + numLat, *lonC = latS + numLat, *lonS = lonC + numLon;
  contour_trig(lat, numLat, lon, numLon, latC, latS, lonC, lonS);
  const int cellsLat = numLat - 1;
  // pass 0 counts (and refuses before anything is written), pass 1 fills
  irt_overlay_segment s0, s1;
  size_t per[IRT_CONTOUR_MAX_THRESHOLDS] = {};
  for (int pass = 0; pass < (out ? 2 : 1); ++pass) {
    size_t k = 0;
    for (int t = 0; t < numThresholds; ++t) {
      const size_t start = k;
      for (int j = 0; j < cellsLat; ++j)
        for (int i = 0; i < cellsLon; ++i) {
          ContourCell K;
          if (!ctr_load(value, found, latC, latS, lonC, lonS, numLon, j, i, i + 1 == numLon ? 0 : i + 1, K)) continue;
          if (pass == 0) {
            const uint32_t kept = ctr_eval<false>(K, threshold[t], style[t], s0, s1);
            k += (kept & 1u) + (kept >> 1);
          } else {
            const uint32_t kept = ctr_eval<true>(K, threshold[t], style[t], s0, s1);
            if (kept & 1u) out[k++] = s0;
            if (kept & 2u) out[k++] = s1;
          }
        }
      per[t] = k - start;
    }
    if (pass == 0) {
      if (k >= kContourMaxSegments) {
        set_error("%s: %zu segments (fewer than 2^24)", what, k);
        return IRT_E_INVALID;
      }
      *count = k;
      if (countPerThreshold) memcpy(countPerThreshold, per, (size_t)numThresholds * sizeof(size_t));
      if (out && capacity < k) {
        set_error("%s: capacity %zu < %zu segments", what, capacity, k);
        return IRT_E_INVALID;
      }
    }
  }
  return IRT_OK;
}

}  // extern "C"
