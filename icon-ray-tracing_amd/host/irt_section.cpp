// irt_section.cpp -- the host side of sections (include/icon_rt_hip.h, "sections"): the argument
// check of irt_section, the columns' trig table from the host's glibc, the points it makes
// (irt_section_points) and the great-circle track between two points (irt_great_circle).  No GPU
// here; the kernel and the context entry point are in csrc/irt_section.hip.

#include <math.h>

#include <algorithm>
#include <thread>

#include "irt_build.h"
#include "irt_internal.h"

namespace irt {

// tab[4 c ..] = {cosf lat[c], sinf lat[c], cosf lon[c], sinf lon[c]}: the four factors of
// toCartesian (ICONGrid.h:44-54), once per column -- the values latlon_trig gives a grid's row and
// column of the same angles.  A long list is split over the host's worker threads: at 2^20 columns
// the four million libm calls are 13 ms on one thread, twice the kernel's time
void section_trig(const float *lat, const float *lon, int numColumns, float *tab) {
  const size_t n = (size_t)numColumns;
  auto part = [=](size_t b, size_t e) {
    for (size_t c = b; c < e; ++c) {
      tab[4 * c] = cosf(lat[c]);
      tab[4 * c + 1] = sinf(lat[c]);
      tab[4 * c + 2] = cosf(lon[c]);
      tab[4 * c + 3] = sinf(lon[c]);
    }
  };
  const size_t threads = n < kSectionTrigSplit ? 1 : (size_t)default_threads();
  if (threads <= 1) return part(0, n);
  std::vector<std::thread> ts;
  const size_t chunk = (n + threads - 1) / threads;
  for (size_t b = 0; b < n; b += chunk) ts.emplace_back(part, b, std::min(n, b + chunk));
  for (auto &t : ts) t.join();
}

// the argument check irt_section and irt_section_points share (latlon_args for one axis of
// pairs; like it, it looks at no angle); *total = the section's points
int section_args(const char *what, const float *lat, const float *lon, int numColumns, const float *radius,
                 int numLevels, size_t *total) {
  if (numColumns < 0 || numLevels < 0) {
    set_error("%s: negative count (%d levels x %d columns)", what, numLevels, numColumns);
    return IRT_E_INVALID;
  }
  // two counts below 2^31: their product fits 64 bits
  const uint64_t points = (uint64_t)numColumns * (uint64_t)numLevels;
  if (points > kSampleMaxPoints) {
    set_error("%s: %d levels x %d columns is more than 2^36 points", what, numLevels, numColumns);
    return IRT_E_INVALID;
  }
  *total = (size_t)points;
  if (points != 0 && (!lat || !lon || !radius)) {
    set_error("%s: null lat, lon or radius", what);
    return IRT_E_INVALID;
  }
  return IRT_OK;
}

}  // namespace irt

using namespace irt;

extern "C" {

int irt_section_points(const float *lat, const float *lon, int numColumns, const float *radius, int numLevels,
                       float *xyz) {
  size_t total = 0;
  int rc = section_args("irt_section_points", lat, lon, numColumns, radius, numLevels, &total);
  if (rc) return rc;
  if (total == 0) return IRT_OK;
  if (!xyz) {
    set_error("irt_section_points: null xyz");
    return IRT_E_INVALID;
  }
  std::vector<float> tab(4 * (size_t)numColumns);
  section_trig(lat, lon, numColumns, tab.data());
  float *out = xyz;
  for (int k = 0; k < numLevels; ++k)
    for (size_t c = 0; c < (size_t)numColumns; ++c, out += 3)
      to_cartesian_trig(radius[k], tab.data() + 4 * c, out[0], out[1], out[2]);
  return IRT_OK;
}

int irt_great_circle(float lat0, float lon0, float lat1, float lon1, int numPoints, float *lat, float *lon,
                     double *arc) {
  const char *what = "irt_great_circle";
  if (numPoints < 1) {
    set_error("%s: %d points (at least 1)", what, numPoints);
    return IRT_E_INVALID;
  }
  if (!(isfinite(lat0) && isfinite(lon0) && isfinite(lat1) && isfinite(lon1))) {
    set_error("%s: an end point (%g, %g) - (%g, %g) is not finite", what, (double)lat0, (double)lon0, (double)lat1,
              (double)lon1);
    return IRT_E_INVALID;
  }
  if (!lat || !lon) {
    set_error("%s: null lat or lon", what);
    return IRT_E_INVALID;
  }
  // the end points' unit vectors, and the angle between them
  const double cl0 = cos((double)lat0), cl1 = cos((double)lat1);
  const double a[3] = {cl0 * cos((double)lon0), cl0 * sin((double)lon0), sin((double)lat0)};
  const double b[3] = {cl1 * cos((double)lon1), cl1 * sin((double)lon1), sin((double)lat1)};
  const double cx = a[1] * b[2] - a[2] * b[1], cy = a[2] * b[0] - a[0] * b[2], cz = a[0] * b[1] - a[1] * b[0];
  const double d = a[0] * b[0] + a[1] * b[1] + a[2] * b[2];
  const double omega = atan2(sqrt(cx * cx + cy * cy + cz * cz), d);
  const double so = sin(omega);
  const bool degenerate = so < 1e-9;
  if (degenerate && d < 0.0) {
    set_error("%s: (%g, %g) and (%g, %g) are antipodal: no unique great circle", what, (double)lat0, (double)lon0,
              (double)lat1, (double)lon1);
    return IRT_E_INVALID;
  }
  if (arc) *arc = omega;
  for (int i = 0; i < numPoints; ++i) {
    if (i == 0 || degenerate) {  // (coincident end points: every point is the start ...
      lat[i] = lat0;
      lon[i] = lon0;
    }
    if (i == numPoints - 1 && i > 0) {  // ... but an end point is always the caller's)
      lat[i] = lat1;
      lon[i] = lon1;
    }
    if (i == 0 || i == numPoints - 1 || degenerate) continue;
    const double t = (double)i / (double)(numPoints - 1);
    const double wa = sin((1.0 - t) * omega) / so, wb = sin(t * omega) / so;
    const double p[3] = {wa * a[0] + wb * b[0], wa * a[1] + wb * b[1], wa * a[2] + wb * b[2]};
    const double len = sqrt(p[0] * p[0] + p[1] * p[1] + p[2] * p[2]);
    const double s = p[2] / len;
    lat[i] = (float)asin(s < -1.0 ? -1.0 : (s > 1.0 ? 1.0 : s));
    lon[i] = (float)atan2(p[1], p[0]);
  }
  return IRT_OK;
}

}  // extern "C"
