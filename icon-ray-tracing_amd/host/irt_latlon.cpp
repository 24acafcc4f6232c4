// irt_latlon.cpp -- the host side of resampling (include/icon_rt_hip.h, "resampling"): the
// lat/lon grid's trig rows from the host's glibc, the points they make, and the host compilation
// of the guard the sampling kernels apply (irt_common.h sample_admits).  No GPU here; the kernels
// and the context entry points are in csrc/irt_sample.hip.

#include <math.h>

#include "icon_rt_hip_debug.h"
#include "irt_build.h"
#include "irt_internal.h"

namespace irt {

// latCS[2 j] = cosf(lat[j]), latCS[2 j + 1] = sinf(lat[j]); lonCS likewise: the four factors of
// toCartesian (ICONGrid.h:44-54), once per row and per column
void latlon_trig(const float *lat, int numLat, const float *lon, int numLon, float *latCS, float *lonCS) {
  for (size_t j = 0; j < (size_t)numLat; ++j) {
    latCS[2 * j] = cosf(lat[j]);
    latCS[2 * j + 1] = sinf(lat[j]);
  }
  for (size_t i = 0; i < (size_t)numLon; ++i) {
    lonCS[2 * i] = cosf(lon[i]);
    lonCS[2 * i + 1] = sinf(lon[i]);
  }
}

// the argument check irt_sample_latlon and irt_latlon_points share; *total = the grid's points
int latlon_args(const char *what, const float *lat, int numLat, const float *lon, int numLon,
                const float *radius, int numLevels, size_t *total) {
  if (numLat < 0 || numLon < 0 || numLevels < 0) {
    set_error("%s: negative count (%d levels x %d lat x %d lon)", what, numLevels, numLat, numLon);
    return IRT_E_INVALID;
  }
  // three counts below 2^31: the product of the first two fits 64 bits, the third is compared
  // by division
  const uint64_t plane = (uint64_t)numLat * (uint64_t)numLon;
  if (plane != 0 && (uint64_t)numLevels > kSampleMaxPoints / plane) {
    set_error("%s: %d levels x %d lat x %d lon is more than 2^36 points", what, numLevels, numLat, numLon);
    return IRT_E_INVALID;
  }
  *total = (size_t)(plane * (uint64_t)numLevels);
  if (*total != 0 && (!lat || !lon || !radius)) {
    set_error("%s: null lat, lon or radius", what);
    return IRT_E_INVALID;
  }
  return IRT_OK;
}

}  // namespace irt

using namespace irt;

extern "C" {

int irt_latlon_points(const float *lat, int numLat, const float *lon, int numLon, const float *radius,
                      int numLevels, float *xyz) {
  size_t total = 0;
  int rc = latlon_args("irt_latlon_points", lat, numLat, lon, numLon, radius, numLevels, &total);
  if (rc) return rc;
  if (total == 0) return IRT_OK;
  if (!xyz) {
    set_error("irt_latlon_points: null xyz");
    return IRT_E_INVALID;
  }
  std::vector<float> latCS(2 * (size_t)numLat), lonCS(2 * (size_t)numLon);
  latlon_trig(lat, numLat, lon, numLon, latCS.data(), lonCS.data());
  float *out = xyz;
  for (int k = 0; k < numLevels; ++k)
    for (int j = 0; j < numLat; ++j)
      for (int i = 0; i < numLon; ++i, out += 3) {
        const float t[4] = {latCS[2 * (size_t)j], latCS[2 * (size_t)j + 1], lonCS[2 * (size_t)i],
                            lonCS[2 * (size_t)i + 1]};
        to_cartesian_trig(radius[k], t, out[0], out[1], out[2]);
      }
  return IRT_OK;
}

int irt_debug_sample_admits(float x, float y, float z) { return sample_admits(x, y, z) ? 1 : 0; }

}  // extern "C"
