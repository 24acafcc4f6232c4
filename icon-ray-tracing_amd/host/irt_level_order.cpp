// irt_level_order.cpp -- the host side of level surfaces (include/icon_rt_hip.h, "level surfaces"): the
// argument check of the radii and the order of the hit slots.  No GPU here; the kernel and the
// context entry point are in csrc/irt_levels.hip.

#include <math.h>

#include "irt_internal.h"

namespace irt {

// the checks of irt_render_levels and irt_levels_order on the radii
int levels_args(const char *what, const float *radius, int numLevels) {
  if (numLevels < 1 || numLevels > IRT_MAX_LEVELS) {
    set_error("%s: %d levels are outside [1, %d]", what, numLevels, IRT_MAX_LEVELS);
    return IRT_E_INVALID;
  }
  if (!radius) {
    set_error("%s: null radius", what);
    return IRT_E_INVALID;
  }
  for (int k = 0; k < numLevels; ++k)
    if (!(isfinite(radius[k]) && radius[k] > 0.f)) {
      set_error("%s: radius[%d] = %g is not finite and positive", what, k, (double)radius[k]);
      return IRT_E_INVALID;
    }
  return IRT_OK;
}

// near[]: the level indices by descending radius, ties by ascending index (an insertion sort that
// never moves an element past an equal one); numLevels in [1, IRT_MAX_LEVELS], checked by the caller
void levels_order(const float *radius, int numLevels, float *sorted, int32_t *index) {
  for (int k = 0; k < numLevels; ++k) {
    int j = k;
    for (; j > 0 && sorted[j - 1] < radius[k]; --j) {
      sorted[j] = sorted[j - 1];
      index[j] = index[j - 1];
    }
    sorted[j] = radius[k];
    index[j] = k;
  }
}

}  // namespace irt

using namespace irt;

extern "C" int irt_levels_order(const float *radius, int numLevels, float *sorted, int32_t *index) {
  int rc = levels_args("irt_levels_order", radius, numLevels);
  if (rc) return rc;
  if (!sorted || !index) {
    set_error("irt_levels_order: null sorted or index");
    return IRT_E_INVALID;
  }
  levels_order(radius, numLevels, sorted, index);
  return IRT_OK;
}
