// irt_column.cpp -- the host side of column products (include/icon_rt_hip.h, "column products"):
// the reduction of a column's levels on the host (irt_column_reduce, the definition the kernels are
// held to) and the argument checks of the column calls.  No GPU here; the kernels and the context
// entry points are in csrc/irt_column.hip.

#include <math.h>

#include "irt_column.h"
#include "irt_internal.h"

namespace irt {

// the weights of a column call: NULL (every weight 1.0f), or numLevels finite floats
int column_weights(const char *what, const float *weight, int numLevels) {
  if (!weight) return IRT_OK;
  for (int k = 0; k < numLevels; ++k)
    if (!isfinite(weight[k])) {
      set_error("%s: weight[%d] = %g is not finite", what, k, (double)weight[k]);
      return IRT_E_INVALID;
    }
  return IRT_OK;
}

// irt_render_column's levels: at least one, every radius finite and positive (as levels_args, without
// its IRT_MAX_LEVELS: the radii travel in the device table, not by value), the weights finite
int column_levels_args(const char *what, const float *radius, const float *weight, int numLevels) {
  if (numLevels < 1) {
    set_error("%s: %d levels (at least 1)", what, numLevels);
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
  return column_weights(what, weight, numLevels);
}

}  // namespace irt

using namespace irt;

extern "C" int irt_column_reduce(const float *value, const uint8_t *found, int numLevels, size_t numColumns,
                                 const float *weight, float missValue, irt_column_out out) {
  if (numLevels < 1) {
    set_error("irt_column_reduce: %d levels (at least 1)", numLevels);
    return IRT_E_INVALID;
  }
  if (numColumns && (!value || !found)) {
    set_error("irt_column_reduce: null value or found");
    return IRT_E_INVALID;
  }
  for (size_t c = 0; c < numColumns; ++c) {
    ColumnAcc a;
    column_init(a);
    for (int k = 0; k < numLevels; ++k) {
      const size_t p = (size_t)k * numColumns + c;
      if (found[p]) column_step(a, k, weight ? weight[k] : 1.f, value[p]);
    }
    column_finish(a, missValue);
    if (out.wsum) out.wsum[c] = a.wsum;
    if (out.vmax) out.vmax[c] = a.mx;
    if (out.vmin) out.vmin[c] = a.mn;
    if (out.kmax) out.kmax[c] = a.kmax;
    if (out.kmin) out.kmin[c] = a.kmin;
    if (out.count) out.count[c] = a.count;
  }
  return IRT_OK;
}
