// irt_column.h -- the column reduction (include/icon_rt_hip.h, "column products"), defined once:
// the running values of one column and the step a found level takes.  The host helper
// (host/irt_column.cpp irt_column_reduce) and the kernels (csrc/irt_column.hip) compile this text,
// so the one-pass kernels and the two-pass path reduce with the same operations in the same order.
#pragma once

#include <stdint.h>

#include "irt_common.h"

namespace irt {

// One column's running reduction: six values, in registers on the device
struct ColumnAcc {
  float wsum, mx, mn;
  int32_t kmax, kmin, count;
};

IRT_HD void column_init(ColumnAcc &a) {
  a.wsum = a.mx = a.mn = 0.f;
  a.kmax = a.kmin = -1;
  a.count = 0;
}

// Level k was found with value v; w = its weight (1.0f where the caller gave none: 1.0f * v is v).
// Levels come in ascending k.  Strict comparisons: a tie keeps the lower k, a NaN never replaces a
// value.  One multiply, then one add (the build is -ffp-contract=off: no fma).
IRT_HD void column_step(ColumnAcc &a, int32_t k, float w, float v) {
  const float wv = w * v;
  if (a.count == 0) {
    a.mn = a.mx = v;
    a.kmin = a.kmax = k;
    a.wsum = wv;
  } else {
    if (v < a.mn) {
      a.mn = v;
      a.kmin = k;
    }
    if (v > a.mx) {
      a.mx = v;
      a.kmax = k;
    }
    a.wsum = a.wsum + wv;
  }
  ++a.count;
}

// After the last level: a column without a found level holds missValue (kmax = kmin = -1 already)
IRT_HD void column_finish(ColumnAcc &a, float missValue) {
  if (a.count == 0) a.wsum = a.mx = a.mn = missValue;
}

// The product irt_render_column shows (IRT_COLUMN_WSUM / _MAX / _MIN) of a finished column
IRT_HD float column_product(const ColumnAcc &a, int product) {
  return product == 1 ? a.mx : (product == 2 ? a.mn : a.wsum);
}

}  // namespace irt
