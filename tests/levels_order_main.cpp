// A stand-alone check of host/irt_level_order.cpp (the radii check and the slot order of
// irt_render_levels), built by tests/test_levels_cpu.py with -fsanitize=address,undefined and run
// there: every output array is a heap block of exactly numLevels elements, so a write past the
// levels given is the sanitizer's to report.  Exit status 0: every check passed.
#include <math.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "irt_internal.h"

static int g_errors = 0;  // set_error calls seen

namespace irt {
void set_error(const char *fmt, ...) {
  (void)fmt;
  ++g_errors;
}
}  // namespace irt

static int fail(const char *what, int n) {
  fprintf(stderr, "levels_order_main: %s (n = %d)\n", what, n);
  return 1;
}

// near order: a permutation, sorted[h] = radius[index[h]], descending, ties by ascending index
static int check(const std::vector<float> &radius) {
  const int n = (int)radius.size();
  std::vector<float> sorted(n);
  std::vector<int32_t> index(n);
  if (irt_levels_order(radius.data(), n, sorted.data(), index.data()) != IRT_OK) return fail("refused", n);
  std::vector<int> seen(n, 0);
  for (int h = 0; h < n; ++h) {
    if (index[h] < 0 || index[h] >= n || seen[index[h]]++) return fail("not a permutation", n);
    if (sorted[h] != radius[index[h]]) return fail("sorted[h] != radius[index[h]]", n);
    if (h && (sorted[h - 1] < sorted[h] || (sorted[h - 1] == sorted[h] && index[h - 1] > index[h])))
      return fail("out of order", n);
  }
  return 0;
}

int main() {
  uint32_t s = 12345u;
  auto rnd = [&]() {
    s = s * 1664525u + 1013904223u;
    return (float)(s >> 8) * (1.f / 16777216.f);
  };
  for (int n = 1; n <= IRT_MAX_LEVELS; ++n) {
    std::vector<float> up(n), down(n), same(n, 6.4e6f), few(n), any(n);
    for (int k = 0; k < n; ++k) {
      up[k] = 6.3e6f + 1000.f * (float)k;
      down[k] = 6.5e6f - 1000.f * (float)k;
      few[k] = 6.3e6f + 1000.f * (float)(int)(rnd() * 3.f);  // many ties
      any[k] = 1.f + rnd() * 7e6f;
    }
    if (check(up) || check(down) || check(same) || check(few) || check(any)) return 1;
  }
  // the refusals: counts outside [1, IRT_MAX_LEVELS], radii that are not finite and positive, NULLs
  std::vector<float> r(IRT_MAX_LEVELS + 1, 6.4e6f), sorted(IRT_MAX_LEVELS + 1);
  std::vector<int32_t> index(IRT_MAX_LEVELS + 1);
  int refused = 0;
  g_errors = 0;
  refused += irt_levels_order(r.data(), 0, sorted.data(), index.data()) == IRT_E_INVALID;
  refused += irt_levels_order(r.data(), -1, sorted.data(), index.data()) == IRT_E_INVALID;
  refused += irt_levels_order(r.data(), IRT_MAX_LEVELS + 1, sorted.data(), index.data()) == IRT_E_INVALID;
  refused += irt_levels_order(nullptr, 3, sorted.data(), index.data()) == IRT_E_INVALID;
  refused += irt_levels_order(r.data(), 3, nullptr, index.data()) == IRT_E_INVALID;
  refused += irt_levels_order(r.data(), 3, sorted.data(), nullptr) == IRT_E_INVALID;
  const float bad[] = {0.f, -0.f, -6.4e6f, INFINITY, -INFINITY, NAN};
  for (float b : bad) {
    r[2] = b;
    refused += irt_levels_order(r.data(), 4, sorted.data(), index.data()) == IRT_E_INVALID;
  }
  if (refused != 12 || g_errors != 12) return fail("a bad argument was accepted, or refused without a message", refused);
  r[2] = 1e-30f;  // finite and positive: accepted
  if (irt_levels_order(r.data(), 4, sorted.data(), index.data()) != IRT_OK) return fail("a tiny radius refused", 4);
  printf("levels_order_main: ok\n");
  return 0;
}
