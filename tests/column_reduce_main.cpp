// A stand-alone check of host/irt_column.cpp (irt_column_reduce, the column reduction's definition
// on the host), built by tests/test_column_cpu.py with -fsanitize=address,undefined and run there:
// every input and output array is a heap block of exactly the size the call may touch, so a read or
// write past it is the sanitizer's to report.  Exit status 0: every check passed.
#include <math.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

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
  fprintf(stderr, "column_reduce_main: %s (n = %d)\n", what, n);
  return 1;
}

struct Out {
  std::vector<float> wsum, vmax, vmin;
  std::vector<int32_t> kmax, kmin, count;
  explicit Out(size_t n) : wsum(n), vmax(n), vmin(n), kmax(n), kmin(n), count(n) {}
  irt_column_out all() { return {wsum.data(), vmax.data(), vmin.data(), kmax.data(), kmin.data(), count.data()}; }
};

// the definition once more, column by column, with the sum in its own loop
static int check(int levels, size_t cols, const std::vector<float> &v, const std::vector<uint8_t> &f,
                 const float *w, float miss) {
  Out o(cols);
  if (irt_column_reduce(v.data(), f.data(), levels, cols, w, miss, o.all()) != IRT_OK) return fail("refused", levels);
  for (size_t c = 0; c < cols; ++c) {
    int kmax = -1, kmin = -1, count = 0;
    float sum = miss;
    for (int k = 0; k < levels; ++k) {
      const size_t p = (size_t)k * cols + c;
      if (!f[p]) continue;
      const float wv = (w ? w[k] : 1.f) * v[p];
      sum = count ? sum + wv : wv;
      if (kmax < 0 || v[p] > v[(size_t)kmax * cols + c]) kmax = k;
      if (kmin < 0 || v[p] < v[(size_t)kmin * cols + c]) kmin = k;
      ++count;
    }
    const float mx = count ? v[(size_t)kmax * cols + c] : miss, mn = count ? v[(size_t)kmin * cols + c] : miss;
    if (o.count[c] != count || o.kmax[c] != kmax || o.kmin[c] != kmin) return fail("count, kmax or kmin", levels);
    if (memcmp(&o.wsum[c], &sum, 4) || memcmp(&o.vmax[c], &mx, 4) || memcmp(&o.vmin[c], &mn, 4))
      return fail("wsum, vmax or vmin", levels);
  }
  // each output alone (the others NULL) is the same output
  Out one(cols);
  irt_column_out only = {nullptr, nullptr, nullptr, nullptr, one.kmin.data(), nullptr};
  if (irt_column_reduce(v.data(), f.data(), levels, cols, w, miss, only) != IRT_OK || one.kmin != o.kmin)
    return fail("kmin alone", levels);
  only = {one.wsum.data(), nullptr, nullptr, nullptr, nullptr, nullptr};
  if (irt_column_reduce(v.data(), f.data(), levels, cols, w, miss, only) != IRT_OK ||
      (cols && memcmp(one.wsum.data(), o.wsum.data(), 4 * cols)))
    return fail("wsum alone", levels);
  return 0;
}

int main() {
  uint32_t s = 2468u;
  auto rnd = [&]() {
    s = s * 1664525u + 1013904223u;
    return (float)(s >> 8) * (1.f / 16777216.f);
  };
  const size_t colCounts[] = {0, 1, 7, 64, 65};
  for (int levels = 1; levels <= 95; levels += (levels < 6 ? 1 : 29))
    for (size_t cols : colCounts) {
      std::vector<float> v((size_t)levels * cols), w(levels);
      std::vector<uint8_t> f((size_t)levels * cols);
      for (auto &x : v) x = floorf(rnd() * 6.f) * 0.37f - 1.f;  // few distinct values: many ties
      for (auto &x : f) x = rnd() < 0.6f ? (uint8_t)(1 + (int)(rnd() * 200.f)) : 0;  // any non-zero byte is "found"
      for (auto &x : w) x = rnd() * 3.f - 1.f;
      w[0] = 0.f;
      if (check(levels, cols, v, f, nullptr, -7.5f) || check(levels, cols, v, f, w.data(), NAN)) return 1;
      std::fill(f.begin(), f.end(), 0);  // nothing found anywhere
      if (check(levels, cols, v, f, w.data(), -7.5f)) return 1;
    }
  // the refusals: fewer than one level; NULL value or found with columns to reduce
  std::vector<float> v(8, 1.f);
  std::vector<uint8_t> f(8, 1);
  Out o(4);
  int refused = 0;
  g_errors = 0;
  refused += irt_column_reduce(v.data(), f.data(), 0, 4, nullptr, 0.f, o.all()) == IRT_E_INVALID;
  refused += irt_column_reduce(v.data(), f.data(), -2, 4, nullptr, 0.f, o.all()) == IRT_E_INVALID;
  refused += irt_column_reduce(nullptr, f.data(), 2, 4, nullptr, 0.f, o.all()) == IRT_E_INVALID;
  refused += irt_column_reduce(v.data(), nullptr, 2, 4, nullptr, 0.f, o.all()) == IRT_E_INVALID;
  if (refused != 4 || g_errors != 4) return fail("a bad argument was accepted, or refused without a message", refused);
  // no columns: nothing is read, NULLs included; no outputs: nothing is written
  if (irt_column_reduce(nullptr, nullptr, 2, 0, nullptr, 0.f, o.all()) != IRT_OK) return fail("no columns refused", 0);
  const irt_column_out none = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  if (irt_column_reduce(v.data(), f.data(), 2, 4, nullptr, 0.f, none) != IRT_OK) return fail("no outputs refused", 4);
  printf("column_reduce_main: ok\n");
  return 0;
}
