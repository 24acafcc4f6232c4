// A stand-alone check of host/irt_contour.cpp (irt_contour_cells), built by tests/test_contour_cpu.py
// with -fsanitize=address,undefined and run there: every input and output array is a heap block of
// exactly the size the call may touch, so a read or write past it is the sanitizer's to report.
// Exit status 0: every check passed.
#include <math.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "irt_contour.h"
#include "irt_internal.h"

static int g_errors = 0;  // set_error calls seen

namespace irt {
void set_error(const char *fmt, ...) {
  (void)fmt;
  ++g_errors;
}
}  // namespace irt

static int fail(const char *what, long n) {
  fprintf(stderr, "contour_main: %s (n = %ld)\n", what, n);
  return 1;
}

struct Grid {
  std::vector<float> lat, lon, value;
  std::vector<uint8_t> found;
};

// value = z + 0.3 x y (+ a checkerboard term) on numLat x numLon points; wrap: the columns close
static Grid make_grid(int numLat, int numLon, bool wrap, float checker, bool holes) {
  Grid g;
  g.lat.resize(numLat);
  g.lon.resize(numLon);
  for (int j = 0; j < numLat; ++j) g.lat[j] = (float)(-1.5 + fmin(3.0 / (numLat - 1), 0.09) * j);
  for (int i = 0; i < numLon; ++i)
    g.lon[i] = wrap ? (float)(-3.1 + 2.0 * M_PI * i / numLon) : (float)(-1.0 + 0.09 * i);
  g.value.resize((size_t)numLat * numLon);
  g.found.assign((size_t)numLat * numLon, 1);
  for (int j = 0; j < numLat; ++j)
    for (int i = 0; i < numLon; ++i) {
      const double cl = cos((double)g.lat[j]), x = cl * cos((double)g.lon[i]), y = cl * sin((double)g.lon[i]);
      g.value[(size_t)j * numLon + i] = (float)(sin((double)g.lat[j]) + 0.3 * x * y) + (((i + j) & 1) ? checker : -checker);
      if (holes && (i * 7 + j * 3) % 23 == 0) g.found[(size_t)j * numLon + i] = 0;
    }
  if (holes) {
    g.value[(size_t)numLon + 1] = NAN;
    g.value.back() = INFINITY;  // the last point: the last cell's corner 2 (and the wrap cell's)
  }
  return g;
}

static int run(const Grid &g, bool withFound, const std::vector<float> &thr, int flags) {
  const int numLat = (int)g.lat.size(), numLon = (int)g.lon.size(), T = (int)thr.size();
  std::vector<int32_t> style(T);
  for (int t = 0; t < T; ++t) style[t] = t % IRT_OVERLAY_MAX_STYLES;
  const uint8_t *found = withFound ? g.found.data() : nullptr;
  size_t n = 0;
  std::vector<size_t> per(T, 7);
  // count only, without and with the per-threshold counts
  int rc = irt_contour_cells(g.value.data(), found, g.lat.data(), numLat, g.lon.data(), numLon, thr.data(),
                             style.data(), T, flags, nullptr, 0, &n, nullptr);
  if (rc != IRT_OK) return fail("size query refused", rc);
  size_t n2 = 0;
  rc = irt_contour_cells(g.value.data(), found, g.lat.data(), numLat, g.lon.data(), numLon, thr.data(), style.data(),
                         T, flags, nullptr, 0, &n2, per.data());
  size_t sum = 0;
  for (size_t p : per) sum += p;
  if (rc != IRT_OK || n2 != n || sum != n) return fail("the counts disagree", (long)n2);
  // exactly the size needed
  std::vector<irt_overlay_segment> out(n);
  if (!out.empty()) memset(out.data(), 0x5a, out.size() * sizeof(irt_overlay_segment));
  rc = irt_contour_cells(g.value.data(), found, g.lat.data(), numLat, g.lon.data(), numLon, thr.data(), style.data(),
                         T, flags, out.data(), out.size(), &n2, per.data());
  if (rc != IRT_OK || n2 != n) return fail("fill refused", rc);
  size_t k = 0;
  for (int t = 0; t < T; ++t)
    for (size_t q = 0; q < per[t]; ++q, ++k) {
      const irt_overlay_segment &s = out[k];
      if (s.style != style[t] || s.pad[0] || s.pad[1]) return fail("style or pad", (long)k);
      const float *f[4] = {s.a, s.b, s.n, s.t};
      for (int v = 0; v < 4; ++v) {
        const float l = (f[v][0] * f[v][0] + f[v][1] * f[v][1]) + f[v][2] * f[v][2];
        if (!(fabsf(l - 1.f) < 1e-5f)) return fail("not unit", (long)k);
      }
      if (!(s.sinHalf > 0.f && s.sinHalf <= 0.1f)) return fail("sinHalf", (long)k);
      if (s.a[0] == s.b[0] && s.a[1] == s.b[1] && s.a[2] == s.b[2]) return fail("a kept degenerate segment", (long)k);
    }
  if (n > 0) {  // one short: refused with the count set, nothing written
    std::vector<irt_overlay_segment> less(n - 1);
    if (!less.empty()) memset(less.data(), 0x5a, less.size() * sizeof(irt_overlay_segment));
    const int before = g_errors;
    n2 = 0;
    rc = irt_contour_cells(g.value.data(), found, g.lat.data(), numLat, g.lon.data(), numLon, thr.data(),
                           style.data(), T, flags, less.data(), less.size(), &n2, nullptr);
    if (rc != IRT_E_INVALID || g_errors != before + 1 || n2 != n) return fail("a short array was accepted", (long)n);
    const unsigned char *b = (const unsigned char *)less.data();
    for (size_t i = 0; i < less.size() * sizeof(irt_overlay_segment); ++i)
      if (b[i] != 0x5a) return fail("a refused call wrote", (long)i);
  }
  return 0;
}

int main() {
  const std::vector<float> some = {-0.6f, 0.0f, 0.35f, 0.8f, 0.35f};
  std::vector<float> many(IRT_CONTOUR_MAX_THRESHOLDS);
  for (size_t t = 0; t < many.size(); ++t) many[t] = -0.9f + 0.12f * (float)t;
  long total = 0;
  for (int wrap = 0; wrap < 2; ++wrap) {
    const int flags = wrap ? IRT_CONTOUR_WRAP : 0;
    if (run(make_grid(37, 67, wrap, 0.f, false), false, some, flags)) return 1;
    if (run(make_grid(37, 67, wrap, 0.f, true), true, some, flags)) return 1;
    if (run(make_grid(35, 64, wrap, 1.f, true), true, many, flags)) return 1;   // saddles everywhere
    if (run(make_grid(2, 64, wrap, 0.f, false), false, {0.0f}, flags)) return 1;
    ++total;
  }
  if (run(make_grid(2, 2, false, 0.f, false), false, {0.0f, 0.9f}, 0)) return 1;  // one cell
  // refusals read nothing they should not: a grid of two points per axis and bad counts
  {
    const Grid g = make_grid(2, 2, false, 0.f, false);
    const std::vector<float> thr = {0.f};
    const std::vector<int32_t> sty = {0};
    size_t n = 99;
    const int before = g_errors;
    if (irt_contour_cells(g.value.data(), nullptr, g.lat.data(), 2, g.lon.data(), 2, thr.data(), sty.data(), 1,
                          IRT_CONTOUR_WRAP, nullptr, 0, &n, nullptr) != IRT_E_INVALID)
      return fail("a wrap over 0.09 rad was accepted", 0);
    if (irt_contour_cells(g.value.data(), nullptr, g.lat.data(), 2, g.lon.data(), 2, thr.data(), sty.data(), 0, 0,
                          nullptr, 0, &n, nullptr) != IRT_E_INVALID)
      return fail("zero thresholds were accepted", 0);
    if (irt_contour_cells(g.value.data(), nullptr, g.lat.data(), 1, g.lon.data(), 2, thr.data(), sty.data(), 1, 0,
                          nullptr, 0, &n, nullptr) != IRT_E_INVALID)
      return fail("one row was accepted", 0);
    if (g_errors != before + 3 || n != 99) return fail("refusals", (long)n);
  }
  printf("contour_main: ok (%ld grid pairs)\n", total);
  return 0;
}
