// A stand-alone check of host/irt_overlay.cpp (irt_overlay_segments, irt_graticule, irt_overlay_bins,
// irt_overlay_cover), built by tests/test_overlay_cpu.py with -fsanitize=address,undefined and run
// there: every input and output array is a heap block of exactly the size the call may touch, so a
// read or write past it is the sanitizer's to report.  Exit status 0: every check passed.
#include <math.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "irt_internal.h"
#include "irt_overlay.h"

static int g_errors = 0;  // set_error calls seen

namespace irt {
void set_error(const char *fmt, ...) {
  (void)fmt;
  ++g_errors;
}
}  // namespace irt

static int fail(const char *what, long n) {
  fprintf(stderr, "overlay_main: %s (n = %ld)\n", what, n);
  return 1;
}

static const irt_overlay_style kStyles[2] = {{{0.9f, 0.45f, 0.15f, 1.0f}, 0.03f}, {{0.2f, 0.8f, 0.35f, 0.6f}, 0.012f}};

// segments of exactly the needed size, from a size query and a second call
static int make(bool graticule, const std::vector<float> &lat, const std::vector<float> &lon,
                const std::vector<int32_t> &first, float arc, int style, std::vector<irt_overlay_segment> &out) {
  size_t n = 0;
  const int lines = (int)first.size() - 1;
  int rc = graticule ? irt_graticule(lat[0], lon[0], arc, style, nullptr, 0, &n)
                     : irt_overlay_segments(lat.data(), lon.data(), first.data(), lines, arc, style, nullptr, 0, &n);
  if (rc != IRT_OK) return fail("size query refused", rc);
  out.assign(n, irt_overlay_segment{});
  rc = graticule ? irt_graticule(lat[0], lon[0], arc, style, out.data(), out.size(), &n)
                 : irt_overlay_segments(lat.data(), lon.data(), first.data(), lines, arc, style, out.data(),
                                        out.size(), &n);
  if (rc != IRT_OK || n != out.size()) return fail("fill refused", rc);
  if (n > 0) {  // one short: refused, nothing written
    std::vector<irt_overlay_segment> less(n - 1, irt_overlay_segment{});
    const int before = g_errors;
    rc = graticule ? irt_graticule(lat[0], lon[0], arc, style, less.data(), less.size(), &n)
                   : irt_overlay_segments(lat.data(), lon.data(), first.data(), lines, arc, style, less.data(),
                                          less.size(), &n);
    if (rc != IRT_E_INVALID || g_errors != before + 1) return fail("a short array was accepted", (long)n);
    for (const irt_overlay_segment &s : less)
      if (s.sinHalf != 0.f) return fail("a refused call wrote", (long)n);
  }
  for (const irt_overlay_segment &s : out) {
    const float la = irt::ov_dot(s.a, s.a), ln = irt::ov_dot(s.n, s.n), lt = irt::ov_dot(s.t, s.t);
    if (fabsf(la - 1.f) > 1e-6f || fabsf(ln - 1.f) > 1e-6f || fabsf(lt - 1.f) > 1e-6f) return fail("not unit", 0);
    if (s.style != style || s.pad[0] || s.pad[1]) return fail("style or pad", s.style);
  }
  return 0;
}

// the bins of exactly the needed size; cover through them equals the scan on the points
static int compare(const std::vector<irt_overlay_segment> &seg, int N, const std::vector<float> &u) {
  const size_t pts = u.size() / 3;
  std::vector<int32_t> scan(pts, -7), binned(pts, -7);
  if (irt_overlay_cover(seg.data(), seg.size(), kStyles, 2, nullptr, nullptr, 0, u.data(), pts, scan.data()))
    return fail("scan refused", N);
  std::vector<uint32_t> start(6 * (size_t)N * N + 1, 0xA5A5A5A5u);
  size_t entries = 0;
  if (irt_overlay_bins(seg.data(), seg.size(), 0.03f, N, start.data(), nullptr, 0, &entries)) return fail("bins query", N);
  if (start.back() != entries) return fail("binStart's end", (long)entries);
  std::vector<uint32_t> lists(entries, 0xA5A5A5A5u);
  if (irt_overlay_bins(seg.data(), seg.size(), 0.03f, N, start.data(), lists.data(), lists.size(), &entries))
    return fail("bins fill", N);
  for (size_t b = 0; b + 1 < start.size(); ++b)
    for (uint32_t k = start[b]; k < start[b + 1]; ++k) {
      if (lists[k] >= seg.size()) return fail("an entry outside the segments", (long)lists[k]);
      if (k > start[b] && lists[k] <= lists[k - 1]) return fail("a list does not ascend", (long)b);
    }
  if (irt_overlay_cover(seg.data(), seg.size(), kStyles, 2, start.data(), lists.data(), N, u.data(), pts, binned.data()))
    return fail("binned cover refused", N);
  long hits = 0;
  for (size_t p = 0; p < pts; ++p) {
    if (scan[p] != binned[p]) return fail("bins differ from the scan", (long)p);
    if (scan[p] < -1 || scan[p] >= (int32_t)seg.size()) return fail("an answer outside the segments", scan[p]);
    hits += scan[p] >= 0;
  }
  return hits > 0 || seg.empty() ? 0 : fail("no point was covered", N);
}

int main() {
  std::vector<irt_overlay_segment> grat, walk, none;
  const std::vector<int32_t> noLines = {0};
  if (make(true, {0.5235988f}, {0.5235988f}, noLines, 0.0872665f, 0, grat)) return 1;
  if (grat.size() != 12 * 37 + 5 * 73) return fail("graticule size", (long)grat.size());
  // a walk of two lines with repeated points, a pole and a date-line crossing
  const std::vector<float> lat = {0.1f, 0.1f, 0.4f, 1.5707964f, 0.9f, -0.2f, -0.2f, -0.25f};
  const std::vector<float> lon = {3.1f, 3.1f, -3.1f, 0.f, 2.f, 1.f, 1.f, 1.3f};
  if (make(false, lat, lon, {0, 5, 8}, 0.05f, 1, walk)) return 1;
  if (walk.size() < 20) return fail("walk size", (long)walk.size());
  if (make(false, lat, lon, {0, 0}, 0.05f, 1, none) || !none.empty()) return fail("an empty line", 0);
  std::vector<irt_overlay_segment> all(grat);
  all.insert(all.end(), walk.begin(), walk.end());

  // points: on and beside the segments, the axes, cube edges and corners, bin borders
  std::vector<float> u;
  auto push = [&](double x, double y, double z) {
    const double l = sqrt(x * x + y * y + z * z);
    u.push_back((float)(x / l));
    u.push_back((float)(y / l));
    u.push_back((float)(z / l));
  };
  for (const irt_overlay_segment &s : all)
    for (double f : {0.0, 0.5, 1.0, 1.02, -0.99}) {
      push(s.a[0] + f * 0.03 * s.n[0], s.a[1] + f * 0.03 * s.n[1], s.a[2] + f * 0.03 * s.n[2]);
      push(s.a[0] + s.b[0] + f * 0.024 * s.n[0], s.a[1] + s.b[1] + f * 0.024 * s.n[1], s.a[2] + s.b[2] + f * 0.024 * s.n[2]);
    }
  for (int sx = -1; sx <= 1; ++sx)
    for (int sy = -1; sy <= 1; ++sy)
      for (int sz = -1; sz <= 1; ++sz)
        if (sx || sy || sz) push(sx, sy, sz);
  for (int k = 0; k <= 64; ++k) {
    const double e = -1.0 + 2.0 * k / 64;
    push(1, e, 0.37), push(-1, 0.11, e), push(e, 1, -0.6), push(0.2, -1, e), push(e, 0.45, 1), push(-0.8, e, -1);
  }
  for (int N : {1, 4, 64, 256})
    if (compare(all, N, u)) return 1;
  if (compare(none, 4, u)) return 1;  // no segments: every answer -1, no list entries

  // refusals leave the outputs alone
  std::vector<int32_t> got(1, 77);
  const int before = g_errors;
  irt_overlay_style wide = {{1, 1, 1, 1}, 0.06f};
  size_t n = 0;
  std::vector<uint32_t> start(7, 77u);
  if (irt_overlay_cover(all.data(), all.size(), &wide, 1, nullptr, nullptr, 0, u.data(), 1, got.data()) != IRT_E_INVALID ||
      irt_overlay_cover(all.data(), all.size(), kStyles, 1, nullptr, nullptr, 0, u.data(), 1, got.data()) != IRT_E_INVALID ||
      irt_overlay_bins(all.data(), all.size(), 0.f, 1, start.data(), nullptr, 0, &n) != IRT_E_INVALID ||
      irt_overlay_bins(all.data(), all.size(), 0.03f, 0, start.data(), nullptr, 0, &n) != IRT_E_INVALID ||
      irt_overlay_segments(lat.data(), lon.data(), noLines.data(), 0, 0.3f, 0, nullptr, 0, &n) != IRT_E_INVALID ||
      irt_graticule(0.f, 0.5f, 0.1f, 0, nullptr, 0, &n) != IRT_E_INVALID)
    return fail("a bad argument was accepted", 0);
  if (g_errors != before + 6 || got[0] != 77 || start[0] != 77u) return fail("a refusal wrote", g_errors - before);
  printf("overlay_main: ok (%zu segments, %zu points)\n", all.size(), u.size() / 3);
  return 0;
}
