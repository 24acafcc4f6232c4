// A stand-alone check of host/irt_section.cpp (irt_section_points and irt_great_circle, the host
// helpers of the sections), built by tests/test_section_cpu.py with -fsanitize=address,undefined and
// run there: every input and output array is a heap block of exactly the size the call may touch,
// so a read or write past it is the sanitizer's to report.  Exit status 0: every check passed.
#include <math.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "irt_build.h"
#include "irt_internal.h"

static int g_errors = 0;  // set_error calls seen

namespace irt {
void set_error(const char *fmt, ...) {
  (void)fmt;
  ++g_errors;
}
int default_threads() { return 3; }  // the long lists below are split: chunk edges under the sanitizers too
}  // namespace irt

static int fail(const char *what, int n) {
  fprintf(stderr, "section_main: %s (n = %d)\n", what, n);
  return 1;
}

// irt_section_points of `cols` pairs on `levels` radii against toCartesian written out
static int check_points(int levels, int cols, uint32_t &s) {
  auto rnd = [&]() {
    s = s * 1664525u + 1013904223u;
    return (float)(s >> 8) * (1.f / 16777216.f);
  };
  std::vector<float> lat(cols), lon(cols), rad(levels), xyz((size_t)3 * levels * cols, -1.f);
  for (auto &x : lat) x = (rnd() - 0.5f) * 3.1415927f;
  for (auto &x : lon) x = (rnd() - 0.5f) * 6.2831855f;
  for (auto &x : rad) x = 6.3e6f + rnd() * 1e5f;
  if (cols > 2) {  // a pole, the date line, a repeated pair
    lat[0] = 1.5707964f;
    lon[1] = -3.1415927f;
    lat[2] = lat[1];
    lon[2] = lon[1];
  }
  if (irt_section_points(lat.data(), lon.data(), cols, rad.data(), levels, xyz.data()) != IRT_OK)
    return fail("points refused", cols);
  for (int k = 0; k < levels; ++k)
    for (int c = 0; c < cols; ++c) {
      const float rc = rad[k] * cosf(lat[c]);
      const float want[3] = {rc * cosf(lon[c]), rc * sinf(lon[c]), rad[k] * sinf(lat[c])};
      if (memcmp(want, &xyz[3 * ((size_t)k * cols + c)], 12)) return fail("a point differs from toCartesian", cols);
    }
  return 0;
}

// irt_great_circle: end points unchanged, every point a unit step along the arc
static int check_circle(float lat0, float lon0, float lat1, float lon1, int n) {
  std::vector<float> lat(n, 9.f), lon(n, 9.f);
  double arc = -1.0;
  if (irt_great_circle(lat0, lon0, lat1, lon1, n, lat.data(), lon.data(), &arc) != IRT_OK)
    return fail("circle refused", n);
  if (lat[0] != lat0 || lon[0] != lon0) return fail("the start moved", n);
  if (n > 1 && (lat[n - 1] != lat1 || lon[n - 1] != lon1)) return fail("the end moved", n);
  if (!(arc >= 0.0 && arc <= 3.141592653589794)) return fail("arc out of range", n);
  auto unit = [](float la, float lo, double *p) {
    p[0] = cos((double)la) * cos((double)lo);
    p[1] = cos((double)la) * sin((double)lo);
    p[2] = sin((double)la);
  };
  for (int i = 0; i + 1 < n; ++i) {
    double a[3], b[3];
    unit(lat[i], lon[i], a);
    unit(lat[i + 1], lon[i + 1], b);
    const double d = sqrt((a[0] - b[0]) * (a[0] - b[0]) + (a[1] - b[1]) * (a[1] - b[1]) + (a[2] - b[2]) * (a[2] - b[2]));
    const double step = 2.0 * sin(0.5 * arc / (n - 1));  // the chord of one step
    if (!(fabs(d - step) < 1e-6)) return fail("steps are not equal", i);
  }
  // without arc, and the call must not touch more than n elements (the vectors are exactly n long)
  if (irt_great_circle(lat0, lon0, lat1, lon1, n, lat.data(), lon.data(), nullptr) != IRT_OK)
    return fail("circle without arc refused", n);
  return 0;
}

int main() {
  uint32_t s = 97531u;
  const int colCounts[] = {0, 1, 7, 63, 64, 65, 130};
  for (int levels = 0; levels <= 5; ++levels)
    for (int cols : colCounts)
      if (check_points(levels, cols, s)) return 1;
  // lists long enough for section_trig's threads: a multiple of the three chunks, and ragged ones
  const int longCounts[] = {(int)irt::kSectionTrigSplit - 1, (int)irt::kSectionTrigSplit, (int)irt::kSectionTrigSplit + 1,
                            (int)irt::kSectionTrigSplit + 2};
  for (int cols : longCounts)
    if (check_points(2, cols, s)) return 1;
  const float hp = 1.5707964f;
  const int ns[] = {1, 2, 3, 64, 130};
  for (int n : ns) {
    if (check_circle(0.f, 3.0f, 0.f, -3.0f, n)) return 1;         // across the date line
    if (check_circle(1.0f, 0.3f, 0.9f, 0.3f + 3.1415927f, n)) return 1;  // over the pole
    if (check_circle(hp, 0.7f, -hp, 0.7f, n)) return 1;           // pole to pole
    if (check_circle(0.30f, -0.40f, 0.36f, -0.28f, n)) return 1;  // short
    if (check_circle(0.5f, 0.25f, 0.5f, 0.25f, n)) return 1;      // coincident
  }
  // the refusals, each with a message
  std::vector<float> lat(4, 0.1f), lon(4, 0.2f), rad(2, 6.4e6f), xyz(24);
  int refused = 0;
  g_errors = 0;
  refused += irt_section_points(lat.data(), lon.data(), -1, rad.data(), 2, xyz.data()) == IRT_E_INVALID;
  refused += irt_section_points(lat.data(), lon.data(), 4, rad.data(), -1, xyz.data()) == IRT_E_INVALID;
  refused += irt_section_points(nullptr, lon.data(), 4, rad.data(), 2, xyz.data()) == IRT_E_INVALID;
  refused += irt_section_points(lat.data(), nullptr, 4, rad.data(), 2, xyz.data()) == IRT_E_INVALID;
  refused += irt_section_points(lat.data(), lon.data(), 4, nullptr, 2, xyz.data()) == IRT_E_INVALID;
  refused += irt_section_points(lat.data(), lon.data(), 4, rad.data(), 2, nullptr) == IRT_E_INVALID;
  refused += irt_section_points(lat.data(), lon.data(), 1 << 30, rad.data(), 1 << 30, xyz.data()) == IRT_E_INVALID;
  refused += irt_great_circle(0.f, 0.f, 1.f, 1.f, 0, lat.data(), lon.data(), nullptr) == IRT_E_INVALID;
  refused += irt_great_circle(NAN, 0.f, 1.f, 1.f, 4, lat.data(), lon.data(), nullptr) == IRT_E_INVALID;
  refused += irt_great_circle(0.f, 0.f, 1.f, INFINITY, 4, lat.data(), lon.data(), nullptr) == IRT_E_INVALID;
  refused += irt_great_circle(0.f, 0.f, 1.f, 1.f, 4, nullptr, lon.data(), nullptr) == IRT_E_INVALID;
  refused += irt_great_circle(0.f, 0.f, 1.f, 1.f, 4, lat.data(), nullptr, nullptr) == IRT_E_INVALID;
  // antipodal: the two poles as floats, half a turn apart in lon (sin w ~ 4e-15)
  refused += irt_great_circle(hp, 0.f, -hp, 3.1415927f, 4, lat.data(), lon.data(), nullptr) == IRT_E_INVALID;
  if (refused != 13 || g_errors != 13) return fail("a bad argument was accepted, or refused without a message", refused);
  for (float v : lat)
    if (v != 0.1f) return fail("a refusal wrote", 0);
  // no points: nothing is read, NULLs included
  if (irt_section_points(nullptr, nullptr, 0, nullptr, 3, nullptr) != IRT_OK) return fail("no columns refused", 0);
  if (irt_section_points(lat.data(), lon.data(), 4, nullptr, 0, nullptr) != IRT_OK) return fail("no levels refused", 0);
  printf("section_main: ok\n");
  return 0;
}
