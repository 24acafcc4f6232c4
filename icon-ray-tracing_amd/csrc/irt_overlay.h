// irt_overlay.h -- lines on the globe (include/icon_rt_hip.h, "overlay"), defined once: which
// great-circle segment covers a unit vector, the cube-map bin of a unit vector, and the composite of
// the line layer with a frame's accum.  The host helpers (host/irt_overlay.cpp) and the kernel
// (csrc/irt_overlay.hip) compile this text.  Everything here is float (-ffp-contract=off, correctly
// rounded division): "equal" means equal integers and equal bits.
//
// A segment is an arc of a great circle no longer than 0.2 rad with a half-width W <= 0.05 rad: the
// set of unit vectors within W of the arc, as a body (a band of 2 W around the circle, cut at the
// arc's ends by the tangent at its midpoint, on the arc's side of the sphere) and two round caps.
// The caps are tested by chord length because cos W of a thin line rounds to 1.0f.
#pragma once

#include <stdint.h>

#include "icon_rt_hip.h"
#include "irt_common.h"

namespace irt {

constexpr int kOverlayMaxBins = 256;            // binsPerEdge
constexpr uint32_t kOverlayMaxSegments = 1u << 24;
constexpr float kOverlayMaxHalfWidth = 0.05f;   // radians
constexpr float kOverlayMaxArc = 0.2f;          // radians
constexpr int kOverlayListTarget = 16;          // binsPerEdge 0: the mean list length aimed at

// A style as the cover test and the kernel read it: 32 B
struct OverlayStyle {
  float L[4];    // the line sample (r a, g a, b a, a), one float multiply each
  float sinW;    // sin(W), in double, rounded once
  float chord2;  // (2 sin(W / 2))^2, in double, rounded once
  float pad[2];
};

IRT_HD float ov_dot(const float *x, const float *y) { return (x[0] * y[0] + x[1] * y[1]) + x[2] * y[2]; }
IRT_HD float ov_abs(float a) { return u2f(f2u(a) & 0x7fffffffu); }

IRT_HD bool overlay_body(const irt_overlay_segment &s, float sinW, const float *u) {
  return ov_abs(ov_dot(u, s.n)) <= sinW && ov_abs(ov_dot(u, s.t)) <= s.sinHalf && ov_dot(u, s.a) + ov_dot(u, s.b) > 0.f;
}
IRT_HD bool overlay_cap(const float *e, float chord2, const float *u) {
  const float d[3] = {u[0] - e[0], u[1] - e[1], u[2] - e[2]};
  return ov_dot(d, d) <= chord2;
}
// u is covered by s drawn in style st (a NaN in u compares false everywhere: not covered)
IRT_HD bool overlay_covers(const irt_overlay_segment &s, const OverlayStyle &st, const float *u) {
  return overlay_body(s, st.sinW, u) || overlay_cap(s.a, st.chord2, u) || overlay_cap(s.b, st.chord2, u);
}

// One axis of the bin: min((int)((p + 1.f) * 0.5f * N), N - 1) clamped at 0 (a NaN gives 0)
IRT_HD int overlay_bin_axis(float p, int N) {
  const float f = ((p + 1.f) * 0.5f) * (float)N;
  return f >= 0.f ? (f < (float)N ? (int)f : N - 1) : 0;
}
// The bin of a unit vector: face = 2 * (axis of the largest |component|, a tie to the lowest axis) +
// (that component negative), (p, q) the two other components in axis order over |major|
IRT_HD int overlay_bin(const float *u, int N) {
  const float ax = ov_abs(u[0]), ay = ov_abs(u[1]), az = ov_abs(u[2]);
  int axis = 0;
  float m = ax;
  if (ay > m) {
    axis = 1;
    m = ay;
  }
  if (az > m) {
    axis = 2;
    m = az;
  }
  const float major = axis == 0 ? u[0] : (axis == 1 ? u[1] : u[2]);
  const float pc = axis == 0 ? u[1] : u[0], qc = axis == 2 ? u[1] : u[2];
  const int face = 2 * axis + (major < 0.f ? 1 : 0);
  const int i = overlay_bin_axis(pc / m, N), j = overlay_bin_axis(qc / m, N);
  return (face * N + j) * N + i;
}

// The segment of u: the lowest index that covers it, or -1.  binStart == nullptr: every segment is
// scanned; else the list of u's bin, which ascends, so its first hit is the lowest.
IRT_HD int32_t overlay_find(const irt_overlay_segment *seg, uint32_t n, const OverlayStyle *styles,
                            const uint32_t *binStart, const uint32_t *binSeg, int N, const float *u) {
  if (!binStart) {
    for (uint32_t i = 0; i < n; ++i)
      if (overlay_covers(seg[i], styles[seg[i].style], u)) return (int32_t)i;
    return -1;
  }
  const int b = overlay_bin(u, N);
  for (uint32_t k = binStart[b]; k < binStart[b + 1]; ++k) {
    const uint32_t i = binSeg[k];
    if (overlay_covers(seg[i], styles[seg[i].style], u)) return (int32_t)i;
  }
  return -1;
}

// The frame: K is the line layer after its lerp, V the frame's accum (both premultiplied); one
// multiply and one add per component.  over: the lines on top of V, else under it.
IRT_HD void overlay_lerp(float w, const float *L, const float *old, float *K) {
  for (int k = 0; k < 4; ++k) K[k] = w * L[k] + (1.f - w) * old[k];
}
IRT_HD void overlay_composite(bool over, const float *V, const float *K, float *out) {
  const float *top = over ? K : V, *below = over ? V : K;
  const float rest = 1.f - top[3];
  for (int k = 0; k < 4; ++k) out[k] = top[k] + rest * below[k];
}

// Host side (host/irt_overlay.cpp): a user's styles as the cover test reads them, after the check
// (numStyles in [1, IRT_OVERLAY_MAX_STYLES], every width in (0, 0.05], rgba finite)
int overlay_styles(const char *what, const irt_overlay_style *styles, int numStyles, OverlayStyle *out);
// ... the check of a segment array against a style table (n < 2^24, NULL with segments, a style
// index outside the table), the largest half-width of the table, and the bins-per-edge a
// binsPerEdge of 0 stands for
int overlay_segments_ok(const char *what, const irt_overlay_segment *seg, size_t n, int numStyles);
float overlay_max_half_width(const irt_overlay_style *styles, int numStyles);
int overlay_auto_bins(const irt_overlay_segment *seg, size_t n, float maxHalfWidth);

}  // namespace irt
