// irt_overlay.cpp -- the host side of the lines on the globe (include/icon_rt_hip.h, "overlay"):
// polylines and the graticule as great-circle segments (irt_overlay_segments, irt_graticule), the
// cube-map bin table (irt_overlay_bins), and the cover test applied to points (irt_overlay_cover,
// the definition the kernel is held to: csrc/irt_overlay.h).  No GPU here; the device object, the
// kernel and the context entry points are in csrc/irt_overlay.hip.

#include <math.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "irt_internal.h"
#include "irt_overlay.h"

namespace irt {
namespace {

struct D3 {
  double x, y, z;
};
D3 cross(const D3 &a, const D3 &b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
double dot(const D3 &a, const D3 &b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
double norm(const D3 &a) { return sqrt(dot(a, a)); }
D3 unit(const D3 &a) {
  const double l = norm(a);
  return {a.x / l, a.y / l, a.z / l};
}
double angle(const D3 &a, const D3 &b) { return atan2(norm(cross(a, b)), dot(a, b)); }
// the axes of to_cartesian_trig (irt_build.h) / irt_latlon_points
D3 from_latlon(float lat, float lon) {
  const double cl = cos((double)lat);
  return {cl * cos((double)lon), cl * sin((double)lon), sin((double)lat)};
}
void put3(float *o, const D3 &v) {
  o[0] = (float)v.x;
  o[1] = (float)v.y;
  o[2] = (float)v.z;
}
bool same_float(const D3 &a, const D3 &b) {
  return (float)a.x == (float)b.x && (float)a.y == (float)b.y && (float)a.z == (float)b.z;
}

bool arc_ok(float maxArc) { return maxArc > 0.f && maxArc <= kOverlayMaxArc; }
bool width_ok(float w) { return w > 0.f && w <= kOverlayMaxHalfWidth; }

// one piece pa -> pb (unit vectors in double, distinct): every field rounded to float at the end
void make_segment(const D3 &pa, const D3 &pb, int style, irt_overlay_segment &s) {
  memset(&s, 0, sizeof(s));
  put3(s.a, pa);
  put3(s.b, pb);
  put3(s.n, unit(cross(pa, pb)));
  put3(s.t, unit(D3{pb.x - pa.x, pb.y - pa.y, pb.z - pa.z}));
  s.sinHalf = (float)sin(0.5 * angle(pa, pb));
  s.style = style;
}

// the face frame of csrc/irt_overlay.h overlay_bin: direction of (face, p, q)
D3 face_point(int face, double p, double q) {
  const int axis = face >> 1;
  const double m = (face & 1) ? -1.0 : 1.0;
  if (axis == 0) return unit(D3{m, p, q});
  if (axis == 1) return unit(D3{p, m, q});
  return unit(D3{p, q, m});
}

}  // namespace

int overlay_styles(const char *what, const irt_overlay_style *styles, int numStyles, OverlayStyle *out) {
  if (numStyles < 1 || numStyles > IRT_OVERLAY_MAX_STYLES) {
    set_error("%s: %d styles are outside [1, %d]", what, numStyles, IRT_OVERLAY_MAX_STYLES);
    return IRT_E_INVALID;
  }
  if (!styles) {
    set_error("%s: null styles", what);
    return IRT_E_INVALID;
  }
  for (int k = 0; k < numStyles; ++k) {
    const irt_overlay_style &s = styles[k];
    if (!width_ok(s.halfWidth)) {
      set_error("%s: style %d: halfWidth %g is outside (0, %g] rad", what, k, (double)s.halfWidth,
                (double)kOverlayMaxHalfWidth);
      return IRT_E_INVALID;
    }
    if (!(isfinite(s.rgba.x) && isfinite(s.rgba.y) && isfinite(s.rgba.z) && isfinite(s.rgba.w))) {
      set_error("%s: style %d: rgba is not finite", what, k);
      return IRT_E_INVALID;
    }
  }
  for (int k = 0; k < numStyles; ++k) {
    const irt_overlay_style &s = styles[k];
    OverlayStyle &o = out[k];
    memset(&o, 0, sizeof(o));
    o.L[0] = s.rgba.x * s.rgba.w;
    o.L[1] = s.rgba.y * s.rgba.w;
    o.L[2] = s.rgba.z * s.rgba.w;
    o.L[3] = s.rgba.w;
    const double W = (double)s.halfWidth, c = 2.0 * sin(0.5 * W);
    o.sinW = (float)sin(W);
    o.chord2 = (float)(c * c);
  }
  return IRT_OK;
}

int overlay_segments_ok(const char *what, const irt_overlay_segment *seg, size_t n, int numStyles) {
  if (n >= kOverlayMaxSegments) {
    set_error("%s: %zu segments (fewer than 2^24)", what, n);
    return IRT_E_INVALID;
  }
  if (n && !seg) {
    set_error("%s: null segments", what);
    return IRT_E_INVALID;
  }
  for (size_t i = 0; i < n; ++i)
    if (seg[i].style < 0 || seg[i].style >= numStyles) {
      set_error("%s: segment %zu: style %d is outside the table of %d", what, i, seg[i].style, numStyles);
      return IRT_E_INVALID;
    }
  return IRT_OK;
}

float overlay_max_half_width(const irt_overlay_style *styles, int numStyles) {
  float w = 0.f;
  for (int k = 0; k < numStyles; ++k) w = std::max(w, styles[k].halfWidth);
  return w;
}

// N doubles from 1 until the estimated mean list -- a segment's cap of radius rho meets about
// (1 + rho N 4 / pi)^2 bins of edge (pi / 2) / N -- is at most kOverlayListTarget
int overlay_auto_bins(const irt_overlay_segment *seg, size_t n, float maxHalfWidth) {
  if (n == 0) return 1;
  double rho = 0.0;
  for (size_t i = 0; i < n; ++i) rho += asin(std::min(1.0, (double)fabsf(seg[i].sinHalf)));
  rho = rho / (double)n + (double)maxHalfWidth;
  int N = 1;
  for (; N < kOverlayMaxBins; N *= 2) {
    const double per = 1.0 + rho * N * (4.0 / M_PI);
    if ((double)n * per * per / (6.0 * N * N) <= (double)kOverlayListTarget) break;
  }
  return N;
}

}  // namespace irt

using namespace irt;

extern "C" {

int irt_overlay_width(const irt_launch_params *lp, float surfaceRadius, float pixels, float *halfWidth) {
  const char *what = "irt_overlay_width";
  if (!lp || !halfWidth) {
    set_error("%s: null lp or halfWidth", what);
    return IRT_E_INVALID;
  }
  if (!(isfinite(surfaceRadius) && surfaceRadius > 0.f && isfinite(pixels) && pixels > 0.f)) {
    set_error("%s: surfaceRadius %g and pixels %g must be finite and positive", what, (double)surfaceRadius,
              (double)pixels);
    return IRT_E_INVALID;
  }
  const D3 du{lp->dir_du.x, lp->dir_du.y, lp->dir_du.z}, dv{lp->dir_dv.x, lp->dir_dv.y, lp->dir_dv.z};
  const D3 d0{lp->dir_00.x, lp->dir_00.y, lp->dir_00.z}, o{lp->org.x, lp->org.y, lp->org.z};
  const D3 n = cross(du, dv);
  const double focal = fabs(dot(d0, n)) / std::max(norm(n), 1e-300);
  const double pixelAngle = norm(dv) / std::max(focal, 1e-300);
  const double dist = fabs(norm(o) - (double)surfaceRadius);
  const double w = 0.5 * (double)pixels * pixelAngle * dist / (double)surfaceRadius;
  *halfWidth = (float)std::min(std::max(w, 1e-7), (double)kOverlayMaxHalfWidth);
  return IRT_OK;
}

int irt_overlay_segments(const float *lat, const float *lon, const int32_t *first, int numLines, float maxArc,
                         int style, irt_overlay_segment *out, size_t capacity, size_t *count) {
  const char *what = "irt_overlay_segments";
  if (!count) {
    set_error("%s: null count", what);
    return IRT_E_INVALID;
  }
  if (numLines < 0) {
    set_error("%s: %d lines", what, numLines);
    return IRT_E_INVALID;
  }
  if (!arc_ok(maxArc)) {
    set_error("%s: maxArc %g is outside (0, %g] rad", what, (double)maxArc, (double)kOverlayMaxArc);
    return IRT_E_INVALID;
  }
  if (style < 0 || style >= IRT_OVERLAY_MAX_STYLES) {
    set_error("%s: style %d is outside [0, %d)", what, style, IRT_OVERLAY_MAX_STYLES);
    return IRT_E_INVALID;
  }
  if (numLines && !first) {
    set_error("%s: null first", what);
    return IRT_E_INVALID;
  }
  for (int l = 0; l < numLines; ++l)
    if (first[l] < 0 || first[l + 1] < first[l]) {
      set_error("%s: first[%d] = %d, first[%d] = %d do not ascend from 0", what, l, first[l], l + 1, first[l + 1]);
      return IRT_E_INVALID;
    }
  const size_t numPoints = numLines ? (size_t)first[numLines] : 0;
  if (numPoints && (!lat || !lon)) {
    set_error("%s: null lat or lon", what);
    return IRT_E_INVALID;
  }
  for (size_t i = numLines ? (size_t)first[0] : 0; i < numPoints; ++i)
    if (!(isfinite(lat[i]) && isfinite(lon[i]))) {
      set_error("%s: point %zu (%g, %g) is not finite", what, i, (double)lat[i], (double)lon[i]);
      return IRT_E_INVALID;
    }
  // first pass: the legs (after merging) and their piece counts; second pass: the pieces
  struct Leg {
    D3 a, b;
    double omega;
    size_t pieces;
  };
  std::vector<Leg> legs;
  size_t total = 0;
  for (int l = 0; l < numLines; ++l) {
    bool have = false;
    D3 prev{};
    for (int i = first[l]; i < first[l + 1]; ++i) {
      const D3 p = from_latlon(lat[i], lon[i]);
      if (have && same_float(prev, p)) continue;  // merged
      if (have) {
        const double omega = angle(prev, p);
        if (sin(omega) < 1e-9 && dot(prev, p) < 0.0) {
          set_error("%s: points %d and %d are antipodal: no unique great circle", what, i - 1, i);
          return IRT_E_INVALID;
        }
        const size_t pieces = std::max<size_t>(1, (size_t)ceil(omega / (double)maxArc));
        legs.push_back({prev, p, omega, pieces});
        total += pieces;
      }
      prev = p;
      have = true;
    }
  }
  *count = total;
  if (!out) return IRT_OK;  // size query
  if (capacity < total) {
    set_error("%s: capacity %zu < %zu segments", what, capacity, total);
    return IRT_E_INVALID;
  }
  size_t k = 0;
  for (const Leg &g : legs) {
    const double so = sin(g.omega);
    D3 pa = g.a;
    for (size_t j = 1; j <= g.pieces; ++j) {
      D3 pb = g.b;
      if (j < g.pieces) {  // slerp; the end points are the leg's own
        const double t = (double)j / (double)g.pieces;
        const double wa = sin((1.0 - t) * g.omega) / so, wb = sin(t * g.omega) / so;
        pb = unit(D3{wa * g.a.x + wb * g.b.x, wa * g.a.y + wb * g.b.y, wa * g.a.z + wb * g.b.z});
      }
      make_segment(pa, pb, style, out[k++]);
      pa = pb;
    }
  }
  return IRT_OK;
}

int irt_graticule(float stepLat, float stepLon, float maxArc, int style, irt_overlay_segment *out, size_t capacity,
                  size_t *count) {
  const char *what = "irt_graticule";
  if (!(stepLat > 0.f && stepLat <= (float)M_PI && stepLon > 0.f && stepLon <= (float)(2.0 * M_PI))) {
    set_error("%s: steps (%g, %g) rad are outside (0, pi] x (0, 2 pi]", what, (double)stepLat, (double)stepLon);
    return IRT_E_INVALID;
  }
  if (!arc_ok(maxArc)) {
    set_error("%s: maxArc %g is outside (0, %g] rad", what, (double)maxArc, (double)kOverlayMaxArc);
    return IRT_E_INVALID;
  }
  std::vector<float> lat, lon;
  std::vector<int32_t> first(1, 0);
  // polyline points a little closer than maxArc, so that float rounding does not split a piece
  const double arc = (double)maxArc * 0.9999;
  // meridians lon = m stepLon, m = 0 .. floor(2 pi / stepLon) - 1, pole to pole
  const int numMer = (int)floor(2.0 * M_PI / (double)stepLon + 1e-6);
  const int merPieces = (int)ceil(M_PI / arc);
  for (int m = 0; m < numMer; ++m) {
    for (int i = 0; i <= merPieces; ++i) {
      lat.push_back((float)(-0.5 * M_PI + M_PI * (double)i / (double)merPieces));
      lon.push_back((float)((double)m * (double)stepLon));
    }
    first.push_back((int32_t)lat.size());
  }
  // parallels lat = k stepLat, |lat| < pi / 2 (the equator is k = 0), closed chains
  const int numPar = (int)ceil(0.5 * M_PI / (double)stepLat - 1e-6) - 1;
  const int parPieces = (int)ceil(2.0 * M_PI / arc);
  for (int k = -numPar; k <= numPar; ++k) {
    for (int i = 0; i <= parPieces; ++i) {
      lat.push_back((float)((double)k * (double)stepLat));
      lon.push_back((float)(2.0 * M_PI * (double)(i % parPieces) / (double)parPieces));
    }
    first.push_back((int32_t)lat.size());
  }
  const int rc = irt_overlay_segments(lat.data(), lon.data(), first.data(), (int)first.size() - 1, maxArc, style, out,
                                      capacity, count);
  return rc;
}

int irt_overlay_bins(const irt_overlay_segment *seg, size_t n, float maxHalfWidth, int binsPerEdge,
                     uint32_t *binStart, uint32_t *binSeg, size_t capacity, size_t *count) {
  const char *what = "irt_overlay_bins";
  if (!count || !binStart) {
    set_error("%s: null count or binStart", what);
    return IRT_E_INVALID;
  }
  if (binsPerEdge < 1 || binsPerEdge > kOverlayMaxBins) {
    set_error("%s: binsPerEdge %d is outside [1, %d]", what, binsPerEdge, kOverlayMaxBins);
    return IRT_E_INVALID;
  }
  if (!width_ok(maxHalfWidth)) {
    set_error("%s: maxHalfWidth %g is outside (0, %g] rad", what, (double)maxHalfWidth, (double)kOverlayMaxHalfWidth);
    return IRT_E_INVALID;
  }
  int rc = overlay_segments_ok(what, seg, n, IRT_OVERLAY_MAX_STYLES);
  if (rc) return rc;
  for (size_t i = 0; i < n; ++i) {
    const irt_overlay_segment &s = seg[i];
    bool ok = isfinite(s.sinHalf) && s.sinHalf >= 0.f && s.sinHalf <= 1.f;
    for (int k = 0; k < 3; ++k) ok = ok && isfinite(s.a[k]) && isfinite(s.b[k]);
    if (!ok) {
      set_error("%s: segment %zu has end points or a sinHalf that are not finite", what, i);
      return IRT_E_INVALID;
    }
  }
  const int N = binsPerEdge;
  const size_t numBins = 6 * (size_t)N * (size_t)N;
  const double slack = 1e-5;
  // a bin's bounding cap: its centre and the largest corner angle, the same on every face
  std::vector<double> binRadius((size_t)N * N);
  for (int j = 0; j < N; ++j)
    for (int i = 0; i < N; ++i) {
      const double p0 = -1.0 + 2.0 * i / N, p1 = -1.0 + 2.0 * (i + 1) / N, q0 = -1.0 + 2.0 * j / N,
                   q1 = -1.0 + 2.0 * (j + 1) / N;
      const D3 c = face_point(0, 0.5 * (p0 + p1), 0.5 * (q0 + q1));
      binRadius[(size_t)j * N + i] = std::max(std::max(angle(c, face_point(0, p0, q0)), angle(c, face_point(0, p1, q0))),
                                              std::max(angle(c, face_point(0, p0, q1)), angle(c, face_point(0, p1, q1))));
    }
  const double maxBinRadius = *std::max_element(binRadius.begin(), binRadius.end());
  // Two passes over the segments in index order (count, then fill): each list ascends.  visit(i, f)
  // calls f(bin) for every bin whose cap comes within the radii's sum + slack of segment i's cap.
  auto visit = [&](size_t si, auto &&f) {
    const irt_overlay_segment &s = seg[si];
    const D3 a{s.a[0], s.a[1], s.a[2]}, b{s.b[0], s.b[1], s.b[2]};
    D3 m{a.x + b.x, a.y + b.y, a.z + b.z};
    const bool whole = !(norm(m) > 1e-3);  // (no such arc comes from irt_overlay_segments): every bin
    if (!whole) m = unit(m);
    const double rho = 0.5 * angle(a, b) + (double)maxHalfWidth + slack;
    // the ball around m that holds the centre of every bin within reach (chord <= angle)
    const double r = rho + maxBinRadius + 1e-6;
    for (int face = 0; face < 6; ++face) {
      int i0 = 0, i1 = N - 1, j0 = 0, j1 = N - 1;
      if (!whole) {
        const int axis = face >> 1;
        const double sgn = (face & 1) ? -1.0 : 1.0;
        const double mm = sgn * (axis == 0 ? m.x : (axis == 1 ? m.y : m.z));
        const double mp = axis == 0 ? m.y : m.x, mq = axis == 2 ? m.y : m.z;
        if (mm + r < 0.55) continue;  // a face's directions have major >= 1 / sqrt 3 = 0.577
        if (mm - r > 0.1) {           // the ball's shadow on the face plane, one bin of margin
          const double lo = mm - r, hi = mm + r;
          const double pl = std::min((mp - r) / lo, (mp - r) / hi), ph = std::max((mp + r) / lo, (mp + r) / hi);
          const double ql = std::min((mq - r) / lo, (mq - r) / hi), qh = std::max((mq + r) / lo, (mq + r) / hi);
          auto cell = [&](double v) { return (int)std::min<double>(N - 1, std::max(0.0, floor((v + 1.0) * 0.5 * N))); };
          i0 = std::max(0, cell(pl) - 1), i1 = std::min(N - 1, cell(ph) + 1);
          j0 = std::max(0, cell(ql) - 1), j1 = std::min(N - 1, cell(qh) + 1);
        }
      }
      for (int j = j0; j <= j1; ++j)
        for (int i = i0; i <= i1; ++i) {
          if (!whole) {
            const D3 c = face_point(face, -1.0 + (2.0 * i + 1.0) / N, -1.0 + (2.0 * j + 1.0) / N);
            if (angle(c, m) > binRadius[(size_t)j * N + i] + rho) continue;
          }
          f(((size_t)face * N + j) * N + i);
        }
    }
  };
  std::vector<uint32_t> cnt(numBins + 1, 0u);
  size_t total = 0;
  for (size_t si = 0; si < n; ++si)
    visit(si, [&](size_t bin) {
      ++cnt[bin + 1];
      ++total;
    });
  *count = total;
  if (total >= (size_t(1) << 32)) {
    set_error("%s: %zu list entries (fewer than 2^32): use fewer bins per edge", what, total);
    return IRT_E_INVALID;
  }
  if (binSeg && capacity < total) {
    set_error("%s: capacity %zu < %zu list entries", what, capacity, total);
    return IRT_E_INVALID;
  }
  for (size_t k = 0; k < numBins; ++k) cnt[k + 1] += cnt[k];
  memcpy(binStart, cnt.data(), (numBins + 1) * sizeof(uint32_t));
  if (!binSeg) return IRT_OK;  // size query: binStart alone
  std::vector<uint32_t> fill(cnt.begin(), cnt.end() - 1);
  for (size_t si = 0; si < n; ++si) visit(si, [&](size_t bin) { binSeg[fill[bin]++] = (uint32_t)si; });
  return IRT_OK;
}

int irt_overlay_cover(const irt_overlay_segment *seg, size_t n, const irt_overlay_style *styles, int numStyles,
                      const uint32_t *binStart, const uint32_t *binSeg, int binsPerEdge, const float *u,
                      size_t numPoints, int32_t *segment) {
  const char *what = "irt_overlay_cover";
  OverlayStyle st[IRT_OVERLAY_MAX_STYLES];
  int rc = overlay_styles(what, styles, numStyles, st);
  if (rc) return rc;
  if ((rc = overlay_segments_ok(what, seg, n, numStyles))) return rc;
  if (binStart && (binsPerEdge < 1 || binsPerEdge > kOverlayMaxBins)) {
    set_error("%s: binsPerEdge %d is outside [1, %d]", what, binsPerEdge, kOverlayMaxBins);
    return IRT_E_INVALID;
  }
  if (binStart && !binSeg && binStart[6 * (size_t)binsPerEdge * binsPerEdge] != 0u) {
    set_error("%s: null binSeg with list entries", what);
    return IRT_E_INVALID;
  }
  if (numPoints && (!u || !segment)) {
    set_error("%s: null u or segment", what);
    return IRT_E_INVALID;
  }
  for (size_t p = 0; p < numPoints; ++p)
    segment[p] = overlay_find(seg, (uint32_t)n, st, binStart, binSeg, binsPerEdge, u + 3 * p);
  return IRT_OK;
}

}  // extern "C"
