// irt_contour.h -- isolines of a lat x lon value grid as overlay segments (include/icon_rt_hip.h,
// "isolines"), defined once: the corners of a cell, the crossing of an isoline with a cell edge, the
// segments of a cell by its mask, and the fields of a segment.  The host helper
// (host/irt_contour.cpp) and the kernels (csrc/irt_contour.hip) compile this text.  All arithmetic is
// double + - * / sqrt on float inputs, never contracted (-ffp-contract=off), with no libm call (the
// square root is the compiler's builtin: sqrtsd on the host, the correctly rounded f64 expansion on
// the device); the saddle's centre value alone is float.  "Equal" means equal bits.
//
// Nothing here indexes an array with a run-time index: the kernels keep a cell's corners, crossings
// and segments in registers.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "icon_rt_hip.h"
#include "irt_common.h"

namespace irt {

constexpr float kContourMaxStep = 0.1f;                // radians between neighbouring rows / columns
constexpr uint64_t kContourMaxPoints = uint64_t(1) << 27;  // numLat * numLon stays below
constexpr size_t kContourMaxSegments = size_t(1) << 24;    // the overlay's limit (kOverlayMaxSegments)

IRT_HD bool ctr_finite(float v) { return (f2u(v) & 0x7f800000u) != 0x7f800000u; }
IRT_HD double ctr_len(double x, double y, double z) { return __builtin_sqrt((x * x + y * y) + z * z); }

// A cell's corners 0 = (j, i), 1 = (j, i1), 2 = (j + 1, i1), 3 = (j + 1, i): unit vectors
// (cl * co, cl * si, sl) from the host's cos / sin tables, and values
struct ContourCell {
  double p[4][3];
  float v[4];
};

IRT_HD void ctr_corner(double cl, double sl, double co, double si, double *p) {
  p[0] = cl * co;
  p[1] = cl * si;
  p[2] = sl;
}

// The cell (j, i) with east column i1 (i + 1, or 0 in the closing column of a wrapped grid).  False:
// a corner is not found or not finite, the cell emits nothing (K is then not filled).
IRT_HD bool ctr_load(const float *value, const uint8_t *found, const double *latC, const double *latS,
                     const double *lonC, const double *lonS, int numLon, int j, int i, int i1, ContourCell &K) {
  const size_t r0 = (size_t)j * (size_t)numLon, r1 = r0 + (size_t)numLon;
  const size_t at[4] = {r0 + (size_t)i, r0 + (size_t)i1, r1 + (size_t)i1, r1 + (size_t)i};
  bool ok = true;
  for (int k = 0; k < 4; ++k) {
    K.v[k] = value[at[k]];
    ok = ok && ctr_finite(K.v[k]) && (!found || found[at[k]] != 0);
  }
  if (!ok) return false;
  ctr_corner(latC[j], latS[j], lonC[i], lonS[i], K.p[0]);
  ctr_corner(latC[j], latS[j], lonC[i1], lonS[i1], K.p[1]);
  ctr_corner(latC[j + 1], latS[j + 1], lonC[i1], lonS[i1], K.p[2]);
  ctr_corner(latC[j + 1], latS[j + 1], lonC[i], lonS[i], K.p[3]);
  return true;
}

// The crossing of the isoline c with the edge from corner A (value va) to corner B (vb), va != vb
IRT_HD void ctr_cross(const double *A, const double *B, float va, float vb, float c, double *P) {
  const double t = ((double)c - (double)va) / ((double)vb - (double)va);
  const double px = A[0] + t * (B[0] - A[0]), py = A[1] + t * (B[1] - A[1]), pz = A[2] + t * (B[2] - A[2]);
  const double l = ctr_len(px, py, pz);
  P[0] = px / l;
  P[1] = py / l;
  P[2] = pz / l;
}

// crossing e of E[4][3] (e in [0, 4)) without a run-time index
IRT_HD void ctr_pick(const double (*E)[3], int e, double *P) {
  for (int k = 0; k < 3; ++k) P[k] = e == 0 ? E[0][k] : (e == 1 ? E[1][k] : (e == 2 ? E[2][k] : E[3][k]));
}

// dropped: the end points are equal as floats
IRT_HD bool ctr_same(const double *a, const double *b) {
  return (float)a[0] == (float)b[0] && (float)a[1] == (float)b[1] && (float)a[2] == (float)b[2];
}

// The record of the segment Pa -> Pb (distinct as floats): every field rounded once
IRT_HD void ctr_segment(const double *a, const double *b, int32_t style, irt_overlay_segment &s) {
  const double nx = a[1] * b[2] - a[2] * b[1], ny = a[2] * b[0] - a[0] * b[2], nz = a[0] * b[1] - a[1] * b[0];
  const double ln = ctr_len(nx, ny, nz);
  const double dx = b[0] - a[0], dy = b[1] - a[1], dz = b[2] - a[2];
  const double ld = ctr_len(dx, dy, dz);
  for (int k = 0; k < 3; ++k) {
    s.a[k] = (float)a[k];
    s.b[k] = (float)b[k];
  }
  s.n[0] = (float)(nx / ln);
  s.n[1] = (float)(ny / ln);
  s.n[2] = (float)(nz / ln);
  s.t[0] = (float)(dx / ld);
  s.t[1] = (float)(dy / ld);
  s.t[2] = (float)(dz / ld);
  s.sinHalf = (float)(0.5 * ld);
  s.style = style;
  s.pad[0] = s.pad[1] = 0u;
}

// The edge pairs (first | second << 2) of the masks with one segment; 0 for masks 0, 5, 10 and 15
IRT_HD uint32_t ctr_pair(uint32_t mask) {
  // mask:                         0  1     2     3     4     5  6     7     8     9     10 11    12    13    14    15
  // first -> second:                 0>3   1>0   1>3   2>1      2>0   2>3   3>2   0>2      1>2   3>1   0>1   3>0
  const uint64_t table = (uint64_t)(0 | 3 << 2) << 4 | (uint64_t)(1 | 0 << 2) << 8 | (uint64_t)(1 | 3 << 2) << 12 |
                         (uint64_t)(2 | 1 << 2) << 16 | (uint64_t)(2 | 0 << 2) << 24 | (uint64_t)(2 | 3 << 2) << 28 |
                         (uint64_t)(3 | 2 << 2) << 32 | (uint64_t)(0 | 2 << 2) << 36 | (uint64_t)(1 | 2 << 2) << 44 |
                         (uint64_t)(3 | 1 << 2) << 48 | (uint64_t)(0 | 1 << 2) << 52 | (uint64_t)(3 | 0 << 2) << 56;
  return (uint32_t)(table >> (4u * mask)) & 15u;
}

// The cell's segments for threshold c.  Returns the kept segments as bits (1: the first candidate, 2:
// the second; a candidate whose end points are equal as floats is dropped) and, when EMIT, fills s0
// and s1 for the kept ones.  The count pass and the emit pass both run this, so they cannot disagree.
template <bool EMIT>
IRT_HD uint32_t ctr_eval(const ContourCell &K, float c, int32_t style, irt_overlay_segment &s0,
                         irt_overlay_segment &s1) {
  const uint32_t b0 = K.v[0] >= c, b1 = K.v[1] >= c, b2 = K.v[2] >= c, b3 = K.v[3] >= c;
  const uint32_t mask = b0 | b1 << 1 | b2 << 2 | b3 << 3;
  if (mask == 0u || mask == 15u) return 0u;
  // the crossed edges, each in its stated direction: e0 0 -> 1, e1 1 -> 2, e2 3 -> 2, e3 0 -> 3
  double E[4][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};
  if (b0 != b1) ctr_cross(K.p[0], K.p[1], K.v[0], K.v[1], c, E[0]);
  if (b1 != b2) ctr_cross(K.p[1], K.p[2], K.v[1], K.v[2], c, E[1]);
  if (b3 != b2) ctr_cross(K.p[3], K.p[2], K.v[3], K.v[2], c, E[2]);
  if (b0 != b3) ctr_cross(K.p[0], K.p[3], K.v[0], K.v[3], c, E[3]);
  uint32_t pair0, pair1 = 0u;
  bool two = false;
  if (mask == 5u || mask == 10u) {
    const float m = ((K.v[0] + K.v[1]) + (K.v[2] + K.v[3])) * 0.25f;
    const bool hi = m >= c;
    two = true;
    if (mask == 5u) {
      pair0 = hi ? (0 | 1 << 2) : (0 | 3 << 2);
      pair1 = hi ? (2 | 3 << 2) : (2 | 1 << 2);
    } else {
      pair0 = hi ? (1 | 2 << 2) : (1 | 0 << 2);
      pair1 = hi ? (3 | 0 << 2) : (3 | 2 << 2);
    }
  } else {
    pair0 = ctr_pair(mask);
  }
  uint32_t kept = 0u;
  double Pa[3], Pb[3];
  ctr_pick(E, (int)(pair0 & 3u), Pa);
  ctr_pick(E, (int)(pair0 >> 2), Pb);
  if (!ctr_same(Pa, Pb)) {
    kept |= 1u;
    if (EMIT) ctr_segment(Pa, Pb, style, s0);
  }
  if (two) {
    ctr_pick(E, (int)(pair1 & 3u), Pa);
    ctr_pick(E, (int)(pair1 >> 2), Pb);
    if (!ctr_same(Pa, Pb)) {
      kept |= 2u;
      if (EMIT) ctr_segment(Pa, Pb, style, s1);
    }
  }
  return kept;
}

// Host side (host/irt_contour.cpp).  The check irt_contour_cells and irt_contour_grid share: the
// grid, the thresholds, the styles and the flags (not the value arrays, the output or the count
// pointers); *cellsLon = the columns of cells
int contour_args(const char *what, const float *lat, int numLat, const float *lon, int numLon, const float *threshold,
                 const int32_t *style, int numThresholds, int flags, int *cellsLon);
// ... and the four tables: cos and sin of every lat and every lon, in double, from the host's glibc
void contour_trig(const float *lat, int numLat, const float *lon, int numLon, double *latC, double *latS,
                  double *lonC, double *lonS);

}  // namespace irt
