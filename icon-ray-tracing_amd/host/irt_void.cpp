// irt_void.cpp -- void packets, the pure part: which 8x8 packets of a launch can only ever render
// the zero colour (csrc/irt_launch.hip prepare_void caches and uploads the bitmap; k_render reads it).
//
// A packet is void when every ray the raygen can generate for its active pixels -- any jitter in
// [0, 1)^2, in any frame -- passes boxTest and fails intersectSphere on the shell's outer sphere
// (and so on the inner one): numRanges == 0, no sample, colour (0, 0, 0, 0)
// (deviceCode.cu:288-340).  That depends on the camera, the frame size, the box and the radii only.
//
// The certificate is computed in double and must hold for the FLOAT evaluation of generateRay,
// boxTest and intersectSphere, as the kernel and the reference run them.  u = 2^-24.
//
// 1. The direction.  generateRay evaluates d = (dir_00 + a dir_du) + b dir_dv with a = (x + .5f) +
//    ju, b = (y + .5f) + jv, each operation rounded: per component at most 8 u (|dir_00| + a |dir_du|
//    + b |dir_dv|) from the exact value for the exact (a, b) in the CLOSED rectangle [x + .5, x + 1.5]
//    x [y + .5, y + 1.5] (the rounding of a and b included, and a sum that rounds up to x + 1.5).
//    With M the sum of those magnitudes over the three components and dmin a lower bound of |d| over
//    the packet, that turns the direction by at most 8 u M / dmin.  normalize() rounds three
//    quotients (< 4 u more), and the clamp `fabsf(c) < 1e-5f -> c = 1e-5f` moves each component of
//    the unit vector by at most 2e-5: sqrt(3) 2e-5 < 3.5e-5.  So the ray the kernel tests deviates
//    from the exact direction of its (a, b) by at most
//        delta = 8 u M / dmin + 4e-5 rad,
//    and its length D satisfies |D - 1| < 1e-4.
//
// 2. The sphere.  For the float direction d' (length D) and eye O (length P), intersectSphere
//    computes disc = B B - 4 A C with A = d'.d', B = 2 d'.O, C = O.O - R R.  Exactly,
//    disc = 4 D^2 (R^2 - p^2), p the distance of the line from the centre = P sin(theta), theta the
//    angle between d' and -O.  The float errors: B/2 is off by <= 3.1 u D P, so B B by <= 29 u D^2
//    P^2; C by <= 5.1 u P^2 and A by 3.1 u D^2, so 4 A C by <= 37 u D^2 P^2; the last subtraction by
//    <= 8 u D^2 P^2: |error| <= 74 u D^2 P^2 < 4 D^2 P^2 eps with eps = 32 u = 2^-19.  The float
//    disc is negative -- the test fails, as required -- whenever
//        sin^2(theta) > (R / P)^2 + eps.
//    This first-order bound is used only while eps P^2 <= R^2 / 100 (P < 72 R; an eye farther away
//    classifies nothing) and for P > 1.001 R (an eye inside or on the sphere classifies nothing).
//    The directions that miss a sphere are not convex, so the packet is bounded by its centre
//    direction and the largest angle `ext` from it to a corner of its rectangle (the angle to a
//    fixed direction is quasi-convex on the image plane below 90 degrees, so its maximum over a
//    rectangle is at a corner): every tested ray has theta in [tc - ext - delta, tc + ext + delta],
//    sin^2 is smallest at the ends of an interval inside [0, pi], and both ends are checked -- on
//    cosines, with ext bounded from the image plane (sphere_rect: no inverse trigonometry).  Where
//    one cone around the whole rectangle is too coarse, the same test on each quarter of it
//    (recursively, to 64 pieces) covers the rectangle piece by piece.  A 64x64 tile is tried as
//    one rectangle first: most tiles lie wholly off the globe or wholly on it.
//    The inner sphere: r <= R makes its float C no smaller and its float disc no larger (every
//    operation is monotone under rounding), so it fails whenever the outer one does.
//
// 3. The box.  The directions from the eye that hit a convex body form a convex cone, so if the four
//    corner directions of the packet's rectangle hit the box shrunk by s on every side, every exact
//    direction of the packet passes through a point q of the shrunk box, at a distance of at most T
//    (the farthest box corner from the eye).  The tested ray, turned by at most delta, passes within
//    T delta of q: through a point at least c = s - T delta inside every face, so its exact slab
//    interval has t1 - t0 >= 2 c / D and t1 > 0.  boxTest's quotients (a correctly rounded
//    difference, a correctly rounded quotient; the clamp keeps every divisor nonzero) are each within
//    2.1 u of exact, signs kept, so the float test passes when 2 c / D > 2.2 * 2.1 u * T / D; c >= 3e-7 T
//    covers it.  Hence s = T (delta + 4e-7), and T < 1e9 keeps the ray's tmax = 1e10 out of it.
//
//
// 4. Interior packets (the second bitmap): every ray of the packet's active pixels, whatever the
//    jitter, passes boxTest, hits both spheres in front of the eye, takes the front-and-back case
//    of the raygen's range selection (t0 < st2 and !(st4 < t0), t0 the float box entry, st2 the
//    inner sphere's near hit, st4 the outer one's far hit) and keeps every divisor of
//    intersect_spheres inside recip_ok's range.  k_render then leaves the box test, the d < 0 exits,
//    the range selection and the fallback divisions out (irt_raygen.h).  For one rectangle, with
//    tc, x0, delta and x = x0 + delta as in section 2 (sphere_rect) and r the inner radius:
//    (a) the box: section 3, unchanged (in_box with the rectangle's delta).
//    (b) the discriminant.  cl = cos(tc)(1 - x^2/2) - sin(tc) x <= cos(tc + x) must be positive
//        (every tested ray points at the globe's side: B < 0); theta <= tc + x < 90 degrees then
//        gives sin^2(theta) <= sm = 1 - cl^2.  The exact disc / (4 D^2)
//        is then at least g = r^2 - P^2 sm, the float one is off by at most eps P^2 (section 2, the
//        same operations with r for R), so it is >= 0 when g >= eps P^2; the certificate asks
//        g >= 4 eps P^2, i.e. rho = eps P^2 / g <= 1/4.  The outer sphere: R >= r makes its float C no
//        larger and its float disc no smaller (every operation monotone under rounding), so it hits
//        whenever the inner one does -- the mirror of section 2's last paragraph.
//    (c) the ranges.  With B < 0, q = -0.5 (B - d) = (|B| + d) / 2 has no cancellation.  Relative
//        errors: |B| / 2 = D P cos(theta) by 3.1 u / cos(theta) <= 3.1 u / cl; d = sqrtf(disc) by rho
//        (sqrt halves the disc's, the bound keeps it whole), and d <= 2 D R against |B| >= 2 D P cl,
//        so q by eq = 3.1 u / cl + rho R / (P cl) + 2 u; C = O.O - r r by eC = 5.1 u P^2 / (P^2 - R^2)
//        (the outer sphere's, the larger); a quotient through recip_d or the division by u.  Hence
//        st2 = fminf(q / A, C / q) >= (1 - err) s / D and st4 >= q_R / A >= (1 - err) (the outer far
//        root) >= (1 - err) s / D, with s the Euclidean distance to the inner sphere's near hit
//        along the tested ray, D its length and err = eq + eC + 8 u.
//        The box entry t0 = fmaxf(0, the three near slab quotients), each within 2.1 u of exact
//        (section 3).  Per axis k: an eye inside the slab [lo_k, hi_k] has a near quotient <= 0.  An
//        eye above it (o_k > hi_k; below: mirrored) and a ray pointing away: negative again.
//        Pointing at it: the quotient is e_k / D, e_k = (o_k - hi_k) / |w_k| for the ray's unit
//        direction w.  Where the slab's side clears the inner sphere, hi_k > r: the near hit X = O +
//        s w has X_k <= r, so s |w_k| >= o_k - r and s >= e_k (1 + m_k), m_k = (hi_k - r) / (o_k -
//        hi_k) -- for the very ray tested, no cone around it; t0 < st2 then follows from
//        (1 + 3 u) < (1 + m_k)(1 - err).  Where it does not (a lat/lon-filtered grid's box need not
//        contain the sphere), the rectangle's own bounds: |w_k| >= wk = min |c_k| / max |c| - delta
//        over the four corner directions c (c_k is affine and |c| convex over the rectangle; all
//        four c_k must point at the slab, or all away from it by more than delta |c|), and s >=
//        s(cu) = P cu - sqrt(r^2 - P^2 (1 - cu^2)), decreasing in cos(theta) <= cu = min(1, cos(tc) +
//        sin(tc) x): (o_k - hi_k) / wk (1 + 3 u) < (1 - err) s(cu).  D cancels throughout.
//        !(st4 < t0) follows from t0 < (1 - err) s / D <= st4.
//    (d) recip_ok: len = |d| before normalize is within 8 u M of [dmin, max |c|], both asked inside
//        [1e-30, 1e30]; A = D^2 is within 3e-4 of 1; q lies in D P cl (1 - eq) .. D (P + R)(1 + eq),
//        and P < 1e12, P cl > 1e-20 keep that inside 2^-100 .. 2^100 with room to spare.
//    A packet the certificate does not cover is simply not interior: no quartering.  Tiles first.
//
// A camera any of this cannot cover (non-finite words, du/dv that let |d| vanish over a packet, a
// box thinner than 2 s) classifies nothing.

#include <math.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "irt_internal.h"

namespace irt {

namespace {

struct V3 {
  double x, y, z;
};
V3 operator+(V3 a, V3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
V3 operator*(double s, V3 a) { return {s * a.x, s * a.y, s * a.z}; }
double dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
double norm(V3 a) { return sqrt(dot(a, a)); }
double abs1(V3 a) { return fabs(a.x) + fabs(a.y) + fabs(a.z); }

// the exact slab test of the ray org + t d, t > 0, against [lo, hi]
bool hits_box(V3 org, V3 d, const double lo[3], const double hi[3]) {
  const double o[3] = {org.x, org.y, org.z}, dd[3] = {d.x, d.y, d.z};
  double t0 = 0.0, t1 = INFINITY;
  for (int k = 0; k < 3; ++k) {
    if (dd[k] == 0.0) {
      if (!(o[k] > lo[k] && o[k] < hi[k])) return false;
      continue;
    }
    const double a = (lo[k] - o[k]) / dd[k], b = (hi[k] - o[k]) / dd[k];
    t0 = std::max(t0, std::min(a, b));
    t1 = std::min(t1, std::max(a, b));
  }
  return t0 < t1;
}

// The camera and what the sphere test needs of it, once per request
struct View {
  V3 org, d00, du, dv, axis;
  double uu, vv, uv;     // du.du, dv.dv, |du.dv|
  double m0, mu, mv;     // the 1-norms of d00, du, dv (M of the head's section 1)
  double cosN, sinN;     // of `need`, the angle every tested ray must keep from the axis
  V3 dir(double a, double b) const { return d00 + a * du + b * dv; }
};
struct Rect {
  double a0, a1, b0, b1;  // screen coordinates, closed
};
enum { kUnbounded = -2, kCentreHits = -1, kUndecided = 0, kClear = 1, kAllHit = 2 };

// One rectangle against the sphere, without inverse trigonometry.  c its centre direction, h the
// largest image-plane distance from the centre to a corner, dmin = |c| - h <= |d| over it: every
// exact direction is within x0 = 1.01 h / dmin of c (sin(angle) <= h / dmin < 0.2, and asin(t) <
// 1.01 t there), every tested ray within x = x0 + delta.  With ct = cos(angle of c to the axis):
//   theta_c - x > need        <=  ct < cos(need + x),  and cos(need + x) >= cosN (1 - x^2/2) - sinN x;
//   theta_c + x < pi - need   <=  ct > -cos(need + x);
//   every exact direction hits (theta_c + x0 < need: nothing to flag)  <=  ct > cosN + sinN x0.
// delta: the rectangle's own (section 1).
int sphere_rect(const View &v, const Rect &r, double &delta) {
  const double ha = 0.5 * (r.a1 - r.a0), hb = 0.5 * (r.b1 - r.b0);
  const V3 c = v.dir(r.a0 + ha, r.b0 + hb);
  const double lc = norm(c), h = sqrt(ha * ha * v.uu + hb * hb * v.vv + 2.0 * ha * hb * v.uv), dmin = lc - h;
  if (!(lc > 0.0) || !(h < 0.16 * lc)) return kUnbounded;  // h / dmin < 0.2
  delta = 8.0 * ldexp(1.0, -24) * (v.m0 + r.a1 * v.mu + r.b1 * v.mv) / dmin + 4e-5;
  const double ct = dot(c, v.axis) / lc, x0 = 1.01 * h / dmin, x = x0 + delta + 1e-9;
  if (ct > v.cosN + v.sinN * x0) return kAllHit;
  if (!(ct < v.cosN)) return kCentreHits;
  const double L = v.cosN * (1.0 - 0.5 * x * x) - v.sinN * x;
  return ct < L && ct > -L ? kClear : kUndecided;
}
// ... and, where one cone around the whole rectangle is too coarse (small frames: a packet spans
// degrees), each of its quarters, down to 64 pieces; a piece whose centre ray hits settles it
bool sphere_clear(const View &v, const Rect &r, int depth) {
  double delta;
  const int res = sphere_rect(v, r, delta);
  if (res != kUndecided || depth == 3) return res == kClear;
  const double am = 0.5 * (r.a0 + r.a1), bm = 0.5 * (r.b0 + r.b1);
  return sphere_clear(v, {r.a0, am, r.b0, bm}, depth + 1) && sphere_clear(v, {am, r.a1, r.b0, bm}, depth + 1) &&
         sphere_clear(v, {r.a0, am, bm, r.b1}, depth + 1) && sphere_clear(v, {am, r.a1, bm, r.b1}, depth + 1);
}

// What section 4 needs of the scene, once per request
struct Shell {
  double P, r, R, eps;
  double o[3], lo[3], hi[3];
};
// One rectangle against section 4 (b), (c), (d); delta: the rectangle's own, for the box test (a)
bool interior_rect(const View &v, const Shell &g, const Rect &r, double &delta) {
  const double u = ldexp(1.0, -24);
  const double ha = 0.5 * (r.a1 - r.a0), hb = 0.5 * (r.b1 - r.b0);
  const V3 c = v.dir(r.a0 + ha, r.b0 + hb);
  const double lc = norm(c), h = sqrt(ha * ha * v.uu + hb * hb * v.vv + 2.0 * ha * hb * v.uv), dmin = lc - h;
  if (!(lc > 0.0) || !(h < 0.16 * lc)) return false;
  delta = 8.0 * u * (v.m0 + r.a1 * v.mu + r.b1 * v.mv) / dmin + 4e-5;
  const double ct = dot(c, v.axis) / lc, x = 1.01 * h / dmin + delta + 1e-9;
  if (!(ct > 0.0) || !(ct <= 1.0)) return false;
  const double st = sqrt(std::max(0.0, 1.0 - ct * ct));
  const double cl = ct * (1.0 - 0.5 * x * x) - st * x;  // <= cos(theta) of every tested ray
  if (!(cl > 0.0)) return false;
  // (b)
  const double P2 = g.P * g.P, gg = g.r * g.r - P2 * (1.0 - cl * cl);
  if (!(gg >= 4.0 * g.eps * P2)) return false;
  const double rho = g.eps * P2 / gg;
  // (c)
  const double eq = 3.1 * u / cl + rho * g.R / (g.P * cl) + 2.0 * u;
  const double eC = 5.1 * u * P2 / (P2 - g.R * g.R);
  const double err = eq + eC + 8.0 * u;
  if (!(err < 0.5)) return false;
  const V3 cn[4] = {v.dir(r.a0, r.b0), v.dir(r.a1, r.b0), v.dir(r.a0, r.b1), v.dir(r.a1, r.b1)};
  double cmax = 0.0;
  for (const V3 &q : cn) cmax = std::max(cmax, norm(q));
  const double cu = std::min(1.0, ct + st * x);
  const double sLow = g.P * cu - sqrt(std::max(0.0, g.r * g.r - P2 * (1.0 - cu * cu)));  // <= s of every tested ray
  for (int k = 0; k < 3; ++k) {
    const bool above = g.o[k] > g.hi[k], below = g.o[k] < g.lo[k];
    if (!above && !below) continue;  // inside the slab: a near quotient <= 0
    const double gap = above ? g.o[k] - g.hi[k] : g.lo[k] - g.o[k];  // > 0
    const double side = above ? g.hi[k] : -g.lo[k];                  // the slab's side towards the eye, from the centre
    if (side > g.r) {
      const double m = (side - g.r) / gap;
      if ((1.0 + m) * (1.0 - err) > 1.0 + 4.0 * u) continue;
    }
    // the rectangle's own bounds
    double kmin = INFINITY, kaway = INFINITY;
    for (const V3 &q : cn) {
      const double ck = k == 0 ? q.x : k == 1 ? q.y : q.z, toward = above ? -ck : ck;  // > 0: pointing at the slab
      kmin = std::min(kmin, toward);
      kaway = std::min(kaway, -toward);
    }
    if (kaway > delta * cmax * 1.0001 + 2e-5 * cmax) continue;  // every tested ray points away (the clamp: 2e-5)
    const double wk = kmin / cmax - delta;
    if (!(wk > 0.0) || !(gap / wk * (1.0 + 4.0 * u) < (1.0 - err) * sLow)) return false;
  }
  // (d)
  if (!(dmin > 1e-30) || !(cmax < 1e30) || !(g.P < 1e12) || !(g.P * cl > 1e-20)) return false;
  return true;
}

}  // namespace

uint32_t void_packets(const VoidRequest &q, uint32_t *bits, VoidLists *lists, uint32_t *interior,
                      uint32_t *numInterior) {
  memset(bits, 0, void_words(q.numTiles) * sizeof(uint32_t));
  if (interior) memset(interior, 0, void_words(q.numTiles) * sizeof(uint32_t));
  if (numInterior) *numInterior = 0;
  if (lists) *lists = VoidLists();
  // only the raygen this certificate describes: woodcockTrackingWithAccel over the shell's spheres
  if (q.raygen != IRT_RAYGEN_WITH_ACCEL || q.accelMode != IRT_ACCEL_SPHERE || q.mode != IRT_MODE_USER_GEOM) return 0;
  if (q.W <= 0 || q.H <= 0 || q.tileStride <= 0 || q.tileBegin < 0) return 0;
  for (int k = 0; k < 12; ++k)
    if (!std::isfinite(q.cam[k])) return 0;
  for (int k = 0; k < 3; ++k)
    if (!std::isfinite(q.bmin[k]) || !std::isfinite(q.bmax[k])) return 0;
  const double R = q.rOuter, r = q.rInner;
  if (!std::isfinite(R) || !std::isfinite(r) || !(r >= 0.0) || !(R >= r) || !(R > 0.0)) return 0;
  const V3 org = {q.cam[0], q.cam[1], q.cam[2]}, d00 = {q.cam[3], q.cam[4], q.cam[5]},
           du = {q.cam[6], q.cam[7], q.cam[8]}, dv = {q.cam[9], q.cam[10], q.cam[11]};
  const double eps = ldexp(1.0, -19);
  const double P = norm(org);
  if (!(P > 1.001 * R) || !(eps * P * P <= 0.01 * R * R)) return 0;  // eye inside, or too far away
  const double need = asin(sqrt((R / P) * (R / P) + eps));            // theta must clear this
  const V3 axis = (-1.0 / P) * org;
  // T: the farthest box corner from the eye
  double T = 0.0;
  for (int k = 0; k < 8; ++k) {
    const V3 cnr = {(k & 1) ? q.bmax[0] : q.bmin[0], (k & 2) ? q.bmax[1] : q.bmin[1], (k & 4) ? q.bmax[2] : q.bmin[2]};
    T = std::max(T, norm(cnr + (-1.0) * org));
  }
  if (!(T < 1e9)) return 0;
  const View v = {org, d00, du, dv, axis, dot(du, du), dot(dv, dv), fabs(dot(du, dv)), abs1(d00), abs1(du), abs1(dv),
                  cos(need), sin(need)};
  const int tilesX = (q.W + 63) / 64, total = tilesX * ((q.H + 63) / 64);
  // interior packets (section 4) need a real inner sphere
  const bool wantInterior = interior != nullptr && r > 0.0;
  const Shell shell = {P, r, R, eps, {org.x, org.y, org.z}, {q.bmin[0], q.bmin[1], q.bmin[2]}, {q.bmax[0], q.bmax[1], q.bmax[2]}};
  uint32_t count = 0, countInterior = 0;
  // the work items, gathered in this pass: the live packets per residue of their block (mod 8), in
  // block then wave order, and the void ones
  std::vector<uint32_t> res[8], voids;
  auto in_box = [&](double a0, double a1, double b0, double b1, double delta) {
    const double s = T * (delta + 4e-7);
    double blo[3], bhi[3];
    for (int j = 0; j < 3; ++j) {
      blo[j] = (double)q.bmin[j] + s;
      bhi[j] = (double)q.bmax[j] - s;
      if (!(blo[j] < bhi[j])) return false;
    }
    return hits_box(org, v.dir(a0, b0), blo, bhi) && hits_box(org, v.dir(a1, b0), blo, bhi) &&
           hits_box(org, v.dir(a0, b1), blo, bhi) && hits_box(org, v.dir(a1, b1), blo, bhi);
  };
  for (int k = 0; k < q.numTiles; ++k) {
    const int tileId = q.tileList ? q.tileList[k] : q.tileBegin + k * q.tileStride;
    if (tileId < 0 || tileId >= total) continue;  // (no launch has such a tile)
    const int tx0 = (tileId % tilesX) * 64, ty0 = (tileId / tilesX) * 64;
    // the tile as one rectangle first (its active pixels): most tiles lie wholly off the globe or
    // wholly on it, and are settled by one test
    double delta = 0.0;
    const Rect tile = {tx0 + 0.5, std::min(tx0 + 64, q.W) + 0.5, ty0 + 0.5, std::min(ty0 + 64, q.H) + 0.5};
    const int whole = sphere_rect(v, tile, delta);
    if (whole == kAllHit && !lists && !wantInterior) continue;
    double tdelta = 0.0;
    const bool tileInterior = wantInterior && (whole == kAllHit || whole == kCentreHits) &&
                              interior_rect(v, shell, tile, tdelta) && in_box(tile.a0, tile.a1, tile.b0, tile.b1, tdelta);
    const bool tileVoid = whole == kClear && in_box(tile.a0, tile.a1, tile.b0, tile.b1, delta);
    for (int j = 0; j < 64; ++j) {
      const size_t p = (size_t)k * 64 + j;
      const int sub = j >> 2, wave = j & 3;  // pixel_of (irt_raygen.h)
      const int x0 = tx0 + (((sub & 3) << 4) | ((wave & 1) << 3)), y0 = ty0 + (((sub >> 2) << 4) | ((wave >> 1) << 3));
      if (x0 >= q.W || y0 >= q.H) continue;  // no active pixel: nothing to merge, and no work item
      bool isVoid = tileVoid;
      if (!tileVoid && whole != kAllHit && !tileInterior) {
        // one past the last active pixel
        const Rect r = {x0 + 0.5, std::min(x0 + 8, q.W) + 0.5, y0 + 0.5, std::min(y0 + 8, q.H) + 0.5};
        double pd = 0.0;  // (pd: the packet's own delta, for the box)
        isVoid = !(sphere_rect(v, r, pd) < 0 || pd == 0.0) && sphere_clear(v, r, 0) && in_box(r.a0, r.a1, r.b0, r.b1, pd);
      }
      if (!isVoid) {
        if (lists) res[(p >> 2) & 7].push_back((uint32_t)p);
        bool isInterior = tileInterior;
        if (wantInterior && !tileInterior && !tileVoid) {
          const Rect r = {x0 + 0.5, std::min(x0 + 8, q.W) + 0.5, y0 + 0.5, std::min(y0 + 8, q.H) + 0.5};
          double pd = 0.0;
          isInterior = interior_rect(v, shell, r, pd) && in_box(r.a0, r.a1, r.b0, r.b1, pd);
        }
        if (isInterior) {
          interior[p >> 5] |= 1u << (p & 31);
          ++countInterior;
        }
        continue;
      }
      bits[p >> 5] |= 1u << (p & 31);
      if (lists) voids.push_back((uint32_t)p);
      ++count;
    }
  }
  if (lists && count) {
    // residue x's k-th packet at index 8 k + x; every residue padded to the longest
    size_t len = 0;
    for (const auto &r : res) len = std::max(len, r.size());
    lists->live = (uint32_t)(8 * len);
    lists->count = count;
    lists->items.assign(8 * len + voids.size(), kVoidEmpty);
    for (size_t x = 0; x < 8; ++x)
      for (size_t k = 0; k < res[x].size(); ++k) lists->items[8 * k + x] = res[x][k];
    std::copy(voids.begin(), voids.end(), lists->items.begin() + 8 * len);
  }
  if (numInterior) *numInterior = countInterior;
  return count;
}

// The cache: one bitmap, kept while the request's key -- everything void_packets reads, the tile
// list by content -- stays what it was (a progressive sequence computes it once).  With `defer`, a
// new key is only noted, and the bitmap computed when the same request comes a second time: a
// camera that gets one launch never pays for a bitmap no later launch would use.
bool VoidCache::lookup(const VoidRequest &q, bool defer) {
  std::vector<unsigned char> k(sizeof(VoidRequest) + (q.tileList ? (size_t)std::max(q.numTiles, 0) * sizeof(int32_t) : 0));
  VoidRequest flat = q;
  flat.tileList = q.tileList ? reinterpret_cast<const int32_t *>(1) : nullptr;  // a list by content, not by address
  memcpy(k.data(), &flat, sizeof(flat));
  if (q.tileList && q.numTiles > 0) memcpy(k.data() + sizeof(flat), q.tileList, (size_t)q.numTiles * sizeof(int32_t));
  const bool same = keyed && k == key;
  if (same && valid) return false;
  if (!same) {
    key.swap(k);
    keyed = true;
    valid = false;
    count = 0;
    interiorCount = 0;
    if (defer) return false;
  }
  bits.assign(void_words(q.numTiles), 0u);
  interior.assign(void_words(q.numTiles), 0u);
  count = void_packets(q, bits.data(), &lists, interior.data(), &interiorCount);
  valid = true;
  ++generation;
  return true;
}

}  // namespace irt
