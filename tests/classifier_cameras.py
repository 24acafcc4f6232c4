"""The camera battery of the packet-classifier sweep, and the float32 restatement both its host and
its device tests share (test_classifier_sweep_cpu.py, test_gpu_classifier_sweep.py; the restatement
also serves test_interior_cpu.py).

The restatement: generateRay, boxTest and intersectSphere in float32, operation for operation as
oracle/icon_oracle.cpp evaluates them -- what the kernel and the reference actually compute, and
what host/irt_void.cpp certifies in double.

Scenes: synth_grid(2, 2, 10) flat, over terrain, and a lat/lon window of the flat grid whose box
sides lie inside the inner sphere.  The same records serve the host and the device tests.

Cameras: the eye at distance P from the centre, R the scene's outer radius, looking at the centre
unless stated; fovy = 2 asin(R / P) / span.  How the construction was chosen, from the float64
census alone (the sweep asks that three quarters of the admitted cameras hold 8 census packets of
each class at 96x72):
- span is 1 (the disc spans the frame's height), not 0.7.  A void packet must pass the box, and the
  flat grid's box is the cube around the globe: from afar its silhouette leaves a ring of 0.004 to
  0.41 R around the disc.  At span 0.7 the disc's radius is 25 px at 96x72 and the ring is narrower
  than an 8x8 packet almost everywhere (census: 6 or 7 void packets from 3 R to 72 R, 0 along an
  axis); at span 1 the frame's corners add whole packets (census: 8 to 11).
- the rule's angle passes 180 degrees below P = 1.27 R.  An eye whose rule gives more than
  FOVY_MAX looks at the horizon instead (the outer sphere's tangent point in the up-vector's
  plane), with fovy 60, or 20 for the eyes at 1.001 R: there the rays that miss the sphere's LINE
  (disc < 0: what the void class is about) lie within 2.7 degrees of the horizon, and the inner
  sphere's limb 6.4 degrees under it.
- the axis-aligned eyes stand at 2 R, where perspective opens the cube's silhouette.
- seeded random cameras: span uniform in [0.8, 1.2] (a larger disc leaves no sky in the frame, a
  smaller one no whole packet in the ring), the look-at point 0.4 to 0.8 R from the centre ACROSS
  the view axis, so it moves the limb in the frame; fovy capped at FOVY_MAX.  SEED was written
  down before the first census was run and has not been changed since; only the rules above were.
  The condition holds with nothing to spare (30 of 39).
- the margin probes (PROBES) stand beside the battery: see there.

The float64 census (no margin): which packets a perfect classifier could flag at all, as the
reference for "there was something to find".

Section 4(c)'s branch for an eye outside a slab whose rays all point away from it cannot carry a
flag: such a ray never enters the slab, so the packet fails the box test first.  No camera reaches
it; WINDOW_EYE_2 covers the mirrored (eye below the slab) side of the rectangle's own bounds instead.
"""
import functools
import math

import numpy as np

import irt
import oracle as O
from helpers import FRAMING  # noqa: F401  (re-exported for the sweeps)

F = np.float32
ONE_BELOW = float(np.nextafter(F(1), F(0)))
EPS = 2.0 ** -19  # host/irt_void.cpp section 2

SIZES = ((96, 72), (64, 64), (203, 71), (67, 33))
SCENES = ("flat", "terrain", "window")
FOVY_MAX = 90.0
NEAR_FOVY = 60.0
SEED = 20250131
NUM_RANDOM = 24


# ------------------------------------------------------------------------------------ the scenes
@functools.lru_cache(maxsize=None)
def cells(scene):
    c = irt.synth_grid(2, 2, 10, terrain=4000.0 if scene == "terrain" else 0.0)
    if scene == "window":  # test_interior_cpu._info(True)'s window: its box does not contain the sphere
        c = c[(c["lat"].min(1) > 0.2) & (c["lat"].max(1) < 1.0) & (c["lon"].min(1) > -0.5) & (c["lon"].max(1) < 0.6)]
        assert len(c) > 0
        c = np.ascontiguousarray(c)
    c.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def info(scene):
    return irt.volume_info(cells(scene))


def radii(scene):
    sb = info(scene).sphericalBounds
    return float(sb.lower.x), float(sb.upper.x)


# ------------------------------------------------------------------------- the float32 restatement
def _packet_rects(W, H):
    """Per packet of a whole-frame launch (4 * block + wave): x0, y0, x1, y1 of its active pixels
    (x1, y1 one past the last; x0 >= W or y0 >= H: none), as irt_raygen.h pixel_of maps them."""
    tx, ty = (W + 63) // 64, (H + 63) // 64
    p = np.arange(tx * ty * 64)
    blk, wave = p >> 2, p & 3
    k, sub = blk >> 4, blk & 15
    x0 = (k % tx) * 64 + ((sub & 3) << 4) + ((wave & 1) << 3)
    y0 = (k // tx) * 64 + ((sub >> 2) << 4) + ((wave >> 1) << 3)
    return x0, y0, np.minimum(x0 + 8, W), np.minimum(y0 + 8, H)


def _dot(a, b):  # vecmath.h:536-538 order
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _rays32(cam, xs, ys, ju, jv):
    """generateRay in float32: (raw length, clamped unit direction)."""
    d00, du, dv = cam[3:6], cam[6:9], cam[9:12]
    a = (xs.astype(F) + F(0.5)) + ju.astype(F)
    b = (ys.astype(F) + F(0.5)) + jv.astype(F)
    d = np.stack([(d00[k] + a * du[k]) + b * dv[k] for k in range(3)], -1)
    ln = np.sqrt(_dot(d, d))
    d = d / ln[..., None]
    d = np.where(np.abs(d) < F(1e-5), F(1e-5), d)
    assert d.dtype == F
    return ln, d


def _box32(org, d, lo, hi):
    tl, th = (lo - org) / d, (hi - org) / d
    nr, fr = np.minimum(tl, th), np.maximum(tl, th)
    t0 = np.maximum(F(0), np.maximum(np.maximum(nr[..., 0], nr[..., 1]), nr[..., 2]))
    t1 = np.minimum(F(1e10), np.minimum(np.minimum(fr[..., 0], fr[..., 1]), fr[..., 2]))
    return t0 < t1, t0, t1


def _sphere32(org, d, radius):
    """intersectSphere: (disc, A, q, tnear, tfar); q and the roots are NaN where disc < 0."""
    A = _dot(d, d)
    B = _dot(d, np.broadcast_to(org, d.shape)) * F(2)
    Cc = _dot(org, org) - F(radius) * F(radius)
    disc = B * B - F(4) * A * Cc
    with np.errstate(invalid="ignore", divide="ignore"):
        s = np.sqrt(disc)
        q = np.where(B < 0, F(-0.5) * (B - s), F(-0.5) * (B + s))
        t1, t2 = q / A, Cc / q
    return disc, A, q, np.minimum(t1, t2), np.maximum(t1, t2)


def _recip_ok(v):
    a = np.abs(v)
    return (a >= F(2.0 ** -100)) & (a <= F(2.0 ** 100))


def _lcg_jitters(aid, W, H, xs, ys):
    L = O.olib()
    two = np.zeros(2, F)
    ju, jv = np.zeros(xs.shape, F), np.zeros(xs.shape, F)
    for i, (x, y) in enumerate(zip(xs.ravel(), ys.ravel())):
        L.oracle_lcg((aid * W * H + int(x)) & 0xFFFFFFFF, int(y), 2, two.ctypes.data)
        jv.ravel()[i], ju.ravel()[i] = two  # the dir_dv jitter is drawn first
    return ju, jv


def _void32(org, d, lo, hi, r_in, r_out):
    """The void twin: boxTest passes and the float32 disc of the outer sphere is < 0, and the inner
    one's; returns (ok per ray, the outer disc, A)."""
    hit, _, _ = _box32(org, d, lo, hi)
    disc_o, A, _, _, _ = _sphere32(org, d, r_out)
    disc_i, _, _, _, _ = _sphere32(org, d, r_in)
    return hit & (disc_o < 0) & (disc_i < 0), disc_o, A


def fixed_jitters():
    """(69, 2) float32: the four corners of [0, 1)^2 with the largest float below 1, the centre (an
    axis-aligned view's middle rays then have components that are exactly 0 before the clamp), and
    64 seeded jitters."""
    rng = np.random.default_rng(20240611)
    sj = np.minimum(rng.random((64, 2)).astype(F), F(ONE_BELOW))
    corners = np.array([(0, 0), (0, ONE_BELOW), (ONE_BELOW, 0), (ONE_BELOW, ONE_BELOW), (0.5, 0.5)], F)
    return np.concatenate([corners, sj])


def packet_pixels(W, H, flagged):
    """The active pixels of the flagged packets: (xs, ys, packet index of each)."""
    x0, y0, x1, y1 = _packet_rects(W, H)
    xs, ys, ps = [], [], []
    for p in np.nonzero(flagged)[0]:
        Y, X = np.mgrid[y0[p]:y1[p], x0[p]:x1[p]]
        xs.append(X.ravel())
        ys.append(Y.ravel())
        ps.append(np.full(X.size, p))
    if not xs:
        z = np.zeros(0, np.int64)
        return z, z, z
    return np.concatenate(xs), np.concatenate(ys), np.concatenate(ps)


def jitters_for(W, H, xs, ys, lcg_ids=()):
    """(ju, jv), each (pixels, J): the fixed set for every pixel, then the LCG's own jitters of the
    given accumIDs."""
    fx = fixed_jitters()
    ju = [np.broadcast_to(fx[:, 0], (len(xs), len(fx)))]
    jv = [np.broadcast_to(fx[:, 1], (len(xs), len(fx)))]
    for aid in lcg_ids:
        a, b = _lcg_jitters(aid, W, H, xs, ys)
        ju.append(a[:, None])
        jv.append(b[:, None])
    return np.concatenate(ju, 1), np.concatenate(jv, 1)


def box32(inf):
    return np.array(inf.bounds.lower.tolist(), F), np.array(inf.bounds.upper.tolist(), F)


# ------------------------------------------------------------------------------------ the cameras
def _unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v)


OFF_AXIS = _unit((0.3, 0.5, -0.8))  # helpers.view_battery's southern direction, off every axis
DIAGONAL = _unit((1.0, 1.0, 1.0))


def _up(view, roll_deg):
    """A unit vector across `view` (from the coordinate axis farthest from it), rolled about it."""
    w = _unit(view)
    e = np.eye(3)[int(np.argmin(np.abs(w)))]
    u0 = _unit(e - (e @ w) * w)
    a = math.radians(roll_deg)
    return math.cos(a) * u0 + math.sin(a) * np.cross(w, u0)


def _tuple(vp, vi, vu, fovy):
    return (tuple(float(x) for x in vp), tuple(float(x) for x in vi), tuple(float(x) for x in vu), float(fovy))


def globe_camera(R, ratio, direction, look=(0.0, 0.0, 0.0), roll=0.0, span=1.0, up=None, keep_look=False,
                 near_fovy=NEAR_FOVY):
    """(vp, vi, vu, fovy) for an eye at ratio * R along `direction`; `look` in units of R."""
    P = ratio * R
    eye = P * _unit(direction)
    vi = R * np.asarray(look, np.float64)
    fovy = math.degrees(2.0 * math.asin(min(1.0, R / P)) / span) if P > R else 2.0 * FOVY_MAX
    vu = _up(vi - eye, roll) if up is None else np.asarray(up, np.float64)
    if fovy > FOVY_MAX:
        if keep_look:
            fovy = FOVY_MAX
        else:  # look at the horizon: the tangent point of the outer sphere, in the plane of eye and vu
            n = -_unit(eye)
            t = _unit(vu - (vu @ n) * n)
            s = min(1.0, R / P)
            vi = eye + R * (math.sqrt(max(0.0, 1.0 - s * s)) * n + s * t)
            vu, fovy = -n, near_fovy
    return _tuple(eye, vi, vu, fovy)


WINDOW_EYE = ((1.2e7, 1.0e6, 9.0e6), (4.6e6, 2.0e5, 3.6e6), (0.0, 0.0, 1.0), 35.0)
# beyond the window box's other y side and under its z slab (the mirrored, eye-below branch of
# section 4(c)); it is still above the x slab, as every eye that sees the window from outside is
WINDOW_EYE_2 = ((1.15e7, 6.5e6, 5.0e5), (4.6e6, 2.0e5, 3.6e6), (0.0, 0.0, 1.0), 35.0)

# name -> (scenes it runs on, keyword arguments of globe_camera or a literal camera, refuses)
_GLOBE = ("flat", "terrain", "window")
NAMED = {
    "P1.0011": (_GLOBE, dict(ratio=1.0011, direction=OFF_AXIS, near_fovy=20.0), False),
    "P1.0009": (_GLOBE, dict(ratio=1.0009, direction=OFF_AXIS, near_fovy=20.0), True),
    "P1.05": (_GLOBE, dict(ratio=1.05, direction=OFF_AXIS), False),
    "P3": (_GLOBE, dict(ratio=3.0, direction=OFF_AXIS), False),
    "P20": (_GLOBE, dict(ratio=20.0, direction=OFF_AXIS), False),
    "P60": (_GLOBE, dict(ratio=60.0, direction=OFF_AXIS), False),
    "P71.5": (_GLOBE, dict(ratio=71.5, direction=OFF_AXIS), False),
    "P72.5": (_GLOBE, dict(ratio=72.5, direction=OFF_AXIS), True),
    # the centre rays' x and y (y and z) fall under the 1e-5 clamp; P = 2 R, where the cube's
    # silhouette leaves room for void packets around the disc
    "axis+z": (_GLOBE, dict(ratio=2.0, direction=(0.0, 0.0, 1.0), up=(0.0, 1.0, 0.0)), False),
    "axis-x": (_GLOBE, dict(ratio=2.0, direction=(-1.0, 0.0, 0.0), up=(0.0, 0.0, 1.0)), False),
    "diagonal": (_GLOBE, dict(ratio=3.0, direction=DIAGONAL), False),
    "look0.8": (_GLOBE, dict(ratio=3.0, direction=OFF_AXIS, look=(0.64, -0.48, 0.0)), False),
    "look0.5far": (_GLOBE, dict(ratio=20.0, direction=DIAGONAL, look=(0.0, 0.3, -0.4)), False),
    "roll30": (_GLOBE, dict(ratio=20.0, direction=OFF_AXIS, roll=30.0), False),
    "roll30look": (_GLOBE, dict(ratio=3.0, direction=DIAGONAL, look=(0.4, 0.0, -0.5), roll=30.0), False),
    "window": (("window",), WINDOW_EYE, False),
    "window2": (("window",), WINDOW_EYE_2, False),
}


def limb_probe(rho, ratio, side, offset, pixel):
    """A camera looking along -z (du along x, dv along y) from ratio * rho away, whose ray (0, 0, -1)
    -- the column where the x component of the direction passes through zero -- runs `offset` rad
    outside the limb of the sphere of radius rho (negative: inside), the globe on the +x side of
    that column for side = +1 and on the -x side for -1.  `pixel`: a pixel's angle at 72 rows.
    The 1e-5 clamp lifts every |x| < 1e-5 to +1e-5: towards the globe for side = +1, away from it
    for -1."""
    P = ratio * rho
    a = math.asin(1.0 / ratio) + offset
    eye = np.array((-side * P * math.sin(a), 0.0, P * math.cos(a)))
    return _tuple(eye, eye + np.array((0.0, 0.0, -1.0e6)), (0.0, 1.0, 0.0), math.degrees(72.0 * pixel))


# The margin probes: narrow frames (3e-6 rad per pixel at 72 rows) on a limb, each aimed at one
# hand-derived margin that no camera of the fovy rule can come near, because a flagged packet's
# cone keeps its rectangle some tenths of a pixel off the limb.  By construction a probe holds one
# class only, so the probes stand beside the battery and are not counted in its three-quarters
# condition; each must hold 8 census packets of its class and get one flagged.
# name -> (sphere: 1 outer / 0 inner, keyword arguments of limb_probe, the class it holds)
PROBES = {
    # section 1's 4e-5: the outer limb 5.5e-6 rad beyond the zero column, sqrt(2) R away (where
    # sin^2 changes fastest).  The packets left of the column end half a pixel beyond it; every ray
    # of theirs within 1e-5 of the column is lifted onto the globe, 4.5e-6 rad inside the limb
    # (2.4 eps): without the clamp term those packets clear the limb by the certificate's other
    # terms (4.5e-6 rad) and would be flagged void.
    "limb_clamp": (1, dict(ratio=math.sqrt(2.0), side=1, offset=5.5e-6, pixel=3e-6), "void"),
    # section 4(b)'s rho <= 1/4 where it binds: the inner limb from 71 R, where the cone's and
    # delta's share of the slack shrinks with R / P (to under an eps), the clamp pushing the zero
    # column's rays outwards.  g = 4 eps P^2 lies 2.7e-4 rad inside the limb there, so with the limb
    # 3e-4 rad beyond the zero column the certificate's own bound crosses the frame's left third.
    "limb_rho": (0, dict(ratio=71.0, side=-1, offset=-3.0e-4, pixel=3e-6), "interior"),
}


@functools.lru_cache(maxsize=None)
def _random_params():
    rng = np.random.default_rng(SEED)
    out = []
    for _ in range(NUM_RANDOM):
        ratio = math.exp(rng.uniform(math.log(1.002), math.log(71.0)))
        direction = _unit(rng.normal(size=3))
        # across the view axis, so the offset moves the limb in the frame and not along the line of sight
        look = _up(direction, rng.uniform(0.0, 360.0)) * rng.uniform(0.4, 0.8)
        out.append(dict(ratio=ratio, direction=tuple(direction), look=tuple(look), roll=rng.uniform(0.0, 360.0),
                        span=rng.uniform(0.8, 1.2), keep_look=True))
    return out


RANDOM = tuple(f"random{k:02d}" for k in range(NUM_RANDOM))


def scenes_of(name):
    return ("flat",) if name in RANDOM or name in PROBES else NAMED[name][0]


def refuses(name):
    return name in NAMED and NAMED[name][2]


def camera(name, scene):
    """The camera tuple of a named or random camera or a probe on a scene (the radii are the scene's own)."""
    if name in PROBES:
        return limb_probe(radii(scene)[PROBES[name][0]], **PROBES[name][1])
    if name in RANDOM:
        spec = _random_params()[RANDOM.index(name)]
    else:
        spec = NAMED[name][1]
    if isinstance(spec, tuple):
        return spec
    return globe_camera(radii(scene)[1], **spec)


def launch_params(name, scene, W, H):
    return irt.setup_frame(cells(scene), W, H, camera=camera(name, scene), info=info(scene)).lp


# ------------------------------------------------------------------------------ the float64 census
JITTERS = np.unique(np.concatenate([np.linspace(0.0, 1.0, 9)[:-1], [ONE_BELOW]]))


def census_void(lp, inf, W, H):
    """test_void_cpu._f64_void: packets all of whose sampled rays miss the outer sphere and pass
    the box, in float64, no margin."""
    from test_void_cpu import _f64_void
    return _f64_void(lp, inf, W, H)


def census_interior(lp, inf, W, H):
    """The interior twin: packets every sampled ray of which (JITTERS^2 per active pixel), in
    float64 and with no margin, passes the box, hits the inner sphere and has t0 < st2."""
    x0, y0, x1, y1 = _packet_rects(W, H)
    c = lp.camera12().astype(np.float64)
    org = c[0:3]
    r = float(inf.sphericalBounds.lower.x)
    lo = np.array(inf.bounds.lower.tolist()) - org
    hi = np.array(inf.bounds.upper.tolist()) - org
    ju, jv = (j.ravel() for j in np.meshgrid(JITTERS, JITTERS))
    ys, xs = np.mgrid[0:H, 0:W]
    ok = np.zeros((H, W), bool)
    for rows in np.array_split(np.arange(H), max(1, H * W // 4096)):  # (bounded temporaries)
        a = (xs[rows][..., None] + 0.5) + ju
        b = (ys[rows][..., None] + 0.5) + jv
        d = c[3:6] + a[..., None] * c[6:9] + b[..., None] * c[9:12]
        d = d / np.linalg.norm(d, axis=-1, keepdims=True)
        d = np.where(np.abs(d) < 1e-5, 1e-5, d)
        tl, th = lo / d, hi / d
        t0 = np.maximum(0.0, np.minimum(tl, th).max(-1))
        t1 = np.minimum(1e10, np.maximum(tl, th).min(-1))
        A = (d * d).sum(-1)
        B = 2.0 * (d @ org)
        Cc = org @ org - r * r
        disc = B * B - 4.0 * A * Cc
        with np.errstate(invalid="ignore", divide="ignore"):
            s = np.sqrt(disc)
            q = np.where(B < 0, -0.5 * (B - s), -0.5 * (B + s))
            st2 = np.minimum(q / A, Cc / q)
            ray = (t0 < t1) & (disc >= 0) & (t0 < st2)
        ok[rows] = ray.all(-1)
    out = np.zeros(len(x0), bool)
    for p in np.nonzero((x0 < W) & (y0 < H))[0]:
        out[p] = ok[y0[p]:y1[p], x0[p]:x1[p]].all()
    return out
