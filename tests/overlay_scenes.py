"""Inputs and the expected answer of the overlay (include/icon_rt_hip.h, "overlay"), shared by
tests/test_overlay_cpu.py (the helpers against float64 NumPy, the bins against the scan, the census of
these inputs) and tests/test_gpu_overlay.py (the device against irt_overlay_cover and the restatement
of the frame, integer for integer and bit for bit).  The rays, the sphere hits, the lerp and the sRGB
bytes come from tests/levels_scenes.py.  Everything is computed once per process and read-only."""
import functools

import numpy as np

import helpers
import irt
import levels_scenes as LS
import sample_scenes as S

F = np.float32
RAD = np.pi / 180.0
SCENE = "flat"  # the context's scene: the overlay reads nothing of it but the globe's radius

# two widths and two alphas, one of them 1.0 (straight alpha; the products r * a round)
W_WIDE, W_THIN = 0.03, 0.012
STYLES = (((0.9, 0.45, 0.15, 1.0), W_WIDE), ((0.2, 0.8, 0.35, 0.6), W_THIN))
MAX_W = max(w for _, w in STYLES)

SIZES = {"one": (1, 1), "packet": (8, 8), "odd": (41, 23), "square": (64, 64)}
# outside the globe, inside it (the far hit), and beside it: part of the frame misses the sphere
VIEWS = {"outside": "framing", "inside": "underground", "beside": "graze"}
COAST_BINS = (4, 64)


def frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def surface_radius():
    return float(S.shell(S.scene(SCENE))[0])


@functools.lru_cache(maxsize=None)
def launch_params(view_name, size, accum_id=0):
    W, H = SIZES[size]
    cam = helpers.view_battery(S.scene(SCENE))[VIEWS[view_name]]
    lp = irt.setup_frame(S.scene(SCENE), W, H, camera=cam).lp
    lp.accumID = accum_id
    return lp


# ------------------------------------------------------------------ the line sets
def unit_latlon(lat, lon):
    lat, lon = np.asarray(lat, np.float64), np.asarray(lon, np.float64)
    return np.stack([np.cos(lat) * np.cos(lon), np.cos(lat) * np.sin(lon), np.sin(lat)], -1)


def latlon_of(v):
    v = np.asarray(v, np.float64)
    v = v / np.linalg.norm(v, axis=-1, keepdims=True)
    return np.arcsin(v[..., 2]), np.arctan2(v[..., 1], v[..., 0])


def line_through(p, q):
    """(lat, lon) float32 of the two points p, q given as 3-vectors."""
    lat, lon = latlon_of(np.array([p, q]))
    return lat.astype(F), lon.astype(F)


@functools.lru_cache(maxsize=None)
def coast_track():
    """A seeded random walk of 5,001 points, steps of about 2e-3 rad (shorter than either width),
    started near the north pole, where the outside view looks."""
    rng = np.random.default_rng(2026)
    p = unit_latlon(80 * RAD, 20 * RAD)
    head = rng.uniform(0, 2 * np.pi)
    pts = [p]
    for _ in range(5000):
        head += rng.normal(0.0, 0.35)
        north = np.array([0.0, 0.0, 1.0]) - p[2] * p
        north = north / np.linalg.norm(north) if np.linalg.norm(north) > 1e-6 else np.array([1.0, 0.0, 0.0])
        east = np.cross(north, p)
        step = 2e-3 * (0.8 + 0.4 * rng.uniform())
        p = p + step * (np.cos(head) * north + np.sin(head) * east)
        p = p / np.linalg.norm(p)
        pts.append(p)
    lat, lon = latlon_of(np.array(pts))
    return frozen(lat.astype(F)), frozen(lon.astype(F))


@functools.lru_cache(maxsize=None)
def view_anchor(view):
    """The middle of what a view sees of the sphere: the normalised mean of its 64 x 64 frame's points."""
    live, u = frame_points(view, "square")
    c = u[live].astype(np.float64).mean(0)
    return frozen(c / np.linalg.norm(c))


@functools.lru_cache(maxsize=None)
def polylines(name):
    """The set's polylines: a list of (lat, lon, max_arc, style)."""
    deg = RAD
    if name == "none":
        return ()
    if name == "single":  # one 1 degree arc, where the outside view looks
        return ((np.array([70, 70.7], F) * F(deg), np.array([10, 12], F) * F(deg), 0.2, 0),)
    if name == "cube-corner":
        # the cube-map corner and the point of a cube-map edge nearest to where a view looks (the inside
        # view sees them from below), a wide arc across each: three faces meet under the first, two under
        # the second
        c = view_anchor("inside")
        corner = np.where(c >= 0, 1.0, -1.0)
        lo = int(np.argmin(np.abs(c)))          # the edge between the faces of the two larger components
        edge = corner.copy()
        edge[lo] = 0.25 * corner[lo]
        out = []
        for k, (p, style) in enumerate(((corner / np.linalg.norm(corner), 0), (edge / np.linalg.norm(edge), 1))):
            e1 = np.cross(p, [0.3, -0.5, 0.8])
            e1 = e1 / np.linalg.norm(e1)
            e2 = np.cross(p, e1)
            d = e1 + (0.4 if k == 0 else -0.3) * e2
            out.append(line_through(p - 0.09 * d, p + 0.085 * d) + (0.2, style))
        return tuple(out)
    if name == "pole":  # a meridian pair through the north pole
        lat = np.array([60, 90, 60], F) * F(deg)
        return ((lat, np.array([30, 30, 210], F) * F(deg), 5 * deg, 0),
                (lat, np.array([120, 120, 300], F) * F(deg), 5 * deg, 1))
    if name == "coast":
        lat, lon = coast_track()
        return ((lat, lon, 0.2, 1),)
    if name == "overlap":
        # where the inside and the outside view look, two lines crossing at 8 degrees: the wide line has
        # the lower indices, so a point inside its width but nearer to the thin line's axis has a lowest
        # covering index that is not its nearest segment
        wide, thin = [], []
        for view, shift in (("inside", 0.0), ("outside", 0.12)):
            c = view_anchor(view)
            e1 = np.cross(c, [0.0, 0.6, 0.8])
            e1 = e1 / np.linalg.norm(e1)
            e2 = np.cross(c, e1)
            c = c + shift * e2
            th = 8 * deg
            wide.append(line_through(c - 0.25 * e1, c + 0.25 * e1) + (0.2, 0))
            d = np.cos(th) * e1 + np.sin(th) * e2
            thin.append(line_through(c - 0.25 * d, c + 0.25 * d) + (0.2, 1))
        return tuple(wide + thin)
    if name == "views":
        # beyond the issue's list: a cross of a wide and a thin line through the middle of what each view
        # sees of the sphere, so that the inside and the beside view have lines, overlaps and free pixels too
        out = []
        for view in VIEWS:
            live, u = frame_points(view, "square")
            c = view_anchor(view)
            e1 = np.cross(c, [0.0, 0.0, 1.0])
            e1 = e1 / np.linalg.norm(e1)
            e2 = np.cross(c, e1)
            reach = 0.5 * np.arccos(np.clip(u[live].astype(np.float64) @ c, -1, 1)).max()
            for k, d in enumerate((e1 + 0.3 * e2, e2 - 0.2 * e1)):
                out.append(line_through(c - reach * d, c + reach * d) + (0.2, k))
        return tuple(out)
    raise KeyError(name)


SET_NAMES = ("none", "single", "cube-corner", "pole", "graticule", "coast", "overlap", "views")


@functools.lru_cache(maxsize=None)
def segments(name):
    if name == "graticule":
        return frozen(irt.graticule(30 * RAD, 30 * RAD, 5 * RAD, 0))
    parts = [irt.overlay_segments(lat, lon, None, arc, style) for lat, lon, arc, style in polylines(name)]
    return frozen(np.concatenate(parts) if parts else np.zeros(0, irt.SEGMENT_DTYPE))


# (set, binsPerEdge for the device object; 0: the library's choice)
DEVICE_SETS = tuple((n, 0) for n in SET_NAMES if n != "coast") + tuple(("coast", b) for b in COAST_BINS)


# ------------------------------------------------------------------ float64 restatements
def restate_segments(lat, lon, max_arc, style):
    """irt_overlay_segments of one polyline in float64 NumPy: the fields before their rounding."""
    p = unit_latlon(np.asarray(lat, F), np.asarray(lon, F))
    keep = [0]
    for i in range(1, len(p)):
        if not np.array_equal(p[i].astype(F), p[keep[-1]].astype(F)):
            keep.append(i)
    p = p[keep]
    out = []
    for a, b in zip(p[:-1], p[1:]):
        omega = np.arctan2(np.linalg.norm(np.cross(a, b)), np.dot(a, b))
        pieces = max(1, int(np.ceil(omega / float(F(max_arc)))))
        ts = np.arange(pieces + 1) / pieces
        q = (np.sin((1 - ts) * omega)[:, None] * a + np.sin(ts * omega)[:, None] * b) / np.sin(omega)
        q = q / np.linalg.norm(q, axis=1, keepdims=True)
        q[0], q[-1] = a, b
        for pa, pb in zip(q[:-1], q[1:]):
            n = np.cross(pa, pb)
            t = pb - pa
            half = 0.5 * np.arctan2(np.linalg.norm(n), np.dot(pa, pb))
            out.append((pa, pb, n / np.linalg.norm(n), t / np.linalg.norm(t), np.sin(half), style))
    return out


def arc_distance(seg, u):
    """The true angular distance (float64) of the unit vectors u (n, 3) to each segment's arc:
    (n, len(seg))."""
    u = np.asarray(u, np.float64)
    u = u / np.linalg.norm(u, axis=-1, keepdims=True)
    a, b = seg["a"].astype(np.float64), seg["b"].astype(np.float64)
    a = a / np.linalg.norm(a, axis=1, keepdims=True)
    b = b / np.linalg.norm(b, axis=1, keepdims=True)
    n = np.cross(a, b)
    n = n / np.linalg.norm(n, axis=1, keepdims=True)
    ang = lambda x, y: np.arctan2(np.linalg.norm(np.cross(x, y), axis=-1), (x * y).sum(-1))  # noqa: E731
    un = u @ n.T                                         # (n, m)
    d_circle = np.abs(np.arcsin(np.clip(un, -1, 1)))
    # the foot of u on the great circle lies on the arc iff it is on b's side of a and a's side of b
    foot_a = (np.cross(a, n)[None] * u[:, None, :]).sum(-1)  # u . (a x n) <= 0 ...
    foot_b = (np.cross(n, b)[None] * u[:, None, :]).sum(-1)
    inside = (foot_a <= 0) & (foot_b <= 0)
    d_a = ang(u[:, None, :], a[None])
    d_b = ang(u[:, None, :], b[None])
    return np.where(inside, d_circle, np.minimum(d_a, d_b))


def widths_of(seg):
    return np.array([w for _, w in STYLES])[seg["style"]]


# ------------------------------------------------------------------ the frames' points
@functools.lru_cache(maxsize=None)
def frame_points(view_name, size, accum_id=0):
    """The restatement of the call's points in float32: (live (H, W) bool, u (H, W, 3) float32)."""
    W, H = SIZES[size]
    lp = launch_params(view_name, size, accum_id)
    org = lp.camera12()[0:3]
    d = LS.rays(lp, W, H)
    hit, tn, tf = LS.sphere_hits(org, d, surface_radius())
    near = tn > 0
    live = hit & (near | (tf > 0))
    t = np.where(near, tn, tf).astype(F)
    P = (org[None, None, :] + d * t[..., None]).astype(F)
    ln = np.sqrt((P[..., 0] * P[..., 0] + P[..., 1] * P[..., 1]) + P[..., 2] * P[..., 2])
    with np.errstate(invalid="ignore", divide="ignore"):
        u = (P / ln[..., None]).astype(F)
    u[~live] = 0
    assert u.dtype == F
    return frozen(live), frozen(u)


@functools.lru_cache(maxsize=None)
def all_frame_points():
    """Every live unit vector of every (view, size): (n, 3) float32."""
    parts = []
    for v in VIEWS:
        for s in SIZES:
            live, u = frame_points(v, s)
            parts.append(u[live])
    return frozen(np.concatenate(parts))


def frame_subset(name):
    """The frames' points a set is judged on: all of them, every eighth for the 5,000-segment coast
    (the float64 distances are points x segments)."""
    return all_frame_points()[::8 if name == "coast" else 1]


@functools.lru_cache(maxsize=None)
def placed_points(name):
    """Points placed on the set's arcs, at their end points, at +-W (1 +- 0.01) beside them and beyond
    their ends, float32 unit vectors (n, 3); at most 400 segments of a set are used (100 of the coast)."""
    seg = segments(name)
    if seg.size == 0:
        return frozen(np.zeros((0, 3), F))
    sel = seg[np.linspace(0, seg.size - 1, min(seg.size, 100 if name == "coast" else 400)).astype(int)]
    a, b, n = (sel[k].astype(np.float64) for k in ("a", "b", "n"))
    w = widths_of(sel)[:, None]
    mid = a + b
    mid = mid / np.linalg.norm(mid, axis=1, keepdims=True)
    t = b - a
    t = t / np.linalg.norm(t, axis=1, keepdims=True)
    out = [a, b, mid, 0.3 * a + 0.7 * b]
    for base in (mid, a, b):
        for f in (0.99, 1.01, -0.99, -1.01, 0.5):
            out.append(base * np.cos(f * w) + n * np.sin(f * w))
    for f in (0.5, 0.99, 1.01, 2.0):  # beyond the ends, along the arc's direction
        out.append(b * np.cos(f * w) + np.cross(n, b) * np.sin(f * w))
        out.append(a * np.cos(f * w) - np.cross(n, a) * np.sin(f * w))
    out.append(-mid)  # the antipode of the arc
    p = np.concatenate(out)
    p = p / np.linalg.norm(p, axis=1, keepdims=True)
    return frozen(p.astype(F))


@functools.lru_cache(maxsize=None)
def border_points(N):
    """Unit vectors on bin borders, cube edges, cube corners and the poles for N bins per edge."""
    rng = np.random.default_rng(N)
    pts = [np.eye(3), -np.eye(3)]
    for sx in (-1, 1):
        for sy in (-1, 1):
            pts.append(np.array([[sx, sy, 1.0], [sx, sy, -1.0], [sx, sy, 0.3], [sx, 0.7, sy], [-0.2, sx, sy]]))
    edges = -1.0 + 2.0 * np.unique(np.concatenate([np.arange(0, N + 1, max(1, N // 8)), [1, N - 1, N]])) / N
    for e in edges:
        q = rng.uniform(-1, 1, 6)
        for face in range(3):
            for sgn in (-1.0, 1.0):
                for other in q:
                    v = [0.0, 0.0, 0.0]
                    v[face], v[(face + 1) % 3], v[(face + 2) % 3] = sgn, e, other
                    pts.append(np.array([v]))
                    v2 = list(v)
                    v2[(face + 1) % 3], v2[(face + 2) % 3] = other, e
                    pts.append(np.array([v2]))
    p = np.concatenate(pts).astype(np.float64)
    p = p / np.linalg.norm(p, axis=1, keepdims=True)
    return frozen(p.astype(F))


@functools.lru_cache(maxsize=None)
def judged_points(name):
    """The points the CPU tests judge the set on: the frames' and the placed ones."""
    return frozen(np.concatenate([frame_subset(name), placed_points(name)]))


@functools.lru_cache(maxsize=None)
def scan(name):
    """irt_overlay_cover with NULL bins on judged_points(name)."""
    return frozen(irt.overlay_cover(segments(name), STYLES, judged_points(name)))


# ------------------------------------------------------------------ the frame's restatement
def line_table():
    """L = (r a, g a, b a, a) per style in float32, one multiply each."""
    t = np.zeros((len(STYLES), 4), F)
    for k, (rgba, _) in enumerate(STYLES):
        r, g, b, a = (F(x) for x in rgba)
        t[k] = (r * a, g * a, b * a, a)
    return t


def prior_cover(W, H):
    """A non-zero premultiplied line layer for accumID > 0 to lerp onto."""
    rng = np.random.default_rng(11)
    a = rng.uniform(0.0, 1.0, (H, W, 1)).astype(F)
    return (rng.uniform(0.0, 1.0, (H, W, 4)).astype(F) * a).astype(F)


def random_accum(W, H):
    """A premultiplied frame accum."""
    rng = np.random.default_rng(13)
    a = rng.uniform(0.0, 1.0, (H, W, 1)).astype(F)
    c = (rng.uniform(0.0, 1.0, (H, W, 3)).astype(F) * a).astype(F)
    return np.concatenate([c, a], -1).astype(F)


def expected_frame(name, view_name, size, accum_id, over, accum_in, prior):
    """(segment (H, W) int32, cover (H, W, 4), fb (H, W) uint32) by the definition: accum_in (H, W, 4) or
    None, prior the cover before the call."""
    W, H = SIZES[size]
    live, u = frame_points(view_name, size, accum_id)
    seg = segments(name)
    s = np.full((H, W), -1, np.int32)
    if live.any():
        s[live] = irt.overlay_cover(seg, STYLES, u[live])
    L = np.zeros((H, W, 4), F)
    if seg.size:
        L[s >= 0] = line_table()[seg["style"][s[s >= 0]]]
    K = LS.lerp(L, prior, accum_id)
    V = np.zeros((H, W, 4), F) if accum_in is None else np.asarray(accum_in, F)
    top, below = (K, V) if over else (V, K)
    out = (top + (F(1.0) - top[..., 3:4]) * below).astype(F)
    assert out.dtype == F
    return s, K, LS.pixels(out)
