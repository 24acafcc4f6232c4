"""Inputs and expected answers of the sections (include/icon_rt_hip.h, "sections"), shared by
tests/test_section_cpu.py (the host helpers, and the census of these inputs by the oracle alone) and
tests/test_gpu_section.py (irt_section on the device, bit for bit).  The scenes are
sample_scenes.scene's, the levels and weights column_scenes', the transfer functions and the
classification levels_scenes'; the answers are the oracle samplers' at irt.section_points.
Everything is computed once per process and read-only."""
import functools

import numpy as np

import column_scenes as CS
import irt
import levels_scenes as LS
import sample_scenes as S

F = np.float32
SCENE_NAMES = S.SCENE_NAMES
MISS = CS.MISS
PI, HALF_PI = F(np.pi), F(np.pi / 2)
BELOW_PI = np.nextafter(PI, F(0))
AMBIENT = LS.AMBIENT  # ((0.9, 0.8, 0.7), 1.25): products that round
TRANSFUNCS = ("default", "translucent")


def _frozen(a):
    a.setflags(write=False)
    return a


# ------------------------------------------------------------------ the columns
# Tracks by irt.great_circle (lat0, lon0, lat1, lon1, n), radians.  Between them and STATIONS the
# column counts 1, 63, 64, 65 and 130: the edges of a wave's 64 columns.
TRACKS = {
    "equator": (0.0, 3.0, 0.0, -3.0, 130),                       # along the equator across the date line
    "pole": (1.0, 0.3, 0.9, 0.3 + np.pi, 65),                    # over the north pole
    "meridian": (float(HALF_PI), 0.7, -float(HALF_PI), 0.7, 64),  # pole to pole, exactly +-pi/2 as floats
    "oblique": (0.30, -0.40, 0.36, -0.28, 63),                   # short, inside filtered's window
    "point": (0.2, 0.1, 0.5, 0.9, 1),                            # one column
}
SETS = tuple(TRACKS) + ("stations",)


@functools.lru_cache(maxsize=None)
def columns(key):
    """(lat, lon) float32 of a set of SETS.  "stations": 41 unordered pairs over the globe -- inside
    and outside filtered's window of lat [-30, 60] x lon [-90, 45] degrees -- with one pair three
    times, lon = -pi and the float below pi, and a lat of exactly 0."""
    if key in TRACKS:
        lat, lon, _ = irt.great_circle(*TRACKS[key])
        return _frozen(lat), _frozen(lon)
    if key != "stations":
        raise KeyError(key)
    rng = np.random.default_rng(41)
    lat = np.arcsin(rng.uniform(-1, 1, 41)).astype(F)
    lon = rng.uniform(-np.pi, np.pi, 41).astype(F)
    lat[:6] = np.radians([10.0, 45.0, -20.0, 30.0, 59.0, 0.0]).astype(F)   # inside the window
    lon[:6] = np.radians([-30.0, 10.0, -80.0, 40.0, -89.0, 0.0]).astype(F)
    lat[7], lon[7] = lat[20], lon[20] = lat[1], lon[1]  # one pair, three times
    lon[9], lon[11] = -PI, BELOW_PI
    lat[13] = F(0.0)
    return _frozen(lat), _frozen(lon)


def levels(name, which="shuffled"):
    """column_scenes' level sets: every layer mid-radius, height[0] and the top exactly, one level
    500 m below the shell and one above, one radius twice -- "ascending" or "shuffled"."""
    return CS.levels(name, which)


weights = CS.weights
WEIGHTS = CS.WEIGHTS


@functools.lru_cache(maxsize=None)
def points(name, key, which="shuffled"):
    """irt.section_points of columns(key) on levels(name, which): (levels, columns, 3)."""
    lat, lon = columns(key)
    return _frozen(irt.section_points(lat, lon, levels(name, which)))


@functools.lru_cache(maxsize=None)
def answers(name, key, which="shuffled", mode=irt.MODE_USER_GEOM):
    """(found uint8, value float32), each (levels, columns): the mode's oracle sampler at
    points(name, key, which) behind the guard of irt_sample_points (levels_scenes.sample)."""
    pts = points(name, key, which)
    f, v = LS.sample(S.scene(name), mode, pts.reshape(-1, 3))
    return _frozen(f.astype(np.uint8).reshape(pts.shape[:2])), _frozen(np.asarray(v, F).reshape(pts.shape[:2]))


def values(name, key, which="shuffled", mode=irt.MODE_USER_GEOM, miss=MISS):
    """What irt_section writes to `value`: the answer where found, `miss` elsewhere."""
    f, v = answers(name, key, which, mode)
    return np.where(f != 0, v, F(miss)).astype(F)


@functools.lru_cache(maxsize=None)
def reduced(name, key, wname, which="shuffled", mode=irt.MODE_USER_GEOM, miss=MISS):
    """irt.column_reduce of answers(...) with weights(wname): the six column outputs, (columns,)."""
    f, v = answers(name, key, which, mode)
    return {k: _frozen(a) for k, a in irt.column_reduce(v, f, weights(wname, v.shape[0]), miss).items()}


# ------------------------------------------------------------------ the curtain
def curtain_of(tf, found, value, ambient=AMBIENT):
    """The definition of rgba restated from the oracle's pieces: s = postClassify(v), a = clamp(s.w,
    0, 1), C = a * ((s.rgb * ambientColor) * ambientRadiance) in float32, the pixel
    make_rgba(linear_to_srgb(C), a); 0 where the point was not found.  uint32 of found's shape."""
    f = np.asarray(found) != 0
    s4 = np.zeros(f.shape + (4,), F)
    s4[f] = LS.classify(tf, np.asarray(value, F)[f])
    a = np.where(s4[..., 3] < 0, F(0), np.where(s4[..., 3] > 1, F(1), s4[..., 3])).astype(F)
    amb, rad = np.array(ambient[0], F), F(ambient[1])
    C = (a[..., None] * ((s4[..., :3] * amb) * rad)).astype(F)
    colour = np.concatenate([C, a[..., None]], -1).astype(F)
    assert colour.dtype == F
    px = LS.pixels(colour.reshape(-1, 1, 4)).reshape(f.shape)
    px[~f] = 0
    return px


@functools.lru_cache(maxsize=None)
def curtain(name, key, tf_name, which="shuffled", ambient=AMBIENT):
    f, v = answers(name, key, which)
    return _frozen(curtain_of(LS.transfunc(name, tf_name), f, v, ambient))


# The curtains both test files walk: (scene, set, transfer function)
CURTAINS = (("flat", "equator", "default"), ("flat", "stations", "translucent"),
            ("terrain", "pole", "translucent"), ("terrain", "stations", "default"),
            ("filtered", "oblique", "default"), ("filtered", "stations", "translucent"))


# ------------------------------------------------------------------ pairs that form a grid
@functools.lru_cache(maxsize=None)
def grid_pairs(name):
    """column_scenes' grid "five" (7 x 9 x 5 levels) and its pairs in row-major order: (lat, lon,
    radius, pair lat, pair lon)."""
    lat, lon, rad = CS.grid(name, "five")
    return lat, lon, rad, _frozen(np.repeat(lat, lon.size)), _frozen(np.tile(lon, lat.size))


# ------------------------------------------------------------------ irt_great_circle restated
def great_circle_numpy(lat0, lon0, lat1, lon1, n):
    """The header's formula in float64 NumPy: unit vectors (n, 3) of the track's points and the arc.
    The end points are the inputs' own unit vectors."""
    def unit(lat, lon):
        lat, lon = np.float64(F(lat)), np.float64(F(lon))
        return np.array([np.cos(lat) * np.cos(lon), np.cos(lat) * np.sin(lon), np.sin(lat)])

    a, b = unit(lat0, lon0), unit(lat1, lon1)
    w = np.arctan2(np.linalg.norm(np.cross(a, b)), np.dot(a, b))
    if n == 1:
        return a[None], w
    if np.sin(w) < 1e-9:  # coincident end points: every point is the start
        return np.concatenate([np.repeat(a[None], n - 1, 0), b[None]]), w
    t = np.arange(n, dtype=np.float64) / (n - 1)
    p = (np.sin((1 - t) * w)[:, None] * a + np.sin(t * w)[:, None] * b) / np.sin(w)
    p /= np.linalg.norm(p, axis=1, keepdims=True)
    p[0], p[-1] = a, b
    return p, w


def unit_vectors(lat, lon):
    lat, lon = np.asarray(lat, np.float64), np.asarray(lon, np.float64)
    return np.stack([np.cos(lat) * np.cos(lon), np.cos(lat) * np.sin(lon), np.sin(lat)], -1)
