"""Scenes, points, lat/lon grids and oracle answers shared by tests/test_sample_cpu.py (the census
of these inputs by the oracle alone) and tests/test_gpu_sample.py (irt_sample_points /
irt_sample_latlon on the device against the same answers).  Everything is computed once per
process and read-only."""
import functools

import numpy as np

import helpers
import irt
import oracle as O

SCENE_NAMES = ("flat", "terrain", "filtered")


def _frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def scene(name):
    if name == "flat":  # R2B03 x 90: every column's layers at the same radii
        return _frozen(irt.synth_grid(2, 3, 90))
    if name == "terrain":  # terrain offsets, unsorted, zero-thickness and inverted records
        return _frozen(helpers.terrain_cells(11))
    if name == "filtered":  # a lat/lon window of a globe: most directions hold no cell
        return _frozen(irt.filter_cells(irt.synth_grid(2, 3, 40), (-30, 60), (-90, 45)))
    raise KeyError(name)


# Points the guard must not hand to a locator.  The first three have an answer in the reference
# (len = 0 or inf against positive heights: a miss), which the oracle gives; the last two are
# misses by definition (a NaN or infinite coordinate).
GUARD_POINTS = np.array([(0, 0, 0), (3e38, 0, 0), (1e-30, 0, 0), (1e6, np.nan, 2e6), (1e6, 2e6, -np.inf)],
                        np.float32)
N_GUARD_ORACLE = 3  # of GUARD_POINTS, those compared with the oracle


@functools.lru_cache(maxsize=None)
def points(name):
    """helpers.locator_points(scene, 5) -- random points in and around the shell, and points on and
    one float either side of record boundaries at cell centres, edge midpoints and corners --
    followed by GUARD_POINTS."""
    return _frozen(np.concatenate([helpers.locator_points(scene(name), 5), GUARD_POINTS]))


@functools.lru_cache(maxsize=None)
def cell_answers(name):
    """(found, value) of oracle.sample_volume(scene, points, fast=1); the two non-finite guard
    points are misses by definition (the oracle is not asked)."""
    pts = points(name)
    n = len(pts) - (len(GUARD_POINTS) - N_GUARD_ORACLE)
    f, v = O.sample_volume(scene(name), pts[:n], fast=1)
    pad = len(pts) - n
    return (_frozen(np.concatenate([f, np.zeros(pad, np.int32)])),
            _frozen(np.concatenate([v, np.zeros(pad, np.float32)])))


# ------------------------------------------------------------------ lat/lon grids
GRID_SHAPES = ((1, 1, 1), (2, 7, 9), (1, 8, 8), (3, 17, 33), (4, 64, 128))  # (levels, lat, lon)

# The census counts a level as below or above the shell when its radius is at least this far
# (metres) from height[0] or the top.  A grid point's own float length sqrtf(x*x + y*y + z*z),
# which sample() tests (ICONGrid.h:184), differs from the level's radius by a few ulp (0.5 m at
# 6.4e6 m): of the level one float below height[0] 14 % of the points round onto it and are found,
# of the level one float above the top 29 %.  Those two levels are compared with the oracle point
# by point like every other, but are neither "inside" nor "outside" for the census.  Every level
# with height[0] < radius < top counts as inside, the two one float inside included.
CENSUS_MARGIN = 8.0


def shell(cells):
    """(height[0] minimum, top maximum, one layer boundary strictly inside) of a scene."""
    top = cells["height"][np.arange(cells.size), cells["numLayers"]]
    i = int(np.argmax(cells["numLayers"]))
    inner = cells["height"][i][int(cells["numLayers"][i]) // 2]
    return np.float32(cells["height"][:, 0].min()), np.float32(top.max()), np.float32(inner)


@functools.lru_cache(maxsize=None)
def grid(name, shape):
    """(lat, lon, radius) float32 of a grid of GRID_SHAPES over scene(name).  lat runs from
    -pi/2 to pi/2 (as floats) with an exact 0, lon from -pi to the float below pi with an exact
    0 (a one-point axis is [0]).  The levels, over the five grids: height[0] and the top exactly,
    one float either side of each, one layer radius inside, mid-shell radii, one level below the
    shell and one above."""
    levels, nlat, nlon = shape
    h0, top, inner = shell(scene(name))
    up, down = np.float32(np.inf), np.float32(0)
    mid = np.float32(0.5 * (float(h0) + float(top)))
    radii = {
        (1, 1, 1): [inner],
        (2, 7, 9): [h0, top],
        (1, 8, 8): [np.float32(h0 - 500.0)],
        (3, 17, 33): [np.nextafter(h0, down), np.nextafter(h0, up), np.float32(top + 500.0)],
        (4, 64, 128): [np.nextafter(top, down), np.nextafter(top, up), inner, mid],
    }[shape]
    assert len(radii) == levels
    half_pi, pi = np.float32(np.pi / 2), np.float32(np.pi)
    lat = np.linspace(-half_pi, half_pi, nlat, dtype=np.float64).astype(np.float32)
    lon = np.linspace(-pi, np.nextafter(pi, down), nlon, dtype=np.float64).astype(np.float32)
    if nlat > 1:
        lat[0], lat[-1] = -half_pi, half_pi
    if nlon > 1:
        lon[0], lon[-1] = -pi, np.nextafter(pi, down)
    lat[nlat // 2] = 0.0
    lon[nlon // 2] = 0.0
    return _frozen(lat), _frozen(lon), _frozen(np.array(radii, np.float32))


def oracle_to_cartesian(r, lat, lon):
    """The oracle's toCartesian (ICONGrid.h:44-54) of one (r, lat, lon), float32 x 3."""
    import ctypes as C
    o = O.OVec3()
    O.olib().oracle_to_cartesian(O.v3((r, lat, lon)), C.byref(o))
    return np.array([o.x, o.y, o.z], np.float32)


@functools.lru_cache(maxsize=None)
def grid_points(name, shape):
    """irt.latlon_points of grid(name, shape): (levels, lat, lon, 3)."""
    return _frozen(irt.latlon_points(*grid(name, shape)))


@functools.lru_cache(maxsize=None)
def grid_answers(name, shape):
    """(found, value) of oracle.sample_volume at grid_points, flat in (level, lat, lon) order."""
    f, v = O.sample_volume(scene(name), grid_points(name, shape).reshape(-1, 3), fast=1)
    return _frozen(f), _frozen(v)


def same_bits(found_a, value_a, found_b, value_b):
    """found flags equal and every value equal as bits (the cell sampler's bar: no NaN leeway)."""
    fa, fb = np.asarray(found_a) != 0, np.asarray(found_b) != 0
    va = np.ascontiguousarray(value_a, np.float32).view(np.uint32)
    vb = np.ascontiguousarray(value_b, np.float32).view(np.uint32)
    bad = (fa != fb) | (va != vb)
    return int(np.flatnonzero(bad)[0]) if bad.any() else -1
