"""Scenes and points for the point-by-point tests of the two unstructured samplers, CUBQL_MODE
wedges and TRIANGLE_MODE (tests/test_samplers_cpu.py, tests/test_gpu_samplers.py).  No GPU is
needed here; every builder is deterministic and returns read-only arrays.

Scenes (SCENE_NAMES):
  heights        accel_scenes.heights(): every TREATMENTS label -- repeated, all-equal, unsorted and
                 reversed heights, records of 0, 1, 2 and 31 layers
  nonfinite      accel_scenes.nonfinite_values(): the same records with NaN, +-inf, +-FLT_MAX and
                 +-0 in value[] (SPECIALS x PLACES) and a hole of all-NaN records
  convert_icon   irt.synth_grid(2, 1, 45, terrain=4000): the layout convert_icon writes, an inverted
                 first layer over land and a last record of 45 % 32 - 1 layers
  terrain        helpers.terrain_cells(): terrain-following columns of three records, some unsorted,
                 some of zero layers, some inverted
  filtered       a lat/lon window of synth_grid(2, 2, 20, noise=0.3): boundary columns without
                 neighbours
  icosahedron    synth_grid(1, 0, 4): 20 faces whose boxes span whole cube-map faces
  single         one record

Both samplers are asked at the same points (points(name)), float32 positions built from a record's
float64 corner directions and placed with helpers.on_radius, so that the float32 |p| is the wanted
radius:
  random      the recipe of test_wedge_locator_matches_oracle_on_coarse_and_fine_grids: a random
              record, barycentric weights reaching past its edges, the radius drawn from
              [min(height[0..nl]) - 3000, max(height[0..nl]) + 3000]
  structured  per sampled record (every TREATMENTS label and every SPECIALS x PLACES combination
              among them, and all-NaN records of the hole): every layer radius height[0..nl], one
              float above it and one float below it, the direction going round the centroid, two
              edge midpoints and a corner; height[0], height[nl // 2] and height[nl] in all four
              directions.  The points whose |p| is exactly height[0] or height[numLayers] are
              TRIANGLE_MODE's radial limits (len == height[0], len == height[numLayers]): at the
              centroid and on the edges the ray toward the centre meets the bottom triangle of the
              record that starts there.
  voids       terrain scenes, records starting above the lowest radius or with an inverted first
              layer: 100 m under height[0] (nothing covers it over land) and in the middle of the
              inverted layer

Census: the share of each scene's points the oracle finds, per sampler, as measured with this
module (x86-64, g++ -O2 -ffp-contract=off); CENSUS holds these figures rounded down to 1 %, and
tests/test_samplers_cpu.py checks that each point set still reaches them.  The floor for every
multi-record scene is 15 % per sampler.  Wedge shares are low because the float Newton iteration
of intersectWedgeEXT often fails to converge at Earth scale, in the reference as here.

  scene         points  wedge found  triangle found
  heights         3258   1142 (0.351)   1020 (0.313)
  nonfinite       5739   2361 (0.411)   1830 (0.319)
  convert_icon    3522    926 (0.263)   1418 (0.403)
  terrain         3518   1027 (0.292)   1046 (0.297)
  filtered        3060   2442 (0.798)   2709 (0.885)
  icosahedron     1600    257 (0.161)   1391 (0.869)
  single           684     58 (0.085)    249 (0.364)
"""
import functools
from collections import namedtuple

import numpy as np

import accel_scenes
import helpers
import irt

SCENE_NAMES = ("heights", "nonfinite", "convert_icon", "terrain", "filtered", "icosahedron", "single")
N_RANDOM = {"heights": 900, "nonfinite": 900, "convert_icon": 900, "terrain": 900, "filtered": 900,
            "icosahedron": 400, "single": 300}
FLOOR = 0.15  # share of a multi-record scene's points each sampler's oracle must find

# name: (points, found by the wedge oracle, found by the triangle oracle), measured
MEASURED = {
    "heights": (3258, 1142, 1020),
    "nonfinite": (5739, 2361, 1830),
    "convert_icon": (3522, 926, 1418),
    "terrain": (3518, 1027, 1046),
    "filtered": (3060, 2442, 2709),
    "icosahedron": (1600, 257, 1391),
    "single": (684, 58, 249),
}
CENSUS = {k: (int(100 * w / n) / 100, int(100 * t / n) / 100) for k, (n, w, t) in MEASURED.items()}

RANDOM, STRUCTURED, VOID = 0, 1, 2
PointSet = namedtuple("PointSet", "points record kind")  # (n, 3) float32, (n,) int32, (n,) uint8


def _frozen(a):
    a = np.ascontiguousarray(a)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def scene(name):
    """The records of scene `name` (read-only)."""
    if name == "heights":
        return accel_scenes.heights()
    if name == "nonfinite":
        return accel_scenes.nonfinite_values()
    if name == "convert_icon":
        return _frozen(irt.synth_grid(2, 1, 45, terrain=4000.0))
    if name == "terrain":
        return _frozen(helpers.terrain_cells())
    if name == "filtered":
        return _frozen(irt.filter_cells(irt.synth_grid(2, 2, 20, noise=0.3), (-30, 60), (-90, 45)))
    if name == "icosahedron":
        return _frozen(irt.synth_grid(1, 0, 4))
    if name == "single":
        return _frozen(np.array(accel_scenes.heights(False)[:1], copy=True))
    raise KeyError(name)


def record_label(name, rec):
    """What a failure message says about record `rec` of scene `name`."""
    c = scene(name)[rec]
    text = f"record {rec} ({int(c['numLayers'])} layers"
    if name in ("heights", "nonfinite"):
        text += ", " + accel_scenes.TREATMENTS[accel_scenes.heights_labels()[rec]]
    if name == "nonfinite":
        k = int(accel_scenes.nonfinite_placed()[rec])
        if k >= 0:
            s, p = divmod(k, len(accel_scenes.PLACES))
            text += f", {accel_scenes.SPECIALS[s]} at {accel_scenes.PLACES[p]}"
        elif accel_scenes.nonfinite_hole()[0][rec]:
            text += ", all NaN"
    return text + ")"


def corner_dirs(c):
    """The three corner directions of record c, float64 unit vectors (3, 3)."""
    lat, lon = c["lat"].astype(np.float64), c["lon"].astype(np.float64)
    return np.stack([np.cos(lat) * np.cos(lon), np.cos(lat) * np.sin(lon), np.sin(lat)], 1)


def _sampled_records(name, cells, rng):
    """The records that get structured points."""
    if name in ("heights", "nonfinite"):
        label = accel_scenes.heights_labels()
        recs = [int(i) for t in range(len(accel_scenes.TREATMENTS)) for i in np.flatnonzero(label == t)[:2]]
        if name == "nonfinite":
            placed = accel_scenes.nonfinite_placed()
            recs += [int(np.flatnonzero(placed == k)[0]) for k in range(placed.max() + 1)]
            recs += [int(i) for i in np.flatnonzero(accel_scenes.nonfinite_hole()[0])[:2]]
        return list(dict.fromkeys(recs))
    return [int(i) for i in rng.choice(cells.size, min(24, cells.size), replace=False)]


@functools.lru_cache(maxsize=None)
def points(name):
    """The PointSet of scene `name`: a few thousand points, the same for both samplers."""
    cells = scene(name)
    rng = np.random.default_rng(SCENE_NAMES.index(name) + 40)
    pts, rec, kind = [], [], []

    def put(v, r, i, k):
        pts.append(helpers.on_radius(v, np.float32(r)))
        rec.append(i)
        kind.append(k)

    for _ in range(N_RANDOM[name]):
        i = int(rng.integers(cells.size))
        c = cells[i]
        h = c["height"][:int(c["numLayers"]) + 1]
        w = rng.dirichlet([1, 1, 1]) * 1.6 - 0.2
        put(w @ corner_dirs(c), rng.uniform(float(h.min()) - 3000, float(h.max()) + 3000), i, RANDOM)
    up, down = np.float32(np.inf), np.float32(0)
    for i in _sampled_records(name, cells, rng):
        c = cells[i]
        d = corner_dirs(c)
        dirs = (d.mean(0), d[0] + d[1], d[1] + d[2], d[0])
        nl = int(c["numLayers"])
        h = c["height"]
        for k in range(nl + 1):
            every = k in (0, nl // 2, nl) or cells.size <= 24  # a small scene: all four everywhere
            for v in (dirs if every else (dirs[k % 4],)):
                for r in (h[k], np.nextafter(h[k], up), np.nextafter(h[k], down)):
                    put(v, r, i, STRUCTURED)
    if name in ("convert_icon", "terrain"):
        h0 = cells["height"][:, 0]
        inverted = (cells["numLayers"] > 0) & (h0 > cells["height"][:, 1])
        raised = h0 > h0.min() + 1
        some = np.concatenate([np.flatnonzero(inverted)[:40], np.flatnonzero(raised & ~inverted)[:40]])
        for i in some:
            c = cells[i]
            d = corner_dirs(c)
            for v in (d.mean(0), d[0] + d[1]):
                put(v, float(c["height"][0]) - 100.0, int(i), VOID)
                if inverted[i]:
                    put(v, 0.5 * (float(c["height"][0]) + float(c["height"][1])), int(i), VOID)
    return PointSet(_frozen(np.array(pts, np.float32)), _frozen(np.array(rec, np.int32)),
                    _frozen(np.array(kind, np.uint8)))


@functools.lru_cache(maxsize=None)
def oracle_answers(name):
    """((found, value) of the oracle's wedge scan, (found, value) of its triangle scan) at
    points(name) of scene(name): computed once, read-only."""
    import oracle as O
    w = O.wedge_sample_points(scene(name), points(name).points)
    t = O.triangle_sample_points(scene(name), points(name).points)
    return tuple(_frozen(a) for a in w), tuple(_frozen(a) for a in t)


# ------------------------------------------------------------------ the comparison
def nan_blind_bits(value):
    """value as uint32 bit patterns, every NaN as one pattern."""
    v = np.ascontiguousarray(value, dtype=np.float32)
    return np.where(np.isnan(v), np.uint32(0x7FC00000), v.view(np.uint32))


def first_difference(found_a, value_a, found_b, value_b):
    """The comparison both sampler test files use: found flags equal, and where found the values
    equal as bits -- except that two NaNs count as equal whatever their sign and payload.  A wedge
    scalar is (NaN + x) * 0.5f where value[] holds a NaN, and the NaN an x86 addss and a GPU
    v_add_f32 produce from the same operands need not carry the same bits (which operand's payload
    survives, the sign of a generated NaN); IEEE 754 leaves that open, and nothing downstream
    reads it.  Returns the first differing index, or -1."""
    fa, fb = np.asarray(found_a) != 0, np.asarray(found_b) != 0
    bad = (fa != fb) | (fa & fb & (nan_blind_bits(value_a) != nan_blind_bits(value_b)))
    return int(np.flatnonzero(bad)[0]) if bad.any() else -1


def assert_same_samples(name, ps, got, want, what):
    """got, want: (found, value) at ps.points; names the first differing point, its record's
    treatment and both answers."""
    k = first_difference(got[0], got[1], want[0], want[1])
    if k < 0:
        return
    g = (int(got[0][k]), float(got[1][k]), hex(int(np.float32(got[1][k]).view(np.uint32))))
    w = (int(want[0][k]), float(want[1][k]), hex(int(np.float32(want[1][k]).view(np.uint32))))
    fa, fb = np.asarray(got[0]) != 0, np.asarray(want[0]) != 0
    n = int(((fa != fb) | (fa & fb & (nan_blind_bits(got[1]) != nan_blind_bits(want[1])))).sum())
    raise AssertionError(
        f"{what} on scene {name}: {n} of {len(ps.points)} points differ; first: point {k} "
        f"{ps.points[k].tolist()} (|p| = {float(np.sqrt(np.float32((ps.points[k] ** 2).sum())))}, "
        f"kind {int(ps.kind[k])}) placed from {record_label(name, int(ps.record[k]))}: "
        f"got (found, value, bits) {g}, oracle {w}")
