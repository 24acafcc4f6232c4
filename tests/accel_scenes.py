"""Scenes for the accelerator edge tests (tests/test_accel_scenes_cpu.py, tests/test_gpu_accel_edges.py):
synthetic grids whose records are edited in numpy so that the shell and grid builds
(csrc/irt_kernels.hip) leave their usual branches.  No GPU is needed here.

Every builder returns read-only arrays and is deterministic.  Heights and lat/lon stay finite,
and untouched columns keep sphericalBounds and bounds those of the whole globe and shell (the
`tails` slices aside, whose bounds are their records' own and never degenerate).
"""
import functools

import numpy as np

import irt

FLT_MAX = np.float32(np.finfo(np.float32).max)
SHELL = 1024  # the shell is 1 x 1024 x 1024 macrocells (lat, lon)
TAIL_SIZES = (1, 3, 255, 256, 257, 513)  # k_shell_build / k_shell_rebuild stage 256 records at a time


def _frozen(a):
    a = np.ascontiguousarray(a)
    a.setflags(write=False)
    return a


def lat_lon_bounds(cells):
    """(lat lo, lat hi, lon lo, lon hi) of the records' corners: sphericalBounds' y and z."""
    return (float(cells["lat"].min()), float(cells["lat"].max()),
            float(cells["lon"].min()), float(cells["lon"].max()))


def rect_extent(lat, lon, sb):
    """The macrocell rectangle of corners lat, lon (..., 3) under sb = (lat lo, lat hi, lon lo,
    lon hi), as buildShell_ICON projects them but in float64: (ylo, yhi, zlo, zhi)."""
    y = np.trunc((np.asarray(lat, np.float64) - sb[0]) / (sb[1] - sb[0]) * (SHELL - 1)).astype(np.int64)
    z = np.trunc((np.asarray(lon, np.float64) - sb[2]) / (sb[3] - sb[2]) * (SHELL - 1)).astype(np.int64)
    return y.min(-1), y.max(-1), z.min(-1), z.max(-1)


def rect_macrocells(cells, sb):
    """Macrocells in each record's rectangle (float64 estimate, rect_extent)."""
    ylo, yhi, zlo, zhi = rect_extent(cells["lat"], cells["lon"], sb)
    return (yhi - ylo + 1) * (zhi - zlo + 1)


# ------------------------------------------------------------------ mixed_rects
SMALL_MAX = 16         # "a few macrocells"
MEDIUM = (28, 56)      # in-lane (<= kShellSmall = 64) but several rows
WIDE_MIN = 200
SHRUNK_FRACTION = 0.3


@functools.lru_cache(maxsize=None)
def _mixed_rects():
    cells = irt.synth_grid(2, 3, 62)  # 5120 columns x 2 records
    per = 2
    ncol = cells.size // per
    lat = cells["lat"][::per].astype(np.float64)
    lon = cells["lon"][::per].astype(np.float64)
    sb = lat_lon_bounds(cells)
    est0 = rect_macrocells(cells[::per], sb)
    # columns that stay: the antimeridian seam (corners on both sides), the poles, and whatever
    # attains the lat/lon bounds (shrinking moves corners inwards only, so the bounds stay)
    seam = (lon.max(1) - lon.min(1)) > np.pi
    pole = np.abs(lat).max(1) > np.pi / 2 - 1e-6
    edge = ((lat.min(1) == sb[0]) | (lat.max(1) == sb[1]) | (lon.min(1) == sb[2]) | (lon.max(1) == sb[3]))
    keep = seam | pole | edge
    assert (est0[keep] >= WIDE_MIN).all()
    rng = np.random.default_rng(62)
    must = np.flatnonzero(~keep & (est0 < WIDE_MIN))  # too narrow to count as wide: shrink those
    free = np.flatnonzero(~keep & (est0 >= WIDE_MIN))
    want = int(SHRUNK_FRACTION * ncol)
    pick = np.concatenate([must, rng.choice(free, max(0, want - must.size), replace=False)])
    pick = rng.permutation(pick)
    # scale each picked column about its lat/lon centroid: the largest factor of a geometric
    # ladder whose float32 corners give an estimate in the wanted class
    ladder = np.geomspace(1.0, 1e-3, 400)
    cen_lat, cen_lon = lat[pick].mean(1, keepdims=True), lon[pick].mean(1, keepdims=True)
    new_lat = np.zeros((pick.size, 3), np.float32)
    new_lon = np.zeros((pick.size, 3), np.float32)
    done = np.zeros(pick.size, bool)
    small = np.arange(pick.size) % 2 == 0
    for s in ladder:
        la = (cen_lat + s * (lat[pick] - cen_lat)).astype(np.float32)
        lo = (cen_lon + s * (lon[pick] - cen_lon)).astype(np.float32)
        ylo, yhi, zlo, zhi = rect_extent(la, lo, sb)
        n = (yhi - ylo + 1) * (zhi - zlo + 1)
        ok = np.where(small, n <= SMALL_MAX, (n >= MEDIUM[0]) & (n <= MEDIUM[1]) & (yhi > ylo) & (zhi > zlo))
        take = ok & ~done
        new_lat[take], new_lon[take] = la[take], lo[take]
        done |= take
    assert done.all()
    for k in range(per):  # all records of a column on the same corners
        cells["lat"][pick * per + k] = new_lat
        cells["lon"][pick * per + k] = new_lon
    assert lat_lon_bounds(cells) == sb
    return _frozen(cells)


def mixed_rects():
    """R2B03 x 62 levels (10240 records) with ~30 % of the columns shrunk about their centroid:
    half to at most 16 macrocells, half to 28..56 in several rows (both in-lane), the rest wide
    -- more than the wide-rectangle list holds -- with the seam and both poles among them."""
    return _mixed_rects()


# ------------------------------------------------------------------ heights
TREATMENTS = ("none", "repeat_start", "repeat_middle", "repeat_end", "all_equal", "unsorted_once",
              "reversed", "h0_above_top", "layers_0", "layers_1", "layers_2", "layers_31")


def slot_values(n):
    """100 + slot index for every slot of every record, unused slots included: a wrong slot shows."""
    return (100 + np.arange(n * 32, dtype=np.float32)).reshape(n, 32)


@functools.lru_cache(maxsize=None)
def _heights(treated):
    cells = irt.synth_grid(2, 1, 62)  # 320 columns x 2 records of 31 layers
    assert (cells["numLayers"] == 31).all()
    n = cells.size
    rng = np.random.default_rng(31)
    label = rng.integers(0, len(TREATMENTS), n)
    label[:4] = 0  # untouched records of both kinds: the radial bounds stay the shell's
    if treated:
        for i in range(n):
            h = cells["height"][i].copy()
            t = TREATMENTS[label[i]]
            nl = 31
            if t == "repeat_start":
                h[1:3] = h[0]
            elif t == "repeat_middle":
                k = int(rng.integers(5, 25))
                h[k + 1:k + 3] = h[k]
            elif t == "repeat_end":
                h[nl - 2:nl] = h[nl]
            elif t == "all_equal":
                h[:nl + 1] = h[0]
            elif t == "unsorted_once":
                k = int(rng.integers(1, nl))
                h[k], h[k + 1] = h[k + 1], h[k]
            elif t == "reversed":
                h[:nl + 1] = h[nl::-1].copy()
            elif t == "h0_above_top":
                h[0] = h[nl] + (h[nl] - h[0])
            elif t.startswith("layers_"):
                nl = int(t[7:])
                h[nl + 1:] = 0  # as a record of nl layers is written
            cells["height"][i] = h
            cells["numLayers"][i] = nl
    cells["value"] = slot_values(n)
    return _frozen(cells), _frozen(label)


def heights(treated=True):
    """R2B01 x 62 levels (640 records), each record's heights under one of TREATMENTS (seeded),
    values 100 + slot index; treated=False: the same values on the grid's own heights."""
    return _heights(bool(treated))[0]


def heights_labels():
    """Index into TREATMENTS per record of heights()."""
    return _heights(True)[1]


# ------------------------------------------------------------------ nonfinite_values
SPECIALS = (np.float32(np.nan), np.float32(np.inf), np.float32(-np.inf), FLT_MAX, -FLT_MAX,
            np.float32(-0.0), np.float32(0.0))
PLACES = ("first_used", "last_used", "slot_numLayers", "all_used")


@functools.lru_cache(maxsize=None)
def _nonfinite():
    cells = np.array(heights(), copy=True)
    n = cells.size
    nl = cells["numLayers"]
    sb = lat_lon_bounds(cells)
    ylo, yhi, zlo, zhi = rect_extent(cells["lat"], cells["lon"], sb)
    # a hole: every record whose rectangle meets that of the smallest one is NaN in all 32 slots
    # (unsorted heights make findHeight reach slot numLayers), so the macrocells in the middle of
    # that rectangle are covered and still keep the empty range
    def meets(i):
        return (ylo <= yhi[i]) & (yhi >= ylo[i]) & (zlo <= zhi[i]) & (zhi >= zlo[i])

    area = (yhi - ylo + 1) * (zhi - zlo + 1)
    kept = np.zeros(n, bool)  # the untouched records 0..3 stay finite: away from them
    for i in range(4):
        kept |= meets(i)
    c0 = int(np.flatnonzero(~kept)[np.argmin(area[~kept])])
    hole = meets(c0)
    assert hole[c0] and not hole[:4].any()
    cells["value"][hole] = np.nan
    rng = np.random.default_rng(7)
    cand = rng.permutation(np.flatnonzero(~hole & (nl >= 1) & (np.arange(n) >= 4)))
    combos = [(s, p) for s in SPECIALS for p in PLACES]
    placed = np.full(n, -1)
    for k, i in enumerate(cand[:6 * len(combos)]):
        s, p = combos[k % len(combos)]
        v = cells["value"][i]
        if p == "first_used":
            v[0] = s
        elif p == "last_used":
            v[nl[i] - 1] = s
        elif p == "slot_numLayers":
            v[nl[i]] = s
        else:
            v[:nl[i]] = s
        placed[i] = k % len(combos)
    centre = ((ylo[c0] + yhi[c0]) // 2, (zlo[c0] + zhi[c0]) // 2)
    return _frozen(cells), _frozen(hole), centre, _frozen(placed)


def nonfinite_values():
    """heights() with NaN, +-inf, +-FLT_MAX and +-0 in value[] (SPECIALS x PLACES, six records
    each) and a hole of all-NaN records; the other records stay finite."""
    return _nonfinite()[0]


def nonfinite_hole():
    """(mask of the all-NaN records of nonfinite_values(), a (y, z) macrocell they alone cover)."""
    return _nonfinite()[1], _nonfinite()[2]


def nonfinite_placed():
    """Per record of nonfinite_values(): index into SPECIALS x PLACES (row-major), or -1."""
    return _nonfinite()[3]


# ------------------------------------------------------------------ tails
def tails(n):
    """The first n records of heights(): the staging batches' edges, n % 4 != 0 among them."""
    assert n in TAIL_SIZES
    return _frozen(np.array(heights()[:n], copy=True))


SCENES = {"mixed_rects": mixed_rects, "heights": heights, "nonfinite_values": nonfinite_values}
SCENES.update({f"tails_{n}": functools.partial(tails, n) for n in TAIL_SIZES})


def scene(name):
    return SCENES[name]()


def untreated_values(name):
    """value[] (n, 32) a context of scene(name)'s records starts from before the update tests
    replace it with the scene's own: the synthetic grid's values."""
    n = scene(name).size
    assert name != "mixed_rects"
    return _frozen(irt.synth_grid(2, 1, 62)["value"][:n].astype(np.float32))


# ------------------------------------------------------------------ the data-range fold
@functools.lru_cache(maxsize=None)
def range_scene():
    """R2B01 x 45 levels: 640 records of 31 and 14 layers in turn."""
    cells = irt.synth_grid(2, 1, 45)
    assert (cells["numLayers"][0::2] == 31).all() and (cells["numLayers"][1::2] == 14).all()
    return _frozen(cells)


@functools.lru_cache(maxsize=None)
def range_value_sets():
    """value[] sets (640, 32) for range_scene() that decide irt_update_values_end's data-range
    fold: min/max of value[0:numLayers) where NaN never counts, and, where that is a zero, the
    sign of the last zero in record order (the host fold's fminf/fmaxf return their second
    argument on a tie).  Records 256 apart sit in different workgroups of the fold."""
    n = range_scene().size
    pos = (1 + np.random.default_rng(3).random((n, 32))).astype(np.float32)  # [1, 2)
    nz, pz, nan, inf = np.float32(-0.0), np.float32(0.0), np.float32(np.nan), np.float32(np.inf)
    sets = {}

    def put(name, base, edits):
        v = np.array(base, copy=True)
        for idx, x in edits:
            v[idx] = x
        sets[name] = _frozen(v)

    put("min_zero_neg_then_pos", pos, [((10, 0), nz), ((500, 3), pz)])
    put("min_zero_pos_then_neg", pos, [((10, 0), pz), ((500, 3), nz)])
    put("max_zero_neg_then_pos", -pos, [((10, 0), nz), ((500, 3), pz)])
    put("max_zero_pos_then_neg", -pos, [((10, 0), pz), ((500, 3), nz)])
    put("zero_pair_in_one_record", pos, [((300, 2), pz), ((300, 9), nz)])
    put("zero_pair_in_one_wave", pos, [((130, 30), nz), ((131, 0), pz)])
    # record 11 has 14 layers, record 12 has 31: these zeros sit in unused slots only
    put("zero_in_unused_slots_only", pos, [((11, 20), pz), ((13, 14), nz), ((12, 31), nz)])
    put("unused_zero_after_used_zero", pos, [((10, 0), pz), ((601, 14), nz), ((602, 31), nz)])
    put("nan_wave", pos, [((slice(64, 128),), nan)])
    put("nan_workgroup_and_tail", pos, [((slice(256, 512),), nan), ((slice(630, 640),), nan)])
    put("all_nan", pos, [((slice(None),), nan)])
    put("inf_both", pos, [((5, 1), inf), ((400, 2), -inf)])
    put("inf_wave", pos, [((slice(128, 192),), inf)])
    put("nan_everywhere_but_one", pos * nan, [((639, 13), np.float32(7))])
    return sets


# ------------------------------------------------------------------ transfer functions
def edge_lut(size):
    """A finite LUT of `size` entries whose alphas are distinct and not monotone, so an index
    range off by one entry changes the maximum."""
    i = np.arange(size)
    lut = np.zeros((size, 4), np.float32)
    lut[:, 0] = (i % 3) / 2.0
    lut[:, 1] = 0.5
    lut[:, 2] = 1.0 - lut[:, 0]
    lut[:, 3] = ((i * 37) % size + 1).astype(np.float32) / np.float32(size + 1)
    return _frozen(lut)
