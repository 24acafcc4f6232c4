"""Fields, grids and an independent restatement of the isolines' definition (include/icon_rt_hip.h,
"isolines"), shared by tests/test_contour_cpu.py (irt_contour_cells against the restatement, the
census, the properties) and tests/test_gpu_contour.py (the device against irt_contour_cells).  The
restatement is float64 NumPy + - * / sqrt, written from the header's text; those are IEEE operations,
so equality is by bits.  cos and sin come from math.cos / math.sin, the C library's, as the header
says (NumPy's own vectorised cos may differ in the last bit).  Everything is computed once per process
and read-only.

The sizes.  The count and emit kernels take 256 cells per workgroup and the scan's one workgroup has
256 threads (4 entries each per round):
 - `smooth` is 37 x 67 wrapped, 36 * 67 = 2,412 cells: no multiple of 64 or 256, 10 workgroups.  (A
   wrapped grid needs at least 63 columns, 2 pi / 0.1: the 53 columns first thought of cannot close
   within the 0.1 rad step limit.  That 37 x 53 grid is kept as `smooth53`, legal without wrap and a
   refusal with it.)
 - `wide` is 200 x 400 wrapped, 199 * 400 = 79,600 cells: 311 workgroups, more than the scan's 256
   threads, and 16 * 311 = 4,976 totals, five rounds of the scan.
"""
import functools
import math

import numpy as np

import irt

F = np.float32
D = np.float64


def frozen(a):
    a.setflags(write=False)
    return a


def trig(x):
    """(cos, sin) of float32 radians in float64, by the C library."""
    x = np.asarray(x, F)
    return (np.array([math.cos(float(v)) for v in x], D), np.array([math.sin(float(v)) for v in x], D))


def corners(lat, lon):
    """The unit vectors (cl*co, cl*si, sl) of every grid point: (numLat, numLon, 3) float64."""
    cl, sl = trig(lat)
    co, si = trig(lon)
    p = np.empty((len(cl), len(co), 3), D)
    p[..., 0] = cl[:, None] * co[None, :]
    p[..., 1] = cl[:, None] * si[None, :]
    p[..., 2] = sl[:, None] * np.ones_like(co)[None, :]
    return p


def grid(num_lat, num_lon, wrap, lat_range=(-1.5, 1.5)):
    lat = np.linspace(lat_range[0], lat_range[1], num_lat).astype(F)
    if wrap:
        lon = (np.arange(num_lon) * (2.0 * np.pi / num_lon) - np.pi + 0.01).astype(F)
    else:
        lon = (np.arange(num_lon) * 0.1 * 0.999 - 2.6).astype(F)
    return lat, lon


def smooth_values(lat, lon):
    p = corners(lat, lon)
    return (p[..., 2] + 0.3 * p[..., 0] * p[..., 1]).astype(F)


class Field:
    def __init__(self, name, lat, lon, value, found, thresholds, styles, wraps):
        self.name, self.wraps = name, tuple(wraps)  # the wrap settings that are legal
        self.lat, self.lon = frozen(np.asarray(lat, F)), frozen(np.asarray(lon, F))
        self.value = frozen(np.ascontiguousarray(value, F))
        self.found = None if found is None else frozen(np.ascontiguousarray(found, np.uint8))
        self.thresholds = frozen(np.asarray(thresholds, F))
        self.styles = frozen(np.asarray(styles, np.int32))
        assert self.value.shape == (self.lat.size, self.lon.size) and self.styles.size == self.thresholds.size


def _styles(n):
    return np.arange(n) % irt.OVERLAY_MAX_STYLES


SMOOTH_T = (-0.6, 0.0, 0.35, 0.8)


@functools.lru_cache(maxsize=None)
def field(name):
    if name in ("smooth", "smooth53"):
        lat, lon = grid(37, 67, True) if name == "smooth" else grid(37, 53, False)
        return Field(name, lat, lon, smooth_values(lat, lon), None, SMOOTH_T, _styles(4),
                     (False, True) if name == "smooth" else (False,))
    if name == "checker":
        # +-1 alternating plus 1e-3 per row: every cell a saddle whose centre value is (2 j + 1) * 5e-4;
        # thresholds on both sides of the centres take both branches of mask 5 and of mask 10
        lat, lon = grid(12, 16, False, (-0.5, 0.5))
        j, i = np.meshgrid(np.arange(12), np.arange(16), indexing="ij")
        v = (np.where((i + j) % 2 == 0, 1.0, -1.0) + 1e-3 * j).astype(F)
        return Field(name, lat, lon, v, None, (-0.25, 0.0052, 0.25, 0.5), _styles(4), (False,))
    if name == "holes":
        f = field("smooth")
        found = np.ones(f.value.shape, np.uint8)
        found[5:9, 10:14] = 0      # a block
        found[20:22, 40:47] = 0    # another, across isolines
        found[15, 66] = 0          # in the wrap column
        v = f.value.copy()
        v[30, 5] = np.nan
        v[12, 33] = np.inf
        v[18, 0] = -np.inf
        return Field(name, f.lat, f.lon, v, found, SMOOTH_T, _styles(4), (False, True))
    if name == "oncorner":
        # integers, thresholds equal to grid values: crossings at t = 0 and t = 1, dropped segments, and a
        # constant region equal to the threshold 2
        lat, lon = grid(9, 11, False, (-0.36, 0.36))
        j, i = np.meshgrid(np.arange(9), np.arange(11), indexing="ij")
        v = ((i * 3 + j * 5) % 7).astype(F)
        v[2:6, 2:6] = 2.0
        v[7, 8] = 9.0  # a strict peak: threshold 9 crosses at this corner alone in its four cells
        return Field(name, lat, lon, v, None, (2.0, 3.0, 9.0, 0.0, 6.0), _styles(5), (False,))
    if name == "poles":
        # lat[0] = -pi/2 and lat[-1] = +pi/2 as floats: every point of a pole row is (nearly) the pole.  The
        # values along a pole row differ (a component of a vector field does there), and thresholds equal to
        # such a row's strict maximum give crossings at that shared corner: dropped segments on a pole row
        lat = np.linspace(-0.5 * np.pi, 0.5 * np.pi, 33).astype(F)
        lon = grid(33, 64, True)[1]
        assert lat[0] == F(-np.pi / 2) and lat[-1] == F(np.pi / 2)
        p = corners(lat, lon)
        v = (p[..., 2] + 0.3 * p[..., 0] * p[..., 1] + 0.05 * np.cos(lon.astype(D) - 0.3)[None, :]).astype(F)
        thr = (-0.5, 0.2, float(v[0].max()), float(v[-1].max()))
        return Field(name, lat, lon, v, None, thr, _styles(4), (False, True))
    if name == "tiny1":  # one cell
        lat, lon = np.array([0.1, 0.15], F), np.array([0.3, 0.38], F)
        return Field(name, lat, lon, np.array([[0.0, 1.0], [2.0, 4.0]], F), None, (1.5, 0.5, 3.5), _styles(3), (False,))
    if name == "tiny3x5":  # 8 cells: under one wave
        lat, lon = grid(3, 5, False, (-0.08, 0.08))
        return Field(name, lat, lon, smooth_values(lat, lon) * F(10), None, (1.0, 1.3, 1.7), _styles(3), (False,))
    if name == "wide":
        lat, lon = grid(200, 400, True)
        thr = np.linspace(-0.9, 0.9, 16)
        return Field(name, lat, lon, smooth_values(lat, lon), None, thr, _styles(16), (False, True))
    raise KeyError(name)


FIELDS = ("smooth", "smooth53", "checker", "holes", "oncorner", "poles", "tiny1", "tiny3x5", "wide")
CASES = tuple((n, w) for n in FIELDS for w in field(n).wraps)
CASE_IDS = tuple(f"{n}-{'wrap' if w else 'open'}" for n, w in CASES)

# first edge, second edge per mask (the header's table)
PAIRS = {1: (0, 3), 2: (1, 0), 3: (1, 3), 4: (2, 1), 6: (2, 0), 7: (2, 3), 8: (3, 2), 9: (0, 2), 11: (1, 2),
         12: (3, 1), 13: (0, 1), 14: (3, 0)}
SADDLES = {(5, True): ((0, 1), (2, 3)), (5, False): ((0, 3), (2, 1)),
           (10, True): ((1, 2), (3, 0)), (10, False): ((1, 0), (3, 2))}
EDGES = ((0, 1), (1, 2), (3, 2), (0, 3))  # from -> to corner


def length(v):
    return np.sqrt((v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2])


class Restated:
    """The restatement's answer: segments (SEGMENT_DTYPE, in output order), per (counts per threshold),
    cell (each segment's cell index) and the census facts."""


@functools.lru_cache(maxsize=None)
def restate(name, wrap):
    f = field(name)
    nlat, nlon = f.value.shape
    cells_lon = nlon if wrap else nlon - 1
    P = corners(f.lat, f.lon)
    j, i = np.meshgrid(np.arange(nlat - 1), np.arange(cells_lon), indexing="ij")
    j, i = j.ravel(), i.ravel()
    i1 = (i + 1) % nlon
    at = ((j, i), (j, i1), (j + 1, i1), (j + 1, i))
    v = [f.value[a] for a in at]           # float32
    p = [P[a] for a in at]                 # float64 (cells, 3)
    ok = np.ones(j.size, bool)
    for k in range(4):
        ok &= np.isfinite(v[k])
        if f.found is not None:
            ok &= f.found[at[k]] != 0
    out = Restated()
    parts, cells, per = [], [], []
    out.masks, out.saddles, out.dropped, out.suppressed = set(), set(), 0, 0
    for c, style in zip(f.thresholds, f.styles):
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            b = [vk >= c for vk in v]
            mask = sum(b[k].astype(np.int64) << k for k in range(4))
            E = np.zeros((j.size, 4, 3), D)
            for e, (ca, cb) in enumerate(EDGES):
                t = (D(c) - v[ca].astype(D)) / (v[cb].astype(D) - v[ca].astype(D))
                q = p[ca] + t[:, None] * (p[cb] - p[ca])
                E[:, e] = q / length(q)[:, None]
            m = ((v[0] + v[1]) + (v[2] + v[3])) * F(0.25)
            assert m.dtype == F
            hi = m >= c
        first = np.zeros((j.size, 2), np.int64)
        second = np.zeros((j.size, 2), np.int64)
        valid = np.zeros((j.size, 2), bool)
        for mk, (e0, e1) in PAIRS.items():
            sel = ok & (mask == mk)
            first[sel, 0], second[sel, 0], valid[sel, 0] = e0, e1, True
        for (mk, h), pairs in SADDLES.items():
            sel = ok & (mask == mk) & (hi == h)
            if sel.any():
                out.saddles.add((mk, h))
            for k, (e0, e1) in enumerate(pairs):
                first[sel, k], second[sel, k], valid[sel, k] = e0, e1, True
        out.masks |= set(int(x) for x in np.unique(mask[ok])) - {0, 15}
        out.suppressed += int((~ok & (mask != 0) & (mask != 15)).sum())
        rows = np.arange(j.size)[:, None]
        Pa, Pb = E[rows, first], E[rows, second]          # (cells, 2, 3)
        same = (Pa.astype(F) == Pb.astype(F)).all(-1)
        out.dropped += int((valid & same).sum())
        keep = valid & ~same
        cell = np.broadcast_to(rows, keep.shape)[keep]     # row-major: cell, then the order within it
        a, bb = Pa[keep], Pb[keep]
        n = np.stack([a[:, 1] * bb[:, 2] - a[:, 2] * bb[:, 1], a[:, 2] * bb[:, 0] - a[:, 0] * bb[:, 2],
                      a[:, 0] * bb[:, 1] - a[:, 1] * bb[:, 0]], -1)
        d = bb - a
        ld = length(d)
        seg = np.zeros(len(a), irt.SEGMENT_DTYPE)
        seg["a"], seg["b"] = a.astype(F), bb.astype(F)
        seg["n"] = (n / length(n)[:, None]).astype(F)
        seg["t"] = (d / ld[:, None]).astype(F)
        seg["sinHalf"] = (0.5 * ld).astype(F)
        seg["style"] = style
        parts.append(seg)
        cells.append(cell)
        per.append(len(seg))
    out.segments = frozen(np.concatenate(parts))
    out.cell = frozen(np.concatenate(cells))
    out.per = frozen(np.array(per, np.int64))
    out.cells_lon = cells_lon
    return out


def host(name, wrap):
    """irt_contour_cells of the field: (segments, counts per threshold)."""
    return _host(name, bool(wrap))


@functools.lru_cache(maxsize=None)
def _host(name, wrap):
    f = field(name)
    seg, per = irt.contour_cells(f.value, f.found, f.lat, f.lon, f.thresholds, f.styles, wrap, return_counts=True)
    return frozen(seg), frozen(per)


def same_bytes(got, want, what):
    """Segment arrays equal byte for byte, with the first difference named."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.size == want.size, f"{what}: {got.size} segments, expected {want.size}"
    g, w = got.view(np.uint32).reshape(-1, 16), want.view(np.uint32).reshape(-1, 16)
    bad = np.argwhere(g != w)
    assert len(bad) == 0, (f"{what}: {len(np.unique(bad[:, 0]))} of {len(g)} segments differ, first segment "
                           f"{bad[0][0]} word {bad[0][1]}: {hex(int(g[tuple(bad[0])]))} vs {hex(int(w[tuple(bad[0])]))}")
