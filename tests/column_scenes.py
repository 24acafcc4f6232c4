"""Inputs and expected answers of the column products, shared by tests/test_column_cpu.py (the
reduction against a NumPy restatement, and the census of these inputs by the oracle alone) and
tests/test_gpu_column.py (irt_column_latlon and irt_render_column on the device, bit for bit).
The scenes are sample_scenes.scene's; the grid answers are oracle.sample_volume at
irt.latlon_points; the expected frames are a restatement of irt_render_column's definition
(include/icon_rt_hip.h, "column products") from the oracle pieces tests/levels_scenes.py uses.
Everything is computed once per process and read-only."""
import functools
from types import SimpleNamespace

import numpy as np

import irt
import levels_scenes as LS
import oracle as O
import sample_scenes as S

F = np.float32
SCENE_NAMES = S.SCENE_NAMES
MISS = -12345.5
OUTPUTS = tuple(irt.COLUMN_OUTPUTS)  # wsum, vmax, vmin, kmax, kmin, count


def _frozen(a):
    a.setflags(write=False)
    return a


# ------------------------------------------------------------------ level sets
@functools.lru_cache(maxsize=None)
def _parts(name):
    """The pieces of a scene's level sets: the layer mid-radii along its thickest column,
    height[0] and the top, one level 500 m below the shell and one above, the duplicated radius."""
    cells = S.scene(name)
    h0, top, _ = S.shell(cells)
    i = int(np.argmax(cells["numLayers"]))
    h = cells["height"][i][:int(cells["numLayers"][i]) + 1].astype(np.float64)
    mids = (0.5 * (h[:-1] + h[1:])).astype(F)
    return SimpleNamespace(h0=h0, top=top, mids=mids, below=F(float(h0) - 500.0), above=F(float(top) + 500.0),
                           dup=mids[(2 * len(mids)) // 3])


@functools.lru_cache(maxsize=None)
def levels(name, which):
    """The radii (float32, in the order given to the calls) of a level set over scene(name):
      one        a layer mid-radius                                      (grid "one")
      five       below the shell, two mid-radii, the first again, the top (grid "five")
      ascending  every mid-radius, height[0] and the top exactly, one level 500 m below the shell
                 and one above, one mid-radius twice -- sorted            (grid "all")
      shuffled   the same list in a shuffled order                        (grid "all")
      render     twelve of the shuffled list, the pair of equal radii and both outside levels
                 among them                                              (irt_render_column)"""
    p = _parts(name)
    m = p.mids
    everything = np.sort(np.concatenate([m, [p.h0, p.top, p.below, p.above, p.dup]]).astype(F))
    if which == "one":
        r = [m[len(m) // 2]]
    elif which == "five":
        r = [p.below, m[len(m) // 4], m[(3 * len(m)) // 4], m[len(m) // 4], p.top]
    elif which == "ascending":
        r = everything
    elif which == "shuffled":
        r = np.random.default_rng(13).permutation(everything)
    elif which == "render":
        pick = m[np.linspace(0, len(m) - 1, 8).astype(int)]
        r = np.random.default_rng(5).permutation(np.concatenate([pick, [p.dup, p.dup, p.below, p.above]]))
    else:
        raise KeyError(which)
    return _frozen(np.array(r, F))


def shuffle_of(name):
    """perm with levels(name, "shuffled") == levels(name, "ascending")[perm]."""
    n = levels(name, "ascending").size
    return np.random.default_rng(13).permutation(n)


# ------------------------------------------------------------------ weights
WEIGHTS = ("none", "ones", "mixed")


@functools.lru_cache(maxsize=None)
def weights(which, n):
    """None, n ones, or n floats uniform in [-1, 2) (products that round) with a negative value
    first and, where the list is longer than two, a 0 in the middle."""
    if which == "none":
        return None
    if which == "ones":
        return _frozen(np.ones(n, F))
    w = np.random.default_rng(n).uniform(-1.0, 2.0, n).astype(F)
    w[0] = F(-0.75)
    if n > 2:
        w[n // 2] = F(0.0)
    return _frozen(w)


# ------------------------------------------------------------------ grids
# (levels, lat, lon): a single point; patch tails in both directions; three patch rows with ragged
# edges.  lat and lon are sample_scenes.grid's (the poles, the date line, an exact 0 in each).
GRIDS = {"one": ("one", (1, 1, 1)), "five": ("five", (2, 7, 9)), "all": ("shuffled", (3, 17, 33)),
         "all_ascending": ("ascending", (3, 17, 33))}
GPU_GRIDS = ("one", "five", "all")


@functools.lru_cache(maxsize=None)
def grid(name, key):
    """(lat, lon, radius) of a grid of GRIDS over scene(name)."""
    which, shape = GRIDS[key]
    lat, lon, _ = S.grid(name, shape)
    return lat, lon, levels(name, which)


@functools.lru_cache(maxsize=None)
def grid_answers(name, key):
    """(found uint8, value float32), each (levels, lat, lon), of oracle.sample_volume(fast=1) at
    irt.latlon_points of grid(name, key)."""
    lat, lon, rad = grid(name, key)
    pts = irt.latlon_points(lat, lon, rad)
    f, v = O.sample_volume(S.scene(name), pts.reshape(-1, 3), fast=1)
    shape = (rad.size, lat.size, lon.size)
    return _frozen((f != 0).astype(np.uint8).reshape(shape)), _frozen(v.reshape(shape))


def reduce_numpy(value, found, weight, miss):
    """The reduction's definition restated in NumPy: an explicit loop over the levels in float32,
    every column at once.  Returns the six outputs, each of shape value.shape[1:]."""
    value = np.asarray(value, F)
    L, shape = value.shape[0], value.shape[1:]
    v = value.reshape(L, -1)
    f = np.asarray(found).reshape(L, -1) != 0
    n = v.shape[1]
    wsum, mx, mn = np.zeros(n, F), np.zeros(n, F), np.zeros(n, F)
    kmax, kmin, count = np.full(n, -1, np.int32), np.full(n, -1, np.int32), np.zeros(n, np.int32)
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(L):
            w = F(1.0) if weight is None else F(weight[k])
            wv = (w * v[k]).astype(F)
            first, later = f[k] & (count == 0), f[k] & (count > 0)
            lt, gt = later & (v[k] < mn), later & (v[k] > mx)
            mn = np.where(first | lt, v[k], mn)
            kmin = np.where(first | lt, k, kmin).astype(np.int32)
            mx = np.where(first | gt, v[k], mx)
            kmax = np.where(first | gt, k, kmax).astype(np.int32)
            wsum = np.where(first, wv, np.where(later, (wsum + wv).astype(F), wsum)).astype(F)
            count = count + f[k].astype(np.int32)
    none = count == 0
    for a in (wsum, mx, mn):
        a[none] = F(miss)
    out = dict(wsum=wsum, vmax=mx, vmin=mn, kmax=kmax, kmin=kmin, count=count)
    return {k: a.reshape(shape) for k, a in out.items()}


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == F else a.view(np.int32)


def same_outputs(a, b, which=OUTPUTS):
    """The name of the first output of `which` whose bits differ between two results, or None."""
    for k in which:
        if a[k].shape != b[k].shape or not np.array_equal(bits(a[k]), bits(b[k])):
            return k
    return None


@functools.lru_cache(maxsize=None)
def reduced(name, key, wname, miss=MISS):
    """The expected outputs of irt_column_latlon on grid(name, key) with weights(wname):
    irt.column_reduce of the oracle's grid answers -- which must be the NumPy restatement's, bit for
    bit (asserted here, so that everything downstream rests on both)."""
    f, v = grid_answers(name, key)
    w = weights(wname, v.shape[0])
    got = irt.column_reduce(v, f, w, miss)
    want = reduce_numpy(v, f, w, miss)
    assert same_outputs(got, want) is None, f"irt_column_reduce differs from NumPy in {same_outputs(got, want)}"
    return {k: _frozen(a) for k, a in got.items()}


# ------------------------------------------------------------------ irt_render_column
PRODUCTS = {"wsum": irt.COLUMN_WSUM, "max": irt.COLUMN_MAX, "min": irt.COLUMN_MIN}
VALUE_RANGE = (-3.0, 10.0)  # holds every product of FRAMES: the weighted sums reach from -2.5 to 9.3


@functools.lru_cache(maxsize=None)
def transfunc(name):
    """(lut, value range, opacityScale) of the frames: levels_scenes' translucent table (every
    alpha in (0, 0.5), so the product's value shows in A as in C) over VALUE_RANGE, so that the
    sums classify to more than the table's two ends."""
    lut, _, scale = LS.transfunc(name, "translucent")
    return lut, VALUE_RANGE, scale


def surface(name):
    """The sphere the product is drawn on: 80 % up the shell, so the "inside" camera (mid-shell)
    is inside it and sees its far hits, the "outside" camera its near hits."""
    p = _parts(name)
    return F(float(p.h0) + 0.8 * (float(p.top) - float(p.h0)))


def render_weights(name, wname):
    return weights(wname, levels(name, "render").size)


@functools.lru_cache(maxsize=None)
def column_samples(name, view_name, size, accum_id, mode=irt.MODE_USER_GEOM):
    """The part of a frame that does not depend on the product or the weights: per pixel the ray,
    the hit slot (near when tn > 0, else far when tf > 0), P, len, and per level the column point
    and the sampler's answer there.  found / value are (levels, H, W)."""
    W, H = LS.SIZES[size]
    lp = LS.launch_params(name, view_name, size, accum_id, mode)
    org = lp.camera12()[0:3]
    d = LS.rays(lp, W, H)
    hit, tn, tf = LS.sphere_hits(org, d, surface(name))
    near = tn > 0
    live = hit & (near | (tf > 0))
    t = np.where(near, tn, tf).astype(F)
    P = (org[None, None, :] + d * t[..., None]).astype(F)
    ln = np.sqrt((P[..., 0] * P[..., 0] + P[..., 1] * P[..., 1]) + P[..., 2] * P[..., 2])
    assert ln.dtype == F
    radii = levels(name, "render")
    found = np.zeros((radii.size, H, W), np.uint8)
    value = np.zeros((radii.size, H, W), F)
    points = np.zeros((radii.size, H, W, 3), F)
    with np.errstate(divide="ignore", invalid="ignore"):
        for k, r in enumerate(radii):
            s = (F(r) / ln).astype(F)
            points[k] = (P * s[..., None]).astype(F)
            if live.any():
                fk, vk = LS.sample(S.scene(name), mode, points[k][live])
                found[k][live], value[k][live] = fk, vk
    return SimpleNamespace(lp=lp, live=live, near=near, found=_frozen(found), value=_frozen(value),
                           points=_frozen(points), W=W, H=H)


@functools.lru_cache(maxsize=None)
def expected_frame(name, view_name, size, accum_id, product, wname, mode=irt.MODE_USER_GEOM, miss=MISS):
    """One frame of irt_render_column by the restatement: .value (H, W), .accum (H, W, 4), .fb, and
    .columns (the six outputs per pixel) -- onto zero accum for accumID 0, onto LS.prior_accum
    otherwise."""
    c = column_samples(name, view_name, size, accum_id, mode)
    lp, W, H = c.lp, c.W, c.H
    col = reduce_numpy(c.value, c.found, render_weights(name, wname), miss)
    v = col[{"wsum": "wsum", "max": "vmax", "min": "vmin"}[product]]
    has = col["count"] > 0
    s4 = np.zeros((H, W, 4), F)
    s4[has] = LS.classify(transfunc(name), v[has])
    a = np.where(s4[..., 3] < 0, F(0), np.where(s4[..., 3] > 1, F(1), s4[..., 3])).astype(F)
    amb, rad = np.array(lp.ambientColor.tolist(), F), F(lp.ambientRadiance)
    C = (a[..., None] * ((s4[..., :3] * amb) * rad)).astype(F)
    colour = np.concatenate([C, a[..., None]], -1).astype(F)
    colour[~has] = 0
    prior = LS.prior_accum(W, H) if accum_id else np.zeros((H, W, 4), F)
    accum = LS.lerp(colour, prior, accum_id)
    return SimpleNamespace(value=v, columns=col, colour=colour, accum=accum, fb=LS.pixels(accum), samples=c)


# The frames both test files walk: (scene, view, size, accumID, product, weights).  Between them:
# both scenes, both cameras, both sizes, accumID 0 and 3, all three products, all three weights.
FRAMES = (
    ("flat", "outside", "odd", 0, "wsum", "mixed"),
    ("flat", "inside", "odd", 3, "max", "none"),
    ("flat", "outside", "packet", 0, "min", "ones"),
    ("terrain", "outside", "odd", 3, "wsum", "none"),
    ("terrain", "inside", "odd", 0, "max", "mixed"),
    ("terrain", "inside", "packet", 3, "min", "mixed"),
)
# ... and one through a sampler other than the cell sampler (the wedge scan: a small frame)
SAMPLER_FRAME = ("flat", "outside", "packet", 0, "wsum", "mixed")


def frame_id(c):
    return "-".join(str(x) for x in c)
