"""Inputs and the expected answer of irt_render_levels, shared by tests/test_levels_cpu.py (the
census of these inputs by the restatement alone) and tests/test_gpu_levels.py (the device against
it, bit for bit).  The expected answer is a plain restatement of the call's definition
(include/icon_rt_hip.h, "level surfaces") from oracle pieces: the rays in numpy float32, operation
for operation as irt_raygen.h gen_ray (oracle_lcg's two draws, the v jitter first); the hits by
oracle_intersect_sphere; the values by oracle.sample_volume(fast=1), wedge_sample_points and
triangle_sample_points; oracle_post_classify; the compositing in numpy float32 in the header's
order; oracle_linear_to_srgb and oracle_make_rgba.  Everything is computed once per process and
read-only."""
import ctypes as C
import functools
from types import SimpleNamespace

import numpy as np

import helpers
import irt
import oracle as O
import sample_scenes as S

F = np.float32
SCENE_NAMES = ("flat", "terrain", "filtered")
SIZES = {"odd": (37, 29), "packet": (8, 8)}  # 37 x 29: packets cut by both frame edges
AMBIENT = ((0.9, 0.8, 0.7), 1.25)            # ambientColor, ambientRadiance: products that round
MISS = -12345.5


# ------------------------------------------------------------------ views
VIEWS = {"outside": "framing",        # the globe framed from outside
         "inside": "shell_horizon",   # |org| = mid-shell: strictly between levels_of's inside levels
         "under": "underground"}      # half of height[0]: inside every sphere


@functools.lru_cache(maxsize=None)
def view(name, view_name):
    return helpers.view_battery(S.scene(name))[VIEWS[view_name]]


# ------------------------------------------------------------------ level sets
@functools.lru_cache(maxsize=None)
def levels_of(name, which):
    """The radii (float32, in the order given to the call) of a level set over scene(name)."""
    cells = S.scene(name)
    h0, top, inner = (float(v) for v in S.shell(cells))
    i = int(np.argmax(cells["numLayers"]))
    k = int(cells["numLayers"][i]) // 2
    mid_layer = 0.5 * (float(cells["height"][i][k]) + float(cells["height"][i][k + 1]))
    at = lambda f: h0 + f * (top - h0)  # noqa: E731
    sets = {
        "inner": [inner],                    # a layer boundary strictly inside the shell
        "midlayer": [mid_layer],             # between two layer boundaries
        # unsorted: one below height[0], two inside (either side of mid-shell), one above the top
        "four": [at(0.7), h0 - 2000.0, top + 2000.0, at(0.3)],
        "dup": [at(0.6), at(0.25), at(0.6)],  # a duplicated radius
        "sixteen": list(np.random.default_rng(16).permutation(np.linspace(h0 - 1000.0, top + 1000.0, 16))),
    }
    r = np.array(sets[which], F)
    r.setflags(write=False)
    return r


# ------------------------------------------------------------------ transfer functions
@functools.lru_cache(maxsize=None)
def transfunc(name, which):
    """(lut (300, 4), value range, opacityScale)."""
    setup = irt.setup_frame(S.scene(name), 8, 8)
    lut = np.array(setup.lut, F, copy=True)
    scale = 1.0
    if which == "scale3":  # the clamp of a acts
        scale = 3.0
    elif which == "translucent":  # every alpha in (0, 0.5): levels show through each other
        lut[:, 3] = F(0.08) + F(0.35) * np.linspace(0, 1, len(lut), dtype=F)
    elif which == "opaque":  # alpha 1 everywhere: the first found slot is the picture
        lut[:, 3] = F(1.0)
    elif which != "default":
        raise KeyError(which)
    lut.setflags(write=False)
    return lut, (float(setup.value_range[0]), float(setup.value_range[1])), scale


def launch_params(name, view_name, size, accum_id=0, mode=irt.MODE_USER_GEOM):
    W, H = SIZES[size]
    lp = irt.setup_frame(S.scene(name), W, H, camera=view(name, view_name)).lp
    lp.accumID = accum_id
    lp.ambientColor = irt.Vec3(*AMBIENT[0])
    lp.ambientRadiance = AMBIENT[1]
    lp.mode = mode
    return lp


# ------------------------------------------------------------------ the restatement
def rays(lp, W, H):
    """gen_ray (irt_raygen.h; generateRay, deviceCode.cu:36-49, with Random rnd(accumID*W*H + x, y),
    288-291) of every pixel in float32: unit directions (H, W, 3)."""
    L = O.olib()
    cam = lp.camera12()
    d00, du, dv = cam[3:6], cam[6:9], cam[9:12]
    jit = np.zeros((H, W, 2), F)
    two = np.zeros(2, F)
    for y in range(H):
        for x in range(W):
            L.oracle_lcg((lp.accumID * W * H + x) & 0xFFFFFFFF, y, 2, two.ctypes.data)
            jit[y, x] = two  # {jv, ju}: the dir_dv jitter is drawn first
    ys, xs = np.mgrid[0:H, 0:W]
    a = (xs.astype(F) + F(0.5)) + jit[..., 1]
    b = (ys.astype(F) + F(0.5)) + jit[..., 0]
    d = np.stack([(d00[k] + a * du[k]) + b * dv[k] for k in range(3)], -1).astype(F)
    ln = np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])
    d = d / ln[..., None]
    d = np.where(np.abs(d) < F(1e-5), F(1e-5), d)
    assert d.dtype == F
    return d


def sphere_hits(org, dirs, radius):
    """oracle_intersect_sphere of every ray: (hit bool, tnear, tfar), each (H, W)."""
    L = O.olib()
    H, W, _ = dirs.shape
    hit = np.zeros((H, W), bool)
    tn, tf = np.zeros((H, W), F), np.zeros((H, W), F)
    a, b = C.c_float(), C.c_float()
    o = O.v3(org)
    for y in range(H):
        for x in range(W):
            if L.oracle_intersect_sphere(o, O.v3(dirs[y, x]), float(radius), C.byref(a), C.byref(b)):
                hit[y, x], tn[y, x], tf[y, x] = True, a.value, b.value
    return hit, tn, tf


def slot_order(radii):
    """near[]: the level indices by descending radius, ties by ascending index; far[] reversed."""
    near = sorted(range(len(radii)), key=lambda i: (-float(radii[i]), i))
    return near, near[::-1]


def sample(cells, mode, pts):
    """(found bool, value) at pts (n, 3): the guard of irt_sample_points (a point whose float
    squared length is not finite and positive is a miss), then the mode's oracle sampler."""
    pts = np.ascontiguousarray(pts, F).reshape(-1, 3)
    with np.errstate(over="ignore", invalid="ignore"):
        r2 = (pts[:, 0] * pts[:, 0] + pts[:, 1] * pts[:, 1]) + pts[:, 2] * pts[:, 2]
    ok = (r2 > 0) & (r2 < np.inf)
    found, value = np.zeros(len(pts), bool), np.zeros(len(pts), F)
    if ok.any():
        entry = {irt.MODE_USER_GEOM: lambda c, p: O.sample_volume(c, p, fast=1),
                 irt.MODE_CUBQL: O.wedge_sample_points, irt.MODE_TRIANGLES: O.triangle_sample_points}[mode]
        f, v = entry(cells, pts[ok])
        found[ok], value[ok] = f != 0, v
    return found, value


def classify(tf, values):
    """oracle_post_classify of each value: (n, 4) float32."""
    lut, vr, scale = tf
    lut = np.ascontiguousarray(lut, F)
    out = np.zeros((len(values), 4), F)
    one = np.zeros(4, F)
    L = O.olib()
    for i, v in enumerate(values):
        L.oracle_post_classify(lut.ctypes.data, len(lut), vr[0], vr[1], scale, float(v), one.ctypes.data)
        out[i] = one
    return out


def pixels(accum):
    """fb = make_rgba(linear_to_srgb(accum)) (deviceCode.cu:336-340) of accum (H, W, 4)."""
    L = O.olib()
    H, W, _ = accum.shape
    fb = np.zeros((H, W), np.uint32)
    c = np.zeros(4, F)
    for y in range(H):
        for x in range(W):
            for k in range(3):
                c[k] = L.oracle_linear_to_srgb(float(accum[y, x, k]))
            c[3] = accum[y, x, 3]
            fb[y, x] = L.oracle_make_rgba(c.ctypes.data)
    return fb


def lerp(colour, prior, accum_id):
    """accum = w * colour + (1 - w) * prior with w = 1 / (accumID + 1), in float32."""
    w = F(1.0) / F(accum_id + 1)
    out = w * colour.astype(F) + (F(1.0) - w) * prior.astype(F)
    assert out.dtype == F
    return out


def prior_accum(W, H):
    """A non-zero accum for frames with accumID > 0 to lerp onto."""
    return np.random.default_rng(7).uniform(0.0, 1.0, (H, W, 4)).astype(F)


def composite(cells, lp, W, H, radii, tf, back, mode=irt.MODE_USER_GEOM, miss=MISS):
    """The definition, slot by slot.  Returns colour (H, W, 4) = (C, A), value, level, and per slot
    the census' facts: live, found, contributes (w != 0), far, outside (the camera is outside the
    slot's sphere: its near slot is live), clamped (the clamp changed a), points."""
    radii = np.asarray(radii, F)
    n = len(radii)
    org = lp.camera12()[0:3]
    amb, rad = np.array(lp.ambientColor.tolist(), F), F(lp.ambientRadiance)
    d = rays(lp, W, H)
    near, far = slot_order(radii)
    hits = {i: sphere_hits(org, d, radii[i]) for i in set(near)}
    Cc = np.zeros((H, W, 3), F)
    A = np.zeros((H, W), F)
    value = np.full((H, W), miss, F)
    level = np.full((H, W), -1, np.int32)
    slots = []
    for s in range(2 * n):
        is_far = s >= n
        i = far[s - n] if is_far else near[s]
        hit, tn, tf_ = hits[i]
        near_live = hit & (tn > 0)
        live = hit & (tf_ > 0) & (np.bool_(back) | ~near_live) if is_far else near_live
        t = tf_ if is_far else tn
        P = (org[None, None, :] + d * t[..., None]).astype(F)
        found = np.zeros((H, W), bool)
        v = np.zeros((H, W), F)
        found[live], v[live] = sample(cells, mode, P[live])
        s4 = np.zeros((H, W, 4), F)
        s4[found] = classify(tf, v[found])
        a = np.where(s4[..., 3] < 0, F(0), np.where(s4[..., 3] > 1, F(1), s4[..., 3])).astype(F)
        c = (s4[..., :3] * amb) * rad
        w = np.where(found, (F(1) - A) * a, F(0)).astype(F)
        Cc = np.where(found[..., None], Cc + w[..., None] * c, Cc).astype(F)
        A = np.where(found, A + w, A).astype(F)
        first = found & (level < 0)
        value[first] = v[first]
        level[first] = i
        slots.append(SimpleNamespace(index=i, far=is_far, live=live, found=found, contributes=found & (w != 0),
                                     outside=near_live, clamped=found & (a != s4[..., 3]), points=P, t=t))
    return SimpleNamespace(colour=np.concatenate([Cc, A[..., None]], -1).astype(F), value=value, level=level,
                           slots=slots, dirs=d, org=org)


@functools.lru_cache(maxsize=None)
def expected(name, view_name, levels, tf_name, size, back, accum_id=0, mode=irt.MODE_USER_GEOM):
    """One frame of irt_render_levels by the restatement: .accum, .fb, .value, .level (and
    composite's .slots) -- onto zero accum for accumID 0, onto prior_accum otherwise."""
    W, H = SIZES[size]
    lp = launch_params(name, view_name, size, accum_id, mode)
    r = composite(S.scene(name), lp, W, H, levels_of(name, levels), transfunc(name, tf_name), back, mode)
    prior = prior_accum(W, H) if accum_id else np.zeros((H, W, 4), F)
    r.accum = lerp(r.colour, prior, accum_id)
    r.fb = pixels(r.accum)
    return r


# The frames both test files walk: (scene, view, level set, transfer function, size, back, accumID).
# Between them: every scene, view, level set, transfer function and size of the issue's list, BACK
# on and off, and accumID 3 onto a non-zero accum.
CASES = (
    ("flat", "outside", "four", "translucent", "odd", False, 0),
    ("flat", "outside", "four", "translucent", "odd", True, 0),
    ("flat", "outside", "inner", "default", "packet", False, 0),
    ("flat", "inside", "four", "scale3", "odd", True, 3),
    ("flat", "under", "sixteen", "translucent", "odd", False, 0),
    ("flat", "outside", "dup", "translucent", "odd", True, 3),
    ("terrain", "outside", "four", "default", "odd", True, 0),
    ("terrain", "inside", "midlayer", "scale3", "odd", False, 3),
    ("terrain", "under", "dup", "translucent", "packet", False, 0),
    ("filtered", "outside", "sixteen", "translucent", "odd", True, 0),
    ("filtered", "inside", "four", "default", "odd", False, 0),
    ("filtered", "under", "inner", "scale3", "odd", False, 0),
)


def case_id(c):
    return "-".join(str(x) for x in c[:5]) + ("-back" if c[5] else "") + f"-a{c[6]}"
