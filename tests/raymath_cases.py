"""Case generators of the raygen's per-value arithmetic, shared by tests/test_raymath_cpu.py,
tests/test_gpu_raymath.py and tests/golden/make_golden.py (kats_raymath.npz): operands of the two
division shortcuts, transfer functions with the values to classify under each, rays for the box and
sphere tests, gen_ray's cameras and the shell grid's coordinates.  Deterministic: seeded numpy only.
"""
import numpy as np

F = np.float32
FLT_MAX = F(3.4028234663852886e38)
FLT_MIN = F(1.1754943508222875e-38)
SEED = 20261021
INT_MIN = -2 ** 31


def f32(x):
    return np.ascontiguousarray(x, dtype=np.float32)


def ulps(x, k):
    """The float32 k steps from x (towards +inf for k > 0)."""
    x = f32(x).copy()
    for _ in range(abs(k)):
        x = np.nextafter(x, F(np.inf) if k > 0 else F(-np.inf))
    return x


def around(x, reach=2):
    """x with its neighbours at +-1 .. +-reach ulps."""
    x = f32(x).ravel()
    return np.concatenate([ulps(x, k) for k in range(-reach, reach + 1)])


# ------------------------------------------------------------------------------- divisions
def div_ties():
    """Quotients that are exact ties between two subnormal floats: a = B odd 2^(k-150), b = B 2^k for
    odd B < 4096, odd = 1, 3 .. 31 and k in {1, 2, 5, 20}: a / b = odd 2^-150.  131,072 pairs."""
    B, odd, k = np.meshgrid(np.arange(1, 4096, 2, dtype=np.float64), np.arange(1, 32, 2, dtype=np.float64),
                            np.array([1, 2, 5, 20], np.float64), indexing="ij")
    a = np.ldexp(B * odd, (k - 150).astype(np.int64))
    b = np.ldexp(B, k.astype(np.int64))
    a32, b32 = f32(a).ravel(), f32(b).ravel()
    assert np.array_equal(a32.astype(np.float64), a.ravel()) and np.array_equal(b32.astype(np.float64), b.ravel())
    return a32, b32


def unfixed_product(a, b):
    """(float)((double)a * (1.0 / (double)b)): the double product without the subnormal guard."""
    with np.errstate(all="ignore"):
        return (f32(a).astype(np.float64) * (1.0 / f32(b).astype(np.float64))).astype(np.float32)


def div_near_midpoints(count=3000):
    """Normal-range worst cases: for odd 24-bit B, M = (-+B)^-1 mod 2^25 and A = (B M +- 1) / 2^25 with
    M in [2^24, 2^25), A in [2^23, 2^24): A / B = M / 2^25 +- 1 / (B 2^25), about 2^-48 (relative) from
    the midpoint M / 2^25 of the 24-bit grid.  Several exponents, both signs."""
    rng = np.random.default_rng(SEED)
    As, Bs = [], []
    for B in (rng.integers(1 << 22, 1 << 23, count) * 2 + 1).tolist():
        for sign in (1, -1):
            M = pow(-sign * B, -1, 1 << 25)
            A, rem = divmod(B * M + sign, 1 << 25)
            assert rem == 0
            if (1 << 24) <= M < (1 << 25) and (1 << 23) <= A < (1 << 24):
                As.append(A)
                Bs.append(B)
    A, B = np.array(As, np.float64), np.array(Bs, np.float64)
    a, b = [], []
    for ea, eb, sa, sb in ((-23, -23, 1, 1), (0, -23, -1, 1), (40, -30, 1, -1), (-60, 20, -1, -1), (-100, -90, 1, 1),
                           (60, 75, 1, 1), (-23, 80, 1, 1)):
        a.append(sa * np.ldexp(A, ea))
        b.append(sb * np.ldexp(B, eb))
    return f32(np.concatenate(a)), f32(np.concatenate(b))


def div_pairs():
    """Every division pair (a, b): name -> (a, b)."""
    rng = np.random.default_rng(SEED + 1)
    out = {"ties": div_ties(), "near_midpoints": div_near_midpoints()}
    ta, tb = out["ties"]
    out["ties_signed"] = (-ta[::16].copy(), tb[::16].copy())
    # divisors at recip_ok's limits, a subnormal, zeros, infinities, NaN -- against every numerator
    bs = np.concatenate([around(F(2.0 ** -100), 1), around(F(2.0 ** 100), 1), f32([1e-40, 0.0, -0.0, np.inf, -np.inf,
                                                                                   np.nan, 1.0, -3.0, 98.0])])
    bs = np.concatenate([bs, -bs[:6]])
    an = f32([0.0, -0.0, 1.0, -1.0, 3.0, 1e-45, -1e-45, FLT_MIN, FLT_MAX, -FLT_MAX, 1e-30, 7e30, np.inf, -np.inf, np.nan,
              0.1, 147 * 2.0 ** -149])
    g = np.meshgrid(an, bs)
    out["special"] = (f32(g[0].ravel()), f32(g[1].ravel()))
    # quotients at the overflow boundary: a = FLT_MAX b and its neighbours, |b| < 1
    n = 2000
    b = f32(rng.uniform(0.5, 1.0, n) * 2.0 ** rng.integers(-20, 1, n))
    b[::2] = -b[::2]
    a0 = f32(np.float64(FLT_MAX) * b.astype(np.float64))
    out["overflow"] = (around(a0), np.tile(b, 5))
    # ... and at the boundary between normal and subnormal quotients: a = FLT_MIN b, b >= 1
    b = f32(rng.uniform(1.0, 2.0, n) * 2.0 ** rng.integers(0, 100, n))
    b[::3] = -b[::3]
    a0 = f32(np.float64(FLT_MIN) * b.astype(np.float64))
    out["underflow"] = (around(a0), np.tile(b, 5))
    # subnormal quotients that are no ties
    m = 20000
    out["subnormal"] = (f32(rng.uniform(-1, 1, m) * 2.0 ** rng.integers(-149, -100, m)),
                        f32(rng.uniform(0.5, 1, m) * 2.0 ** rng.integers(0, 40, m)))
    # the kernel's own operand ranges (tests/test_host_logic.py): (value - tfLo) / (tfHi - tfLo),
    # (lat - lo) / (hi - lo), direction / length, slab / direction
    out["tf"] = (f32(rng.uniform(-0.1, 1.1, m)) - F(0.0123), np.full(m, F(0.987) - F(0.0123), np.float32))
    out["lat"] = (f32(rng.uniform(-1.6, 1.6, m)) - F(-1.5707964), np.full(m, F(1.5707964) - F(-1.5707964), np.float32))
    d = f32(rng.uniform(-1, 1, (m, 3)))
    out["normalize"] = (d[:, 0].copy(), f32(np.sqrt((d * d).sum(1, dtype=np.float32))))
    out["slab"] = (f32(rng.uniform(-7e6, 7e6, m)) - F(1.4e7), np.where(np.abs(d[:, 1]) < 1e-5, F(1e-5), d[:, 1]).astype(F))
    return {k: (f32(a), f32(b)) for k, (a, b) in out.items()}


# every KAT_STRIDE[name]-th pair of a list goes into tests/golden/kats_raymath.npz (the edge lists
# denser than the random ones; the device tests run every pair against the oracle)
KAT_STRIDE = {"ties": 16, "ties_signed": 4, "near_midpoints": 4, "special": 1, "overflow": 4, "underflow": 4,
              "subnormal": 8, "tf": 16, "lat": 16, "normalize": 16, "slab": 16}


# ---------------------------------------------------------------------------- classification
LUT_SIZES = (1, 2, 3, 5, 300, 1024)
RANGES = {
    "kelvin": (250.3, 310.7), "unit": (0.0, 1.0), "zero98": (0.0, 98.0), "negative": (-40.5, -3.25),
    "reversed": (310.7, 250.3), "empty": (5.0, 5.0), "subnormal": (0.0, 1e-41), "infinite": (-3e38, 3e38),
    "halfinf": (0.0, np.inf),
}
OPACITY_SCALES = (1.0, 0.0, 3.0, 0.25, -1.0)


def lut(size, nonfinite=False):
    """A seeded LUT (size, 4): entries in [-0.25, 1.5], with alphas of exactly 0, below 0 and above 1;
    nonfinite: a NaN and an inf entry too."""
    rng = np.random.default_rng(SEED + 100 + size)
    t = f32(rng.uniform(-0.25, 1.5, (size, 4)))
    t[0, 3] = 0.0
    if size > 1:  # entry 1 is postClassify's second term for idx = 0: zeros there leave a tiny first term alone
        t[0, 3], t[1, 3], t[1, 0] = -0.125, 0.0, 0.0
    if size > 2:
        t[size - 1, 3] = 1.75
    if nonfinite:
        t[size // 2, 3], t[size // 2, 0] = np.nan, np.inf
        t[size - 1, 2] = -np.inf
    return t


def transfer_functions():
    """name -> (lut, lo, hi, opacityScale): every LUT size on the Kelvin range, every range with 300
    and with 5 entries, every opacityScale, the tie range with three more sizes, and the LUT holding a
    NaN and an inf."""
    tfs = {}
    for size in LUT_SIZES:
        tfs[f"size{size}"] = (lut(size), *RANGES["kelvin"], 1.0)
    for name, (lo, hi) in RANGES.items():
        tfs[f"{name}_300"] = (lut(300), lo, hi, 1.0)
        tfs[f"{name}_5"] = (lut(5), lo, hi, 3.0)
    for k, s in enumerate(OPACITY_SCALES):
        tfs[f"scale{k}"] = (lut(300), 0.0, 1.0, s)
    for size in (1, 2, 1024):
        tfs[f"zero98_{size}"] = (lut(size), 0.0, 98.0, 0.25)
    tfs["nonfinite_5"] = (lut(5, True), 0.0, 1.0, 1.0)
    tfs["nonfinite_300"] = (lut(300, True), 250.3, 310.7, -1.0)
    return {k: (t, F(lo), F(hi), F(s)) for k, (t, lo, hi, s) in tfs.items()}


TIES_98 = f32([49.0 * odd * 2.0 ** -149 for odd in range(1, 32, 2)])  # / 98 = odd 2^-150


def classify_values(tf, thin=False):
    """The values to classify under tf = (lut, lo, hi, scale).  thin: the known-answer file's shorter
    list -- fewer interior nodes and random values, every edge case kept."""
    t, lo, hi, _ = tf
    size = len(t)
    lo64, hi64 = np.float64(lo), np.float64(hi)
    with np.errstate(all="ignore"):
        w = hi64 - lo64
        rng = np.random.default_rng(SEED + 7 * size)
        ks = np.arange(size + 1)
        if thin and size > 16:
            ks = np.unique(np.concatenate([ks[:3], ks[-3:], rng.choice(ks, 40, replace=False)]))
        half = np.array([-2.0, -1.5, -1.0, -0.5, 0.5, size - 0.5, size + 0.5, size + 1.0, size + 1.5])
        nodes = lo64 + np.concatenate([ks.astype(np.float64), half]) * w / size
        ws = w if np.isfinite(w) and w != 0 else 1.0
        outside = np.concatenate([lo64 - ws * np.array([0.0137, 0.513, 1.07, 10.3, 1e6]),
                                  hi64 + ws * np.array([0.0137, 0.513, 1.07, 10.3, 1e6])])
        big = F(2.0 ** 31)
        below = np.nextafter(big, F(0))
        edge = f32([below, big, -below, -big]).astype(np.float64)  # v * size at f2i's limit
        limit = lo64 + edge / size * w
        inside = lo64 + rng.uniform(0, 1, 48 if thin else 256) * ws
        special = f32([np.nan, np.inf, -np.inf, 0.0, -0.0, FLT_MAX, -FLT_MAX, 1e-45, -1e-45, 1e-40, -1e-40,
                       np.nextafter(FLT_MIN, F(0)), -np.nextafter(FLT_MIN, F(0)), FLT_MIN])
        v = [around(f32(nodes)), around(f32(outside), 1), around(f32(limit), 4 if thin else 8), f32(inside), special]
        if float(lo) == 0.0 and float(hi) == 98.0:
            v += [TIES_98, -TIES_98]
    return f32(np.concatenate(v))


# ------------------------------------------------------------------------------------- rays
def _unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v)


def ray_scene(window=False):
    """(box6, radiusA, radiusB) of synth_grid(2, 2, 10): the volume's box and the shell's outer and
    inner radius; window: the box of its cells inside a lat/lon window."""
    import irt
    cells = irt.synth_grid(2, 2, 10)
    if window:
        cells = irt.filter_cells(cells, (10, 55), (-30, 60))
    i = irt.volume_info(cells)
    box = f32([i.bounds.lower.x, i.bounds.lower.y, i.bounds.lower.z, i.bounds.upper.x, i.bounds.upper.y, i.bounds.upper.z])
    return box, F(i.sphericalBounds.upper.x), F(i.sphericalBounds.lower.x)


def rays(box, rA, rB):
    """Rays (n, 6) = {org, dir} for box_test and the sphere tests around (box, rA, rB)."""
    rng = np.random.default_rng(SEED + 3)
    lo, hi = box[:3].astype(np.float64), box[3:].astype(np.float64)
    mid = (lo + hi) / 2
    rA64, rB64 = float(rA), float(rB)
    eyes = [(1.4e7, 3e6, 5e6), (0.0, 0.0, 1.4e7),            # outside
            (hi[0], mid[1], mid[2]), (mid[0], lo[1], mid[2]),  # on a box face
            (rA64, 0.0, 0.0), (0.0, -rB64, 0.0),               # on a sphere: C == 0 for that radius
            (0.0, 0.0, 0.0), ((rA64 + rB64) / 2, 0.0, 0.0),    # the centre, inside the shell
            (4096.0, rA64, 0.0), (0.0, 4096.0, rB64)]          # d == 0 with dir = +x / +y (see tangents)
    out = []
    for e in eyes:
        e = np.asarray(e, np.float64)
        to = _unit(mid - e) if np.linalg.norm(mid - e) > 0 else np.array([0.0, 0.0, 1.0])
        d = [to, -to, (1, 0, 0), (0, 1, 0), (0, 0, 1), (-1, 0, 0), (0, -1, 0), (0, 0, -1)]
        d += [_unit(to + 0.6 * rng.normal(size=3)) for _ in range(40)]
        d += [_unit(rng.normal(size=3)) for _ in range(20)]                       # mostly misses
        base = _unit(to + 0.2 * rng.normal(size=3))
        for ax in range(3):
            for c in (1e-5, -1e-5, 2.0 ** -101, -2.0 ** -101, 2.0 ** 101, 0.0, -0.0, np.inf, -np.inf, np.nan,
                      float(np.nextafter(F(1e-5), F(0))), 2.0 ** -100, 2.0 ** 100):
                v = base.copy()
                v[ax] = c
                d.append(v)
        d += [base * s for s in (0.37, 3.0, 1e3, 1e-3, 2.0 ** -60, 2.0 ** 60)]      # A != 1
        out += [np.concatenate([e, np.asarray(v, np.float64)]) for v in d]
    # tangents: dir +x from (x0, y, 0) grazes the sphere of radius y; with x0 = 4096 and y = the radius
    # itself every product is exact and d == 0; y a few ulps either side gives near-tangent rays
    for r in (rA, rB):
        for k in range(-24, 25):
            y = float(ulps(r, k)[0])
            out.append(np.array([4096.0, y, 0.0, 1.0, 0.0, 0.0]))
            out.append(np.array([-3.0e6, y, 0.0, 1.0, 1e-5, 1e-5]))
            out.append(np.array([0.0, y, 0.0, 1.0, 0.0, 0.0]))   # the eye on the tangent point: q == 0
    return f32(np.array(out))


def recip_ok(x):
    with np.errstate(invalid="ignore"):
        a = np.abs(f32(x))
        return (a >= F(2.0 ** -100)) & (a <= F(2.0 ** 100))


def interior_valid(terms7):
    """intersect_spheres_interior's precondition from the oracle's terms (oracle_ray_tests_n): both
    discriminants >= 0, recip_ok for dot(dir, dir) and both q."""
    t = terms7
    with np.errstate(invalid="ignore"):
        return (t[:, 1] >= 0) & (t[:, 4] >= 0) & recip_ok(t[:, 0]) & recip_ok(t[:, 2]) & recip_ok(t[:, 5])


# ---------------------------------------------------------------------------------- gen_ray
GEN_RAY_CAMERAS = (("axis+z", "flat"), ("roll30", "flat"), ("look0.8", "flat"))
GEN_RAY_SIZES = ((16, 16), (67, 33))
GEN_RAY_ACCUM_IDS = (0, 3, 2 ** 31 - 1)


def gen_ray_cases():
    """(name, camera12, W, H, accumID) for the axis-aligned, rolled and off-centre cameras of
    tests/classifier_cameras.py."""
    import classifier_cameras as CC
    out = []
    for name, scene in GEN_RAY_CAMERAS:
        for W, H in GEN_RAY_SIZES:
            lp = CC.launch_params(name, scene, W, H)
            for aid in GEN_RAY_ACCUM_IDS:
                out.append((f"{name}_{W}x{H}_{aid}", lp.camera12(), W, H, aid))
    return out + gen_ray_tie_cases()


def gen_ray_tie_cases():
    """Cameras whose every ray is dir_00 (du = dv = 0) with one component a = 49 odd 2^(k-150) beside
    one of 49 2^k: its square underflows, the length is 49 2^k exactly and normalize's quotient is an
    exact tie between subnormal floats -- whichever neighbour a division shortcut gives, the 1e-5 clamp
    must overwrite it."""
    out = []
    t = 2.0 ** -149
    for j, d00 in enumerate(((147 * t, 98.0, 0.0), (0.0, -196.0, 294 * t), (-98.0, -49 * 7 * t, 0.0),
                             (49 * 11 * 2 * t, 0.0, 196.0), (1568.0, 0.0, -49 * 5 * 16 * t))):
        cam = f32([0.0, 0.0, 1.4e7, *d00, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0])
        out.append((f"tie{j}_8x8_0", cam, 8, 8, 0))
    return out


# ------------------------------------------------------------------------- grid coordinates
def project_cases(dim):
    """(s, lo, hi) for project_axis_inv on a dim-cell axis: lo, hi, NaN, huge values and the floats
    either side of every integer crossing of (s - lo) / (hi - lo) * (dim - 1) (at most 64 of them)."""
    lo, hi = F(6.371229e6), F(6.446229e6)
    ks = np.arange(dim) if dim <= 64 else np.unique(np.linspace(0, dim - 1, 64).astype(int))
    with np.errstate(all="ignore"):
        cross = np.float64(lo) + ks / max(dim - 1, 1) * (np.float64(hi) - np.float64(lo))
    s = np.concatenate([around(f32(cross), 3), around(f32([lo, hi]), 2),
                        f32([np.nan, np.inf, -np.inf, FLT_MAX, -FLT_MAX, 0.0, 1e30, -1e30, 6.3e6, 6.5e6])])
    return f32(s), lo, hi


def project_tie_cases():
    """(s, lo, hi) with lo = 0 and hi = 49 2^k: the pairs of div_ties with that divisor, and their
    negatives -- (s - lo) / (hi - lo) is an exact tie between subnormal floats, and the cell is 0
    whichever neighbour the quotient is."""
    a, b = div_ties()
    out = []
    for hi in (98.0, 196.0, 1568.0, 49.0 * 2.0 ** 20):
        s = a[b == F(hi)]
        assert s.size == 16
        out.append((f32(np.concatenate([s, -s])), F(0.0), F(hi)))
    return out


def sphere_tie_rays():
    """(rays, radiusA, radiusB) that make intersect_spheres' t1 = q / A an exact tie between subnormal
    floats on its reciprocal path: dir = (m 2^43, 0, 0), org = (odd m 2^-108, 0, 0), radii whose
    squares underflow.  Then dot(org, org) = 0, C = 0, B = 2 m^2 odd 2^-65 exactly, d = B^2,
    q = -B, A = m^2 2^86 and q / A = -odd 2^-150 (t2 = C / q = -0); recip_ok holds for A and q."""
    r = []
    for m in range(3, 128, 2):
        for odd in (1, 3, 5, 7, 9, 11, 13, 15):
            for sgn in (1.0, -1.0):
                r.append([sgn * odd * m * 2.0 ** -108, 0.0, 0.0, sgn * m * 2.0 ** 43, 0.0, 0.0])
    return f32(r), F(0.0), F(2.0 ** -80)


def wrap_cases(d):
    return np.concatenate([np.arange(-3 * d, 3 * d + 1), [INT_MIN, 2 ** 31 - 1, INT_MIN + 1, 2 ** 31 - 2]]).astype(np.int32)


# ------------------------------------------------------------------------- oracle answers
def _p(a):
    return a.ctypes.data


def oracle_div(a, b):
    import oracle as O
    a, b = f32(a), f32(b)
    out = np.zeros(a.size, np.float32)
    O.olib().oracle_div_n(_p(a), _p(b), a.size, _p(out))
    return out


def oracle_classify(tf, v):
    """(post_classify (n, 4), quotient, idx, frac) of v under tf, by the oracle."""
    import oracle as O
    t, lo, hi, scale = tf
    t, v = f32(t), f32(v)
    out = np.zeros((v.size, 4), np.float32)
    q, idx, frac = np.zeros(v.size, np.float32), np.zeros(v.size, np.int32), np.zeros(v.size, np.float32)
    O.olib().oracle_post_classify_n(_p(t), len(t), float(lo), float(hi), float(scale), _p(v), v.size, _p(out))
    O.olib().oracle_classify_index_n(len(t), float(lo), float(hi), _p(v), v.size, _p(q), _p(idx), _p(frac))
    return out, q, idx, frac


def oracle_ray_tests(r, box, rA, rB):
    """(flags, out (n, 6), terms (n, 7)) of oracle_ray_tests_n."""
    import oracle as O
    r = f32(r).reshape(-1, 6)
    flags = np.zeros(len(r), np.int32)
    out, terms = np.zeros((len(r), 6), np.float32), np.zeros((len(r), 7), np.float32)
    O.olib().oracle_ray_tests_n(_p(r), len(r), O.b3(box[:3], box[3:]), float(rA), float(rB), _p(flags), _p(out),
                                _p(terms))
    return flags, out, terms


def oracle_gen_ray(camera12, W, H, accum_id):
    import oracle as O
    cam = f32(camera12)
    d, st = np.zeros((H, W, 3), np.float32), np.zeros((H, W), np.uint32)
    O.olib().oracle_generate_ray_n(_p(cam), int(accum_id), W, H, _p(d), _p(st))
    return d, st


def oracle_grid_coord(s, lo, hi, dim, c, d):
    import oracle as O
    s, c = f32(s), np.ascontiguousarray(c, np.int32)
    cell, wrapped = np.zeros(s.size, np.int32), np.zeros(c.size, np.int32)
    O.olib().oracle_grid_coord_n(_p(s), s.size, float(lo), float(hi), dim, _p(cell), _p(c), c.size, d, _p(wrapped))
    return cell, wrapped


def same_bits(a, b):
    """Elementwise: equal as bits, two NaNs counting as equal."""
    a, b = f32(a), f32(b)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))
