"""The raygen's per-value arithmetic on the device, value by value against the oracle: the two
division shortcuts, classification, the ray tests, gen_ray and the shell grid's coordinates, through
the irt_debug_* hooks of csrc/irt_debug_raymath.hip (which call the kernels' own inline functions) on
the cases of tests/raymath_cases.py.  Every comparison is bit for bit, two NaNs counting as equal."""
import numpy as np
import pytest

import irt
import raymath_cases as RC

pytestmark = pytest.mark.gpu

CHUNK = 1 << 18  # values per hook call


def _differ(got, ref):
    return ~RC.same_bits(np.asarray(got).ravel(), np.asarray(ref).ravel())


def _report(name, bad, *cols):
    n = int(bad.sum())
    if n:
        k = np.flatnonzero(bad)[:4]
        print(f"{name}: {n} of {bad.size} differ, first", [[np.asarray(c).ravel()[i] for c in cols] for i in k])
    return n


@pytest.fixture(scope="module")
def ctx():
    with irt.Context(irt.synth_grid(2, 2, 10), device=0) as c:
        yield c


def test_divisions_equal_the_f32_division():
    """div_uniform (with the inverse a launch computes) and div_recip (or the fallback division where
    recip_ok fails) equal a / b on every pair of raymath_cases.div_pairs: the exact subnormal ties,
    quotients 2^-48 from a normal-range midpoint, divisors at recip_ok's limits, zeros, infinities,
    NaN, the overflow and the subnormal boundary, the kernel's own operand ranges."""
    failed = {}
    for name, (a, b) in RC.div_pairs().items():
        ref = RC.oracle_div(a, b)
        for at in range(0, a.size, CHUNK):
            s = slice(at, at + CHUNK)
            u, r = irt.debug_device_div(a[s], b[s])
            nu = _report(f"div_uniform {name}", _differ(u, ref[s]), a[s], b[s], u, ref[s])
            nr = _report(f"div_recip {name}", _differ(r, ref[s]), a[s], b[s], r, ref[s])
            if nu or nr:
                failed[name] = (failed.get(name, (0, 0))[0] + nu, failed.get(name, (0, 0))[1] + nr)
    assert not failed, f"(div_uniform, div_recip) mismatches per case list: {failed}"


@pytest.mark.parametrize("name", sorted(RC.transfer_functions()))
def test_classification_equals_the_oracle(ctx, name):
    """post_classify equals the oracle's postClassify on every value of raymath_cases.classify_values
    under the transfer function, and classify_alpha equals post_classify's alpha as bits."""
    tf = RC.transfer_functions()[name]
    t, lo, hi, scale = tf
    ctx.set_transfunc(t, (lo, hi), scale)
    v = RC.classify_values(tf)
    ref = RC.oracle_classify(tf, v)[0]
    got, alpha = ctx.debug_classify(v)
    bad = _differ(got, ref).reshape(-1, 4).any(1)
    n = _report(f"post_classify {name}", bad, v, got[:, 3], ref[:, 3])
    na = _report(f"classify_alpha {name}", _differ(alpha, got[:, 3]), v, alpha, got[:, 3])
    assert n == 0 and na == 0, (name, n, na)


@pytest.mark.parametrize("window", [False, True])
def test_ray_tests_equal_the_oracle(window):
    """box_test and intersect_sphere equal the oracle's boxTest and intersectSphere; intersect_spheres
    equals two intersect_sphere calls, and so does intersect_spheres_interior on the rays the oracle's
    terms admit (both discriminants >= 0, recip_ok for A and both q)."""
    box, rA, rB = RC.ray_scene(window)
    r = RC.rays(box, rA, rB)
    flags, out, terms = RC.oracle_ray_tests(r, box, rA, rB)
    ok = RC.interior_valid(terms)
    assert ok.sum() > 100
    gf, g = irt.debug_ray_tests(r, ok, box, rA, rB)
    assert np.array_equal(gf & 7, flags), np.flatnonzero((gf & 7) != flags)[:8]
    assert _report("box_test / intersect_sphere", _differ(g[:, :6], out).reshape(-1, 6).any(1), r[:, 0], r[:, 3]) == 0
    # the two-sphere forms against the single calls, on the device's own outputs
    assert np.array_equal((gf >> 3) & 3, (gf >> 1) & 3)
    assert _report("intersect_spheres", _differ(g[:, 6:10], g[:, 2:6]).reshape(-1, 4).any(1), r[:, 0], r[:, 3]) == 0
    assert np.array_equal((gf & 32) != 0, ok)
    assert _report("intersect_spheres_interior", _differ(g[ok, 10:14], g[ok, 2:6]).reshape(-1, 4).any(1)) == 0
    assert not g[~ok, 10:14].any()


def test_gen_ray_equals_the_oracle():
    """gen_ray's direction and LCG state per pixel equal the oracle's generateRay for the axis-aligned,
    rolled and off-centre cameras, at 16 x 16 and 67 x 33, accumIDs 0, 3 and 2^31 - 1 -- and for the
    cameras of raymath_cases.gen_ray_tie_cases, whose normalised components are exact ties between
    subnormal floats before the 1e-5 clamp (gen_ray keeps the bare product there)."""
    for name, cam, W, H, aid in RC.gen_ray_cases():
        lp = irt.LaunchParams()
        lp.org, lp.dir_00, lp.dir_du, lp.dir_dv = (irt.vec3(cam[3 * k:3 * k + 3]) for k in range(4))
        lp.accumID = aid
        d, st = irt.debug_gen_ray(lp, W, H)
        rd, rst = RC.oracle_gen_ray(cam, W, H, aid)
        assert np.array_equal(st, rst), name
        assert _report(f"gen_ray {name}", _differ(d, rd)) == 0, name


@pytest.mark.parametrize("dim,d", [(2, 1), (1024, 1024), (2, 1024), (1024, 1)])
def test_grid_coordinates_equal_the_oracle(dim, d):
    """project_axis_inv equals projectToSphericalGrid's axis (lo, hi, NaN, huge values, the floats
    either side of every integer crossing) and wrap_coord normalizeGridCoord over [-3d, 3d], INT_MIN
    and INT_MAX."""
    s, lo, hi = RC.project_cases(dim)
    c = RC.wrap_cases(d)
    cell, wrapped = irt.debug_grid_coord(s, lo, hi, dim, c, d)
    rcell, rwrapped = RC.oracle_grid_coord(s, lo, hi, dim, c, d)
    assert np.array_equal(cell, rcell), (s[cell != rcell][:4], cell[cell != rcell][:4], rcell[cell != rcell][:4])
    assert np.array_equal(wrapped, rwrapped), c[wrapped != rwrapped][:4]


def test_box_test_redoes_subnormal_slab_quotients():
    """box_test with a box face at 147 2^-149 times odd numbers, the eye at the origin and direction
    components of 98 and its doubles: slab quotients that are exact ties between subnormal floats, where
    the products alone differ from the division (all six quotients are then redone by it)."""
    t = np.float32(np.ldexp(147.0, -149))
    box = RC.f32([t, 3 * t, 5 * t, 1.0, 2.0, 3.0])
    dirs = [(98.0, 196.0, 392.0), (196.0, 98.0, 98.0), (-98.0, 98.0, 3136.0), (98.0, -196.0, 98.0), (1.0, 1.0, 98.0)]
    r = RC.f32([[0.0, 0.0, 0.0, *d] for d in dirs])
    flags, out, terms = RC.oracle_ray_tests(r, box, 1.0, 0.5)
    un = RC.unfixed_product(np.tile(box[:3], (len(r), 1)).ravel(), r[:, 3:].ravel())
    with np.errstate(all="ignore"):
        assert (~RC.same_bits(un, np.tile(box[:3], (len(r), 1)).ravel() / r[:, 3:].ravel())).sum() > 0
    gf, g = irt.debug_ray_tests(r, np.zeros(len(r), np.uint8), box, 1.0, 0.5)
    assert np.array_equal(gf & 7, flags)
    assert _report("box_test on subnormal ties", _differ(g[:, :6], out).reshape(-1, 6).any(1), r[:, 3], g[:, 0], out[:, 0]) == 0


def test_intersect_spheres_redoes_subnormal_quotients():
    """intersect_spheres on raymath_cases.sphere_tie_rays: t1 = q / A is an exact tie between subnormal
    floats on the reciprocal path (recip_ok holds for A and q), where the product alone differs from the
    division on some rays; both spheres must still equal intersect_sphere and the oracle."""
    r, rA, rB = RC.sphere_tie_rays()
    box = RC.f32([-1, -1, -1, 1, 1, 1])
    flags, out, terms = RC.oracle_ray_tests(r, box, rA, rB)
    assert RC.recip_ok(terms[:, 0]).all() and RC.recip_ok(terms[:, 2]).all() and RC.recip_ok(terms[:, 5]).all()
    gf, g = irt.debug_ray_tests(r, np.zeros(len(r), np.uint8), box, rA, rB)
    assert np.array_equal(gf & 6, flags & 6) and np.array_equal((gf >> 3) & 3, (gf >> 1) & 3)
    assert _report("intersect_sphere on ties", _differ(g[:, 2:6], out[:, 2:6]).reshape(-1, 4).any(1), r[:, 0], g[:, 2], out[:, 2]) == 0
    assert _report("intersect_spheres on ties", _differ(g[:, 6:10], g[:, 2:6]).reshape(-1, 4).any(1), r[:, 0], g[:, 6], g[:, 2]) == 0


@pytest.mark.parametrize("dim", [2, 1024])
def test_project_axis_on_subnormal_ties(dim):
    """project_axis_inv keeps the bare product: on quotients that are exact ties between subnormal
    floats (raymath_cases.project_tie_cases) its cell still equals the oracle's, 0."""
    for s, lo, hi in RC.project_tie_cases():
        c = np.zeros(1, np.int32)
        cell, _ = irt.debug_grid_coord(s, lo, hi, dim, c, 1)
        rcell, _ = RC.oracle_grid_coord(s, lo, hi, dim, c, 1)
        assert np.array_equal(cell, rcell) and not rcell.any(), (float(hi), cell, rcell)
