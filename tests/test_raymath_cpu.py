"""The cases of tests/raymath_cases.py on the CPU: the oracle's answers equal the reference build's
(tests/golden/kats_raymath.npz, bit for bit, two NaNs counting as equal), and a census that keeps
tests/test_gpu_raymath.py from passing on empty edges."""
import os

import numpy as np

import raymath_cases as RC

KATS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kats_raymath.npz")


def _same(a, b):
    return bool(RC.same_bits(np.asarray(a).ravel(), np.asarray(b).ravel()).all())


def test_oracle_divisions_equal_the_reference_kats():
    z = np.load(KATS)
    for name, (a, b) in RC.div_pairs().items():
        a, b = a[::RC.KAT_STRIDE[name]], b[::RC.KAT_STRIDE[name]]
        assert np.array_equal(RC.f32(a).view(np.uint32), z[f"div_a_{name}"].view(np.uint32)), name
        assert np.array_equal(RC.f32(b).view(np.uint32), z[f"div_b_{name}"].view(np.uint32)), name
        assert _same(RC.oracle_div(a, b), z[f"div_q_{name}"]), name


def test_oracle_post_classify_equals_the_reference_kats():
    z = np.load(KATS)
    for name, tf in RC.transfer_functions().items():
        v = RC.classify_values(tf, thin=True)
        assert _same(v, z[f"tf_v_{name}"]) and _same(tf[0], z[f"tf_lut_{len(tf[0])}_{int(np.isnan(tf[0]).any())}"]), name
        assert _same(np.float32([tf[1], tf[2], tf[3]]), z[f"tf_range_{name}"]), name
        assert _same(RC.oracle_classify(tf, v)[0], z[f"tf_out_{name}"]), name
        # the thinned list is a part of the full one
        assert np.isin(v.view(np.uint32), RC.classify_values(tf).view(np.uint32)).all(), name


def test_oracle_ray_tests_equal_the_reference_kats():
    z = np.load(KATS)
    for w in (False, True):
        box, rA, rB = RC.ray_scene(w)
        r = RC.rays(box, rA, rB)
        assert _same(np.float32(list(box) + [rA, rB]), z[f"ray_scene_{int(w)}"]) and _same(r, z[f"ray_rays_{int(w)}"])
        flags, out, _ = RC.oracle_ray_tests(r, box, rA, rB)
        assert np.array_equal(flags, z[f"ray_flags_{int(w)}"].astype(np.int32))
        assert _same(out, z[f"ray_out_{int(w)}"])


def test_oracle_generate_ray_equals_the_reference_kats():
    z = np.load(KATS)
    for name, cam, W, H, aid in RC.gen_ray_cases():
        assert _same(cam, z[f"gen_cam_{name}"]), name
        d, st = RC.oracle_gen_ray(cam, W, H, aid)
        step = 1 if W * H <= 256 else 7
        assert _same(d.reshape(-1, 3)[::step], z[f"gen_dir_{name}"]), name
        assert np.array_equal(st.ravel()[::step], z[f"gen_state_{name}"]), name


def test_division_cases_hold_ties_the_double_product_gets_wrong():
    """Of the 131,072 exact subnormal ties of raymath_cases.div_ties, (float)((double)a * (1.0 /
    (double)b)) differs from a / b on 7,768 (153 more among the 8,192 negated ones); outside the
    subnormal results the product equals the division on every other list, and redoing the products
    that come out subnormal by the division (irt_device.h div_unsettled) leaves no difference at all."""
    P = RC.div_pairs()
    count = {}
    for name, (a, b) in P.items():
        ref, un = RC.oracle_div(a, b), RC.unfixed_product(a, b)
        bad = ~RC.same_bits(ref, un)
        count[name] = int(bad.sum())
        assert (np.abs(ref[bad]) <= RC.FLT_MIN).all(), name
        fixed = np.where((np.abs(un) < RC.FLT_MIN) & (un != 0), ref, un)
        assert RC.same_bits(fixed, ref).all(), name
    assert count["ties"] == 7768 and count["ties_signed"] == 153, count
    assert all(n == 0 for k, n in count.items() if k not in ("ties", "ties_signed", "special")), count
    a, b = P["near_midpoints"]
    assert a.size > 10000


def test_classification_cases_reach_every_edge():
    """Judged by the oracle, the classification cases hold idx == INT_MIN, a negative idx with a
    negative frac, idx == -1, idx == size - 1, idx >= size, a NaN result and a quotient that is an exact
    tie between two subnormal floats -- and on the tie range the unfixed quotient changes an output."""
    n = dict(intmin=0, negfrac=0, minus1=0, last=0, over=0, nan=0, tie=0, tie_visible=0)
    sizes = set()
    for name, tf in RC.transfer_functions().items():
        t, lo, hi, scale = tf
        size = len(t)
        sizes.add(size)
        v = RC.classify_values(tf)
        out, q, idx, frac = RC.oracle_classify(tf, v)
        n["intmin"] += int((idx == RC.INT_MIN).sum())
        n["negfrac"] += int(((idx < 0) & (idx > RC.INT_MIN) & (frac < 0)).sum())
        n["minus1"] += int((idx == -1).sum())
        n["last"] += int((idx == size - 1).sum())
        n["over"] += int((idx >= size).sum())
        n["nan"] += int(np.isnan(out).any(1).sum())
        with np.errstate(all="ignore"):
            exact = (v.astype(np.float64) - np.float64(lo)) / (np.float64(hi) - np.float64(lo)) * 2.0 ** 150
            tie = np.isfinite(exact) & (exact == np.rint(exact)) & (np.abs(exact) < 2.0 ** 24) & (np.rint(exact) % 2 == 1)
            n["tie"] += int(tie.sum())
            # the outputs with the unfixed quotient in place of the division
            un = RC.unfixed_product(v - lo, np.full(v.size, hi - lo, np.float32))
            wrong = tie & ~RC.same_bits(un, q)
            if wrong.any() and size > 1:
                s = np.float32(size)
                i1 = np.clip((un[wrong] * s).astype(np.int64), 0, size - 1)
                fr = un[wrong] * s - i1.astype(np.float32)
                got_w = t[i1, 3] * fr + t[np.clip(i1 + 1, 0, size - 1), 3] * (np.float32(1) - fr) * scale
                n["tie_visible"] += int((~RC.same_bits(got_w, out[wrong, 3])).sum())
    assert sizes == set(RC.LUT_SIZES)
    assert all(c > 0 for c in n.values()), n


def test_ray_cases_reach_every_edge():
    """The ray cases hold the fallback division on every axis, d < 0, d == 0, C == 0 and q == 0 for each
    radius, box misses and hits, and rays valid for the interior form."""
    for w in (False, True):
        box, rA, rB = RC.ray_scene(w)
        r = RC.rays(box, rA, rB)
        flags, out, terms = RC.oracle_ray_tests(r, box, rA, rB)
        for ax in range(3):
            assert (~RC.recip_ok(r[:, 3 + ax])).sum() > 0
        for k in (0, 1):
            d, q, c = terms[:, 1 + 3 * k], terms[:, 2 + 3 * k], terms[:, 3 + 3 * k]
            assert (d < 0).sum() > 0 and (d == 0).sum() > 0 and (c == 0).sum() > 0 and (q == 0).sum() > 0
            assert (d > 0).sum() > 0
        assert ((flags & 1) == 0).sum() > 0 and (flags & 1).sum() > 0
        assert RC.interior_valid(terms).sum() > 100
        assert (terms[:, 0] != 1).sum() > 0 and (np.abs(r[:, 3:]) == np.float32(1e-5)).sum() > 0


def test_tie_cases_reach_the_sites_that_keep_or_guard_the_product():
    """The tie inputs of gen_ray, project_axis_inv and intersect_spheres are ties on which the bare
    double product differs from the division: gen_ray's cameras (3 components, each clamped to 1e-5 by
    the oracle), project_axis_inv's values (12 of 32 per divisor, every cell 0) and intersect_spheres'
    rays (t1 = q / A subnormal on 882 of 1,008 rays, the product differing on 76; recip_ok holds for A
    and q, so the device takes its reciprocal path)."""
    n = 0
    for name, cam, W, H, aid in RC.gen_ray_tie_cases():
        d00 = cam[3:6]
        ln = np.sqrt(np.float32(np.float32(d00[0] * d00[0] + d00[1] * d00[1]) + d00[2] * d00[2]))
        with np.errstate(all="ignore"):
            q = d00 / ln
        n += int((~RC.same_bits(q, RC.unfixed_product(d00, np.full(3, ln, np.float32)))).sum())
        d, _ = RC.oracle_gen_ray(cam, W, H, aid)
        small = (np.abs(q) < RC.FLT_MIN)
        assert small.sum() == 2 and (d[..., small] == np.float32(1e-5)).all(), name
    assert n == 3
    for s, lo, hi in RC.project_tie_cases():
        b = np.full(s.size, hi - lo, np.float32)
        assert int((~RC.same_bits(RC.oracle_div(s - lo, b), RC.unfixed_product(s - lo, b))).sum()) == 12
        for dim in (2, 1024):
            assert not RC.oracle_grid_coord(s, lo, hi, dim, np.zeros(1, np.int32), 1)[0].any()
    r, rA, rB = RC.sphere_tie_rays()
    flags, out, t = RC.oracle_ray_tests(r, RC.f32([-1, -1, -1, 1, 1, 1]), rA, rB)
    assert (flags & 6 == 6).all() and RC.recip_ok(t[:, 0]).all() and RC.recip_ok(t[:, 2]).all()
    with np.errstate(all="ignore"):
        t1 = t[:, 2] / t[:, 0]
    assert int(((np.abs(t1) < RC.FLT_MIN) & (t1 != 0)).sum()) == 882
    assert int((~RC.same_bits(t1, RC.unfixed_product(t[:, 2], t[:, 0]))).sum()) == 76
    assert _same(np.minimum(t1, np.float32(-0.0)), out[:, 2])
