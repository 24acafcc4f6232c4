"""irt_render_levels without a GPU: the restatement tests/levels_scenes.py is checked where the
oracle allows it, the inputs of tests/test_gpu_levels.py are counted by the restatement alone (so
that the device comparison cannot pass on empty pictures), and the host side of the call -- the
radii check and the slot order -- is exercised through the binding and, under the address and
undefined-behaviour sanitizers, by a stand-alone program (tests/levels_order_main.cpp)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import irt
import levels_scenes as LS
import sample_scenes as S

F = np.float32


def expected(case):
    return LS.expected(*case)


def slot_radius(case, slot):
    return float(LS.levels_of(case[0], case[2])[slot.index])


# ------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("view_name", list(LS.VIEWS))
def test_rays_are_the_float64_rays_rounded(view_name):
    """The float32 restatement of gen_ray against the same expression in float64 (the idiom of
    tests/test_void_cpu.py::_rays64, with the restatement's own jitters): unit length, the clamp,
    and every component within float32 rounding of the float64 ray."""
    W, H = LS.SIZES["odd"]
    lp = LS.launch_params("flat", view_name, "odd", accum_id=3)
    d = LS.rays(lp, W, H)
    assert d.dtype == F and d.shape == (H, W, 3)
    c = lp.camera12().astype(np.float64)
    # the jitters back out of nothing: recompute them as the restatement draws them
    import oracle as O
    two = np.zeros(2, F)
    ys, xs = np.mgrid[0:H, 0:W]
    jit = np.zeros((H, W, 2))
    for y in range(H):
        for x in range(W):
            O.olib().oracle_lcg((3 * W * H + x) & 0xFFFFFFFF, y, 2, two.ctypes.data)
            jit[y, x] = two
    assert ((jit >= 0) & (jit < 1)).all() and np.unique(jit).size > W * H
    a, b = (xs + 0.5) + jit[..., 1], (ys + 0.5) + jit[..., 0]
    d64 = c[3:6] + a[..., None] * c[6:9] + b[..., None] * c[9:12]
    d64 /= np.linalg.norm(d64, axis=-1, keepdims=True)
    d64 = np.where(np.abs(d64) < 1e-5, 1e-5, d64)
    assert np.abs(d - d64).max() < 4e-7
    assert np.abs(np.linalg.norm(d.astype(np.float64), axis=-1) - 1).max() < 1e-6


def test_a_level_far_outside_the_shell_is_missed_everywhere():
    W, H = LS.SIZES["odd"]
    cells = S.scene("flat")
    top = float(S.shell(cells)[1])
    lp = LS.launch_params("flat", "outside", "odd")
    r = LS.composite(cells, lp, W, H, [top + 5e5], LS.transfunc("flat", "opaque"), True)
    assert r.slots[0].live.sum() > 100 and r.slots[1].live.sum() > 100  # the sphere is in view
    assert not any(s.found.any() for s in r.slots)
    assert (r.colour == 0).all() and (r.level == -1).all() and (r.value == F(LS.MISS)).all()


def test_one_opaque_level_covers_exactly_the_sphere():
    """flat is a whole globe: every hit point of a level inside the shell is in a cell, so with
    alpha 1 everywhere A == 1 exactly where the ray hits the sphere in front of the camera."""
    W, H = LS.SIZES["odd"]
    cells = S.scene("flat")
    lp = LS.launch_params("flat", "outside", "odd")
    radii = LS.levels_of("flat", "midlayer")
    r = LS.composite(cells, lp, W, H, radii, LS.transfunc("flat", "opaque"), False)
    hit, tn, _ = LS.sphere_hits(r.org, r.dirs, radii[0])
    front = hit & (tn > 0)
    assert 100 < front.sum() < W * H
    assert np.array_equal(r.colour[..., 3] == 1, front) and (r.colour[..., 3][~front] == 0).all()
    assert np.array_equal(r.level == 0, front)


def test_lerp_and_pixels_of_an_empty_frame():
    """A ray that finds nothing lerps (0, 0, 0, 0): accumID 3 scales the prior accum by 3/4."""
    prior = LS.prior_accum(5, 3)
    out = LS.lerp(np.zeros((3, 5, 4), F), prior, 3)
    assert np.array_equal(out, (F(0.25) * F(0)) + (F(1) - F(0.25)) * prior)
    fb = LS.pixels(out)
    assert fb.dtype == np.uint32 and ((fb >> 24) == np.minimum(255, (out[..., 3] * F(256)).astype(np.int64))).all()


# ------------------------------------------------------------------ the census
def _first_found(r):
    """(first found slot is a near slot, ... is a far slot) per pixel."""
    seen = np.zeros(r.level.shape, bool)
    near, far = seen.copy(), seen.copy()
    for s in r.slots:
        new = s.found & ~seen
        (far if s.far else near)[new] = True
        seen |= s.found
    return near, far


def test_census_every_case_has_something_to_show():
    for case in LS.CASES:
        r = expected(case)
        assert (r.level >= 0).sum() >= 40, LS.case_id(case)
        assert (r.value[r.level < 0] == F(LS.MISS)).all()
        assert np.unique(r.fb).size > 8, LS.case_id(case)


def test_census_a_pixels_without_a_live_slot():
    for case in LS.CASES:
        r = expected(case)
        none = ~np.any([s.live for s in r.slots], axis=0)
        if case[1] == "outside":
            assert none.sum() >= 20, LS.case_id(case)
            assert (r.accum[none] == LS.lerp(np.zeros(4, F), LS.prior_accum(*LS.SIZES[case[4]])[none]
                                             if case[6] else np.zeros(4, F), case[6])).all()


def test_census_b_first_found_near_and_far():
    near = sum(int(_first_found(expected(c))[0].sum()) for c in LS.CASES)
    far = sum(int(_first_found(expected(c))[1].sum()) for c in LS.CASES)
    assert near >= 500 and far >= 500
    # ... and within one frame (the camera between the levels)
    n, f = _first_found(expected(("flat", "inside", "four", "scale3", "odd", True, 3)))
    assert n.sum() >= 100 and f.sum() >= 100


def test_census_c_several_translucent_levels_show_through():
    for back in (False, True):
        r = expected(("flat", "outside", "four", "translucent", "odd", back, 0))
        n = np.sum([s.contributes for s in r.slots], axis=0)
        assert (n >= 2).sum() >= 300
        assert ((r.colour[..., 3] > 0) & (r.colour[..., 3] < 1)).sum() >= 300


def test_census_d_back_sides_of_spheres_seen_from_outside():
    r = expected(("flat", "outside", "four", "translucent", "odd", True, 0))
    off = expected(("flat", "outside", "four", "translucent", "odd", False, 0))
    n = sum(int((s.far & s.outside & s.contributes).sum()) for s in r.slots)
    assert n >= 300
    assert sum(int((s.far & s.outside & s.live).sum()) for s in off.slots) == 0
    assert not np.array_equal(r.fb, off.fb)


@pytest.mark.parametrize("name", ["filtered", "terrain"])
def test_census_e_live_slots_that_find_nothing(name):
    """... on levels inside the shell: the window's edge on "filtered", the columns' offsets on
    "terrain" (a level outside the shell finds nothing anywhere: not counted)."""
    h0, top, _ = (float(v) for v in S.shell(S.scene(name)))
    n = 0
    for case in LS.CASES:
        if case[0] == name:
            r = expected(case)
            n += sum(int((s.live & ~s.found).sum()) for s in r.slots if h0 < slot_radius(case, s) < top)
    assert n >= 50


def test_census_f_several_levels_in_one_picture():
    best = max(np.unique(expected(c).level[expected(c).level >= 0]).size for c in LS.CASES)
    assert best >= 2
    r = expected(("flat", "inside", "four", "scale3", "odd", True, 3))
    assert np.unique(r.level[r.level >= 0]).size >= 2


def test_census_g_the_clamp_acts():
    n = sum(int(s.clamped.sum()) for c in LS.CASES if c[3] == "scale3" for s in expected(c).slots)
    assert n >= 50
    for c in LS.CASES:  # the translucent alphas stay inside (0, 0.5)
        if c[3] == "translucent":
            assert sum(int(s.clamped.sum()) for s in expected(c).slots) == 0


def test_census_duplicates_resolve_by_index():
    """A duplicated radius: the lower index comes first among the near slots (and, translucent,
    both contribute), the higher first among the far slots."""
    r = expected(("flat", "outside", "dup", "translucent", "odd", True, 3))
    assert [s.index for s in r.slots] == [0, 2, 1, 1, 2, 0]
    assert (r.slots[0].contributes & r.slots[1].contributes).sum() >= 300
    assert set(np.unique(r.level)) == {-1, 0}
    r = expected(("terrain", "under", "dup", "translucent", "packet", False, 0))
    assert set(np.unique(r.level)) <= {-1, 1}  # from inside: far[] = (1, 2, 0)


def test_views_are_where_the_issue_puts_them():
    for name in LS.SCENE_NAMES:
        h0, top, _ = (float(v) for v in S.shell(S.scene(name)))
        four = np.sort(LS.levels_of(name, "four").astype(np.float64))
        dist = lambda v: float(np.linalg.norm(np.array(LS.view(name, v)[0], np.float64)))  # noqa: E731
        assert four[0] < h0 < four[1] < dist("inside") < four[2] < top < four[3] < dist("outside")
        assert dist("under") < min(float(LS.levels_of(name, w).min()) for w in ("inner", "four", "dup", "sixteen"))
        assert h0 < float(LS.levels_of(name, "inner")[0]) < top and h0 < float(LS.levels_of(name, "midlayer")[0]) < top
        assert LS.levels_of(name, "sixteen").size == irt.MAX_LEVELS


# ------------------------------------------------------------------ the host side
def test_python_side_radius_validation():
    for bad in ([], [6.4e6] * 17, [6.4e6, 0.0], [-1.0], [np.nan], [np.inf, 6.4e6]):
        with pytest.raises(irt.IrtError) as e:
            irt.levels_radii(bad)
        assert e.value.code == irt.E_INVALID
    r = irt.levels_radii([6.4e6, 6.38e6])
    assert r.dtype == np.float32 and r.flags.c_contiguous and r.size == 2
    assert irt.MAX_LEVELS == 16 and irt.LEVELS_BACK == 1


def test_levels_order_is_the_restatements_slot_order():
    rng = np.random.default_rng(3)
    sets = [LS.levels_of(n, w) for n in LS.SCENE_NAMES for w in ("inner", "four", "dup", "sixteen")]
    sets += [rng.choice([6.37e6, 6.38e6, 6.39e6], k).astype(F) for k in range(1, 17)]
    for radii in sets:
        out, idx = irt.levels_order(radii)
        near, far = LS.slot_order(radii)
        assert list(idx) == near and far == near[::-1]
        assert np.array_equal(out, np.asarray(radii, F)[near])
    for bad in ([], [6.4e6] * 17, [0.0], [np.nan, 1.0]):
        with pytest.raises(irt.IrtError) as e:
            irt.levels_order(bad)
        assert e.value.code == irt.E_INVALID


def test_level_order_under_the_sanitizers(tmp_path):
    """host/irt_level_order.cpp and tests/levels_order_main.cpp as one program of their own, built
    with -fsanitize=address,undefined and run here (no code loaded into python is involved)."""
    cxx = shutil.which(os.environ.get("CXX", "g++"))
    assert cxx, "no C++ compiler"
    repo = os.path.dirname(os.path.abspath(irt.PKG_DIR))
    exe = str(tmp_path / "levels_order_main")
    # (the sanitizers' runtimes linked into the program: nothing depends on the order of the
    # process's shared libraries)
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-static-libasan", "-static-libubsan",
           "-ffp-contract=off", "-I" + os.path.join(repo, "include"), "-I" + os.path.join(irt.PKG_DIR, "csrc"),
           os.path.join(irt.PKG_DIR, "host", "irt_level_order.cpp"),
           os.path.join(os.path.dirname(os.path.abspath(__file__)), "levels_order_main.cpp"), "-o", exe]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "levels_order_main: ok" in run.stdout
