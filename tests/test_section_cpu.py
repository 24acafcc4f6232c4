"""The sections without a GPU: irt_section_points against the oracle's toCartesian and against
irt_latlon_points, irt_great_circle against a float64 NumPy restatement, the census of
tests/test_gpu_section.py's inputs by the oracle alone (so that the device comparison cannot pass
on columns that exercise nothing), the refusals, and the two helpers under the address and
undefined-behaviour sanitizers in a stand-alone program (tests/section_main.cpp)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import irt
import sample_scenes as S
import section_scenes as SS

F = np.float32


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


# ------------------------------------------------------------------ irt_section_points
@pytest.mark.parametrize("key", SS.SETS)
def test_section_points_are_the_oracles_to_cartesian(key):
    lat, lon = SS.columns(key)
    rad = SS.levels("terrain")[:4]
    pts = irt.section_points(lat, lon, rad)
    assert pts.shape == (rad.size, lat.size, 3) and pts.dtype == F
    for k in range(rad.size):
        for c in range(lat.size):
            want = S.oracle_to_cartesian(rad[k], lat[c], lon[c])
            assert np.array_equal(bits(pts[k, c]), bits(want)), (key, k, c, pts[k, c], want)


@pytest.mark.parametrize("name", SS.SCENE_NAMES)
def test_section_points_of_a_grids_pairs_are_latlon_points(name):
    lat, lon, rad, plat, plon = SS.grid_pairs(name)
    grid = irt.latlon_points(lat, lon, rad)
    pairs = irt.section_points(plat, plon, rad)
    assert pairs.shape == (rad.size, lat.size * lon.size, 3)
    assert np.array_equal(bits(pairs), bits(grid.reshape(pairs.shape)))


def test_section_points_layout_and_empty_sections():
    lat, lon = SS.columns("stations")
    rad = np.array([6.4e6, 6.41e6, 6.39e6], F)
    flat = np.full(3 * rad.size * lat.size + 2, 7.0, F)  # the C layout: xyz[3 * (k * n + c)]
    L = irt.lib()
    assert L.irt_section_points(lat.ctypes.data, lon.ctypes.data, lat.size, rad.ctypes.data, rad.size,
                                flat[1:].ctypes.data) == 0
    assert flat[0] == 7.0 and flat[-1] == 7.0
    assert np.array_equal(bits(flat[1:-1]), bits(irt.section_points(lat, lon, rad)).reshape(-1))
    assert irt.section_points([], [], rad).shape == (3, 0, 3) and irt.section_points(lat, lon, []).shape == (0, 41, 3)
    with pytest.raises(irt.IrtError, match="pairs"):
        irt.section_points(lat, lon[:5], rad)


# ------------------------------------------------------------------ irt_great_circle
CIRCLES = list(SS.TRACKS.values()) + [
    (0.0, 3.0, 0.0, -3.0, 2), (-1.2, 2.0, 1.1, -0.9, 257), (0.5, 0.25, 0.5, 0.25, 9),
    (0.0, 0.0, 0.0, float(SS.PI), 33),       # half a turn along the equator, 8.7e-8 rad short of antipodal
    (float(SS.HALF_PI), -2.0, 0.2, 1.0, 17)]  # from a pole


@pytest.mark.parametrize("case", CIRCLES, ids=lambda c: "_".join(f"{v:g}" for v in c))
def test_great_circle_is_the_numpy_restatement(case):
    """Every point's unit vector within 3e-7 of the float64 restatement's: the float rounding of
    lat and lon is at most half an ulp of pi each (1.2e-7 rad), the rest is double noise.  Positions,
    not angles, so the pole and the date line need no special case.  End points exact, arc to 1e-12."""
    lat0, lon0, lat1, lon1, n = case
    lat, lon, arc = irt.great_circle(*case)
    want, w = SS.great_circle_numpy(*case)
    assert lat.dtype == F and lon.dtype == F and lat.shape == (n,) and lon.shape == (n,)
    assert np.isfinite(lat).all() and np.isfinite(lon).all()
    assert (np.abs(lat) <= SS.HALF_PI).all()
    err = np.linalg.norm(SS.unit_vectors(lat, lon) - want, axis=1)
    print(f"{case}: arc {arc:.9f}, largest distance from the restatement {err.max():.3g}")
    assert err.max() <= 3e-7
    assert abs(arc - w) <= 1e-12
    assert bits(lat[0]) == bits(F(lat0)) and bits(lon[0]) == bits(F(lon0))
    if n > 1:
        assert bits(lat[-1]) == bits(F(lat1)) and bits(lon[-1]) == bits(F(lon1))


def test_great_circle_tracks_go_where_the_scenes_say():
    lat, lon = SS.columns("equator")
    assert (np.abs(lat) < 1e-7).all() and (lon[:65] > 3.0 - 1e-6).all() and (lon[65:] < -3.0 + 1e-6).all()
    lat, lon = SS.columns("pole")
    assert lat.max() > 1.5 and lat.size == 65
    lat, lon = SS.columns("meridian")
    assert bits(lat[0]) == bits(SS.HALF_PI) and bits(lat[-1]) == bits(-SS.HALF_PI) and lat.size == 64
    assert (np.diff(lat) < 0).all()
    lat, lon = SS.columns("oblique")
    assert lat.size == 63 and SS.columns("point")[0].size == 1
    # coincident end points: every point is the start
    lat, lon, arc = irt.great_circle(0.5, 0.25, 0.5, 0.25, 9)
    assert (lat == F(0.5)).all() and (lon == F(0.25)).all() and arc == 0.0
    assert sorted(c[0].size for c in map(SS.columns, SS.SETS)) == [1, 41, 63, 64, 65, 130]


def test_great_circle_refusals():
    L = irt.lib()
    lat, lon = np.full(4, 7.0, F), np.full(4, 7.0, F)
    arc = C.c_double(-5.0)

    def call(a=0.1, b=0.2, c=0.3, d=0.4, n=4, la=lat, lo=lon, arc=arc):
        p = lambda x: x.ctypes.data if x is not None else None  # noqa: E731
        return L.irt_great_circle(a, b, c, d, n, p(la), p(lo), C.byref(arc) if arc is not None else None)

    def refused(rc, word):
        assert rc == irt.E_INVALID and word in L.irt_last_error().decode(), L.irt_last_error()

    refused(call(n=0), "points")
    refused(call(n=-3), "points")
    for bad in (np.nan, np.inf, -np.inf):
        for k in "abcd":
            refused(call(**{k: bad}), "not finite")
    refused(call(la=None), "null lat or lon")
    refused(call(lo=None), "null lat or lon")
    # antipodal: the two poles as floats, half a turn apart in lon (sin w ~ 4e-15, a . b < 0)
    refused(call(float(SS.HALF_PI), 0.0, -float(SS.HALF_PI), float(SS.PI)), "antipodal")
    assert (lat == 7.0).all() and (lon == 7.0).all() and arc.value == -5.0  # nothing written
    assert call(arc=None) == 0 and arc.value == -5.0 and (lat != 7.0).all()
    with pytest.raises(irt.IrtError, match="points"):
        irt.great_circle(0, 0, 1, 1, 0)


# ------------------------------------------------------------------ the census
@pytest.mark.parametrize("name", SS.SCENE_NAMES)
def test_census_of_values_and_columns(name):
    """Per scene, over the sets test_gpu_section.py walks: found and missed points, a level with no
    found point (the level the kernel's locator is skipped at), extremes at different levels; on
    filtered, columns that find nothing and columns that find some of the levels."""
    found = missed = empty_levels = kdiff = 0
    for key in SS.SETS:
        f, v = SS.answers(name, key)
        lat, _ = SS.columns(key)
        rad = SS.levels(name)
        assert f.shape == v.shape == (rad.size, lat.size) and f.dtype == np.uint8
        found += int(f.sum())
        missed += int((f == 0).sum())
        empty_levels += int((f.sum(1) == 0).sum())
        r = SS.reduced(name, key, "none")
        assert np.array_equal(r["count"], f.sum(0))
        kdiff += int((r["kmax"] != r["kmin"]).sum())
        p = SS.CS._parts(name)
        assert not f[(rad == p.below) | (rad == p.above)].any()  # outside the shell: found nowhere
    print(f"{name}: {found} found, {missed} missed, {empty_levels} levels without a found point, "
          f"{kdiff} columns with kmax != kmin")
    assert found >= 2000 and missed >= 500 and empty_levels >= 12 and kdiff >= 50
    if name == "filtered":
        c = SS.reduced(name, "stations", "none")["count"]
        assert (c == 0).sum() >= 10 and ((c > 0) & (c < SS.levels(name).size)).sum() >= 10
        assert not SS.answers(name, "equator")[0].any()  # a whole track outside the window
    asc, shuf = SS.answers(name, "stations", "ascending"), SS.answers(name, "stations")
    perm = SS.CS.shuffle_of(name)
    assert np.array_equal(shuf[0], asc[0][perm]) and np.array_equal(bits(shuf[1]), bits(asc[1][perm]))


def test_census_the_stations():
    lat, lon = SS.columns("stations")
    pairs = list(zip(bits(lat).tolist(), bits(lon).tolist()))
    assert max(pairs.count(p) for p in pairs) == 3
    assert (lon == -SS.PI).any() and (lon == SS.BELOW_PI).any() and (lat == 0).sum() >= 2
    assert (np.diff(lat) < 0).any() and (np.diff(lat) > 0).any() and (np.diff(lon) < 0).any()
    inside = (np.degrees(lat) > -30) & (np.degrees(lat) < 60) & (np.degrees(lon) > -90) & (np.degrees(lon) < 45)
    assert inside.sum() >= 6 and (~inside).sum() >= 10


@pytest.mark.parametrize("case", SS.CURTAINS, ids="-".join)
def test_census_every_curtain_has_something_to_show(case):
    px = SS.curtain(*case)
    f, _ = SS.answers(case[0], case[1])
    print(f"{case}: {np.unique(px[px != 0]).size} distinct non-zero pixels, {int((px == 0).sum())} zero")
    assert np.unique(px[px != 0]).size >= 2 and (px == 0).any() and (px[f == 0] == 0).all()
    assert ((px >> 24)[f != 0] > 0).any()  # a found point shows: alpha above 0
    other = SS.curtain_of(SS.LS.transfunc(case[0], case[2]), f, SS.answers(case[0], case[1])[1], ((1, 1, 1), 1.0))
    assert not np.array_equal(other, px)  # the ambient terms are in the picture


def test_census_both_transfer_functions_are_used_and_differ():
    assert {c[2] for c in SS.CURTAINS} == set(SS.TRANSFUNCS)
    assert not np.array_equal(SS.curtain("flat", "oblique", "default"), SS.curtain("flat", "oblique", "translucent"))


@pytest.mark.parametrize("mode", [irt.MODE_CUBQL, irt.MODE_TRIANGLES])
def test_census_of_the_unstructured_samplers(mode):
    for key in ("oblique", "stations"):
        f, v = SS.answers("flat", key, "shuffled", mode)
        r = SS.reduced("flat", key, "mixed", "shuffled", mode)
        assert f.sum() >= 500 and (f == 0).sum() >= 50 and (r["kmax"] != r["kmin"]).sum() >= 20


def test_the_grids_pairs_are_a_grid():
    lat, lon, rad, plat, plon = SS.grid_pairs("flat")
    assert plat.size == plon.size == lat.size * lon.size == 63 and rad.size == 5
    assert plat[lon.size] == lat[1] and plon[lon.size + 2] == lon[2]


# ------------------------------------------------------------------ the host side of irt_section
def test_section_of_a_null_context_is_refused_without_a_device():
    L = irt.lib()
    lat, lon = SS.columns("oblique")
    rad = np.array([6.4e6], F)
    rc = L.irt_section(None, 0, lat.ctypes.data, lon.ctypes.data, lat.size, rad.ctypes.data, None, 1,
                       irt.vec3((1, 1, 1)), 1.0, irt.SectionOut(), 0.0, None)
    assert rc == irt.E_INVALID and "null context" in L.irt_last_error().decode()
    assert C.sizeof(irt.SectionOut) == 9 * C.sizeof(C.c_void_p)
    assert set(irt.SECTION_OUTPUTS) == {"value", "found", "rgba"}


def test_section_helpers_under_the_sanitizers(tmp_path):
    """host/irt_section.cpp and tests/section_main.cpp as one program of their own, built with
    -fsanitize=address,undefined and run here (no code loaded into python is involved)."""
    cxx = shutil.which(os.environ.get("CXX", "g++"))
    assert cxx, "no C++ compiler"
    repo = os.path.dirname(os.path.abspath(irt.PKG_DIR))
    exe = str(tmp_path / "section_main")
    # (the sanitizers' runtimes linked into the program: nothing depends on the order of the
    # process's shared libraries)
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-static-libasan", "-static-libubsan", "-pthread",
           "-ffp-contract=off", "-I" + os.path.join(repo, "include"), "-I" + os.path.join(irt.PKG_DIR, "csrc"),
           os.path.join(irt.PKG_DIR, "host", "irt_section.cpp"),
           os.path.join(os.path.dirname(os.path.abspath(__file__)), "section_main.cpp"), "-o", exe]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "section_main: ok" in run.stdout
