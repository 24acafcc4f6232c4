"""Resampling without a GPU: irt_latlon_points against the oracle's toCartesian bit for bit, the
sampling calls' guard (irt_debug_sample_admits) on the points it exists for, the argument errors
that need no device, and the census of tests/test_gpu_sample.py's inputs by the oracle alone --
what keeps that test from passing on all-miss data."""
import ctypes as C

import numpy as np
import pytest

import irt
import sample_scenes as S

INVALID = -1


@pytest.mark.parametrize("shape", S.GRID_SHAPES, ids=str)
@pytest.mark.parametrize("name", ["flat", "filtered"])
def test_latlon_points_are_the_oracles_to_cartesian(name, shape):
    lat, lon, rad = S.grid(name, shape)
    got = S.grid_points(name, shape)
    assert got.shape == shape + (3,) and got.dtype == np.float32
    want = np.array([[[S.oracle_to_cartesian(r, a, o) for o in lon] for a in lat] for r in rad], np.float32)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_grids_hold_the_edge_angles_and_radii():
    """What the GPU test's grids must contain: +-pi/2 and 0 as latitudes, -pi, 0 and the float below
    pi as longitudes, and over the five grids height[0] and the top exactly, one float either side
    of each, a layer radius inside, one level below the shell and one above."""
    h0, top, inner = S.shell(S.scene("flat"))
    radii = np.concatenate([S.grid("flat", s)[2] for s in S.GRID_SHAPES])
    up, down = np.float32(np.inf), np.float32(0)
    for r in (h0, top, np.nextafter(h0, up), np.nextafter(h0, down), np.nextafter(top, up),
              np.nextafter(top, down), inner):
        assert (radii == r).any(), r
    assert (radii <= h0 - S.CENSUS_MARGIN).any() and (radii >= top + S.CENSUS_MARGIN).any()
    assert h0 < inner < top
    for shape in S.GRID_SHAPES[1:]:
        lat, lon, _ = S.grid("flat", shape)
        assert lat[0] == -np.float32(np.pi / 2) and lat[-1] == np.float32(np.pi / 2) and (lat == 0).any()
        assert lon[0] == -np.float32(np.pi) and (lon == 0).any()
        assert lon[-1] == np.nextafter(np.float32(np.pi), np.float32(0))
        assert (np.diff(lat) > 0).all() and (np.diff(lon) > 0).all()


def test_latlon_points_argument_errors():
    L = irt.lib()
    one = np.zeros(1, np.float32)
    out = np.zeros(3, np.float32)
    p = irt._ptr
    assert L.irt_latlon_points(p(one), -1, p(one), 1, p(one), 1, p(out)) == INVALID
    assert b"negative" in L.irt_last_error()
    assert L.irt_latlon_points(p(one), 1, p(one), 1, p(one), 1, None) == INVALID
    assert L.irt_latlon_points(None, 1, p(one), 1, p(one), 1, p(out)) == INVALID
    # 2^12 x 2^12 x 2^13 = 2^37 points: refused before any array is read
    assert L.irt_latlon_points(p(one), 1 << 12, p(one), 1 << 12, p(one), 1 << 13, p(out)) == INVALID
    assert b"2^36" in L.irt_last_error()
    # a zero count: nothing to do, nothing read or written
    assert L.irt_latlon_points(None, 0, None, 5, None, 5, None) == 0


NAN, INF = float("nan"), float("inf")


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_guard_rejects_non_finite_coordinates(axis):
    for bad in (NAN, INF, -INF):
        p = [6.4e6, -1.0e6, 2.0e6]
        p[axis] = bad
        assert not irt.sample_admits(*p), p
    for zero in (0.0, -0.0):  # a zero coordinate is an ordinary one
        p = [6.4e6, -1.0e6, 2.0e6]
        p[axis] = zero
        assert irt.sample_admits(*p), p
        q = [zero, zero, zero]
        assert not irt.sample_admits(*q), q


def test_guard_on_lengths_that_overflow_or_vanish():
    assert not irt.sample_admits(0.0, 0.0, 0.0)      # the origin
    assert not irt.sample_admits(-0.0, 0.0, -0.0)
    assert not irt.sample_admits(3e38, 0.0, 0.0)     # finite, but x * x = inf
    assert not irt.sample_admits(0.0, -3e38, 0.0)
    assert not irt.sample_admits(1.5e19, 1.5e19, 1.5e19)  # each square finite, their sum not
    assert not irt.sample_admits(1e-30, 0.0, 0.0)    # x * x underflows to 0
    assert not irt.sample_admits(0.0, 0.0, -1e-30)
    assert irt.sample_admits(1e-20, 0.0, 0.0)        # a denormal squared length is positive
    assert irt.sample_admits(1e19, 0.0, 0.0)
    for p in ((6.371229e6, 0.0, 0.0), (-3.1e6, 4.2e6, -3.6e6), (1.0, 2.0, 3.0), (0.0, 0.0, -6.4e6)):
        assert irt.sample_admits(*p), p
    assert [irt.sample_admits(*p) for p in S.GUARD_POINTS] == [False] * len(S.GUARD_POINTS)


def test_sampling_calls_reject_bad_arguments_without_a_device():
    L = irt.lib()
    one = np.zeros(1, np.float32)
    p = irt._ptr
    nan = C.c_float(NAN)
    assert L.irt_sample_points(None, 0, None, 0, None, None, nan, None) == INVALID
    assert b"irt_sample_points" in L.irt_last_error()
    assert L.irt_sample_points(None, 0, p(one), 1, p(one), None, nan, None) == INVALID
    assert L.irt_sample_latlon(None, 0, p(one), 1, p(one), 1, p(one), 1, p(one), None, nan, None) == INVALID
    assert b"irt_sample_latlon" in L.irt_last_error()
    assert L.irt_sample_latlon(None, 0, p(one), -1, p(one), 1, p(one), 1, p(one), None, nan, None) == INVALID


# ------------------------------------------------------------------ the census
@pytest.mark.parametrize("name", S.SCENE_NAMES)
def test_census_locator_points(name):
    """The oracle finds more than a third of the points and misses at least one (the bar of
    test_gpu_parity._locator_check); the guard points with a reference answer are misses."""
    found, value = S.cell_answers(name)
    n = len(found) - len(S.GUARD_POINTS)
    print(f"{name}: {n} points, oracle finds {int(found[:n].sum())}")
    assert found[:n].sum() > n // 3 and (found[:n] == 0).any()
    assert not found[n:].any()
    assert len(np.unique(value[:n][found[:n] != 0])) > 50  # and the values tell cells apart


def _levels(name):
    """(shape, level index, radius, fraction found by the oracle) of every grid level."""
    for shape in S.GRID_SHAPES:
        rad = S.grid(name, shape)[2]
        found = S.grid_answers(name, shape)[0].reshape(shape[0], -1)
        for k in range(shape[0]):
            yield shape, k, rad[k], float(found[k].mean())


def test_census_grids_on_the_globe():
    """Over the unfiltered flat globe the triangles tile the sphere: a level strictly inside the
    shell is found nearly everywhere (the margin is for plane-test rounding on shared edges), a
    level below or above the shell nowhere."""
    h0, top, _ = S.shell(S.scene("flat"))
    inside = outside = 0
    for shape, k, r, frac in _levels("flat"):
        print(f"flat {shape} level {k} r = {float(r)!r}: {frac:.4f} found")
        if h0 < r < top:
            assert frac >= 0.99, (shape, k)
            inside += 1
        elif r <= h0 - S.CENSUS_MARGIN or r >= top + S.CENSUS_MARGIN:
            assert frac == 0.0, (shape, k)
            outside += 1
    assert inside >= 5 and outside >= 2


def test_census_grids_on_the_filtered_scene():
    """A lat/lon window of the globe: on an interior level some grid points are found, some not."""
    h0, top, _ = S.shell(S.scene("filtered"))
    mixed = 0
    for shape, k, r, frac in _levels("filtered"):
        print(f"filtered {shape} level {k} r = {float(r)!r}: {frac:.4f} found")
        if h0 < r < top and shape[1] * shape[2] > 1:
            assert 0.0 < frac < 1.0, (shape, k)
            mixed += 1
    assert mixed >= 4
