"""The column products without a GPU: irt_column_reduce (host/irt_column.cpp) against a NumPy
restatement of its definition on the oracle's answers, the census of tests/test_gpu_column.py's
inputs by the oracle alone (so that the device comparison cannot pass on columns that exercise
nothing), the helper's refusals, and the helper under the address and undefined-behaviour
sanitizers in a stand-alone program (tests/column_reduce_main.cpp)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import column_scenes as CS
import irt
import levels_scenes as LS

F = np.float32


def first_last_found(found):
    """Per column the first and the last found level (L and -1 where none is)."""
    L = found.shape[0]
    ks = np.arange(L).reshape((L,) + (1,) * (found.ndim - 1))
    return np.where(found != 0, ks, L).min(0), np.where(found != 0, ks, -1).max(0)


def inside_levels(name, key):
    p = CS._parts(name)
    rad = CS.grid(name, key)[2]
    return int(((rad >= p.h0) & (rad <= p.top)).sum())


# ------------------------------------------------------------------ the reduction against NumPy
@pytest.mark.parametrize("wname", CS.WEIGHTS)
@pytest.mark.parametrize("key", list(CS.GRIDS))
@pytest.mark.parametrize("name", CS.SCENE_NAMES)
def test_column_reduce_is_the_numpy_restatement(name, key, wname):
    """... on the oracle's sample_volume answers, every output as bits (CS.reduced asserts it),
    with a finite and a NaN missValue."""
    r = CS.reduced(name, key, wname)
    f, v = CS.grid_answers(name, key)
    assert r["count"].shape == v.shape[1:] and r["wsum"].dtype == F and r["kmax"].dtype == np.int32
    assert np.array_equal(r["count"], (f != 0).sum(0))
    nan = irt.column_reduce(v, f, CS.weights(wname, v.shape[0]), float("nan"))
    assert CS.same_outputs(nan, CS.reduce_numpy(v, f, CS.weights(wname, v.shape[0]), float("nan"))) is None
    none = r["count"] == 0
    assert np.isnan(nan["wsum"][none]).all() and (r["vmax"][none] == F(CS.MISS)).all()
    assert (r["kmax"][none] == -1).all() and (r["kmin"][none] == -1).all() and (r["kmax"][~none] >= 0).all()


def test_reduction_ignores_values_of_levels_not_found():
    f, v = CS.grid_answers("terrain", "all")
    junk = np.where(f != 0, v, F(np.nan))
    assert CS.same_outputs(irt.column_reduce(junk, f, None, CS.MISS), CS.reduced("terrain", "all", "none")) is None


def test_a_nan_never_replaces_a_value_and_ties_keep_the_lower_level():
    v = np.array([[2, 5, np.nan, 1], [np.nan, 5, 3, 1], [1, 4, 2, 1]], F)
    r = irt.column_reduce(v, np.ones_like(v, np.uint8), None, CS.MISS)
    assert list(r["kmax"]) == [0, 0, 0, 0] and list(r["kmin"]) == [2, 2, 0, 0]
    assert np.isnan(r["vmax"][2]) and np.isnan(r["vmin"][2]) and r["vmax"][0] == 2 and r["vmin"][0] == 1


# ------------------------------------------------------------------ the census
def test_census_columns_without_with_some_and_with_all_levels():
    zero = sum(int((CS.reduced(n, k, "none")["count"] == 0).sum()) for n in CS.SCENE_NAMES for k in CS.GPU_GRIDS)
    assert int((CS.reduced("filtered", "all", "none")["count"] == 0).sum()) >= 100 and zero >= 200
    n_in = inside_levels("terrain", "all")
    c = CS.reduced("terrain", "all", "none")["count"]
    assert ((c > 0) & (c < n_in)).sum() >= 200  # over terrain: some of the inside levels
    for name in ("flat", "filtered"):
        c = CS.reduced(name, "all", "none")["count"]
        assert (c == inside_levels(name, "all")).sum() >= 80  # full columns
    for name in CS.SCENE_NAMES:  # the levels outside the shell are found nowhere
        f, _ = CS.grid_answers(name, "all")
        rad, p = CS.grid(name, "all")[2], CS._parts(name)
        assert not f[(rad == p.below) | (rad == p.above)].any()
        assert CS.reduced(name, "one", "none")["count"].shape == (1, 1)


def test_census_extremes_inside_the_column_and_apart():
    for name in CS.SCENE_NAMES:
        r = CS.reduced(name, "all", "none")
        first, last = first_last_found(CS.grid_answers(name, "all")[0])
        has = r["count"] > 0
        assert (has & (r["kmax"] != first) & (r["kmax"] != last)).sum() >= 50, name
        assert (has & (r["kmin"] != r["kmax"])).sum() >= 50, name


def test_census_a_tie_resolves_to_the_lower_index():
    """The duplicated radius gives two levels with the same points, so the same values; where that
    value is the column's extreme, the lower of the two indices holds it and the higher never."""
    n = 0
    for name in CS.SCENE_NAMES:
        for key in ("five", "all"):
            rad = CS.grid(name, key)[2]
            u, c = np.unique(rad, return_counts=True)
            a, b = np.flatnonzero(rad == u[c > 1][0])
            assert a < b
            f, v = CS.grid_answers(name, key)
            both = (f[a] != 0) & (f[b] != 0)
            assert np.array_equal(v[a][both], v[b][both]) and both.any()
            r = CS.reduced(name, key, "none")
            assert not (both & ((r["kmax"] == b) | (r["kmin"] == b))).any()
            n += int((both & ((r["kmax"] == a) | (r["kmin"] == a))).sum())
    assert n >= 50


def test_census_the_summation_order_is_tested():
    """Float32 sequential sums that differ from the float64 sum rounded once, and sums that differ
    between the ascending and the shuffled level order (weights permuted with the levels)."""
    for name in CS.SCENE_NAMES:
        for wname in ("none", "mixed"):
            f, v = CS.grid_answers(name, "all")
            w = CS.weights(wname, v.shape[0])
            w64 = np.ones(v.shape[0]) if w is None else w.astype(np.float64)
            s64 = (np.where(f != 0, v.astype(np.float64), 0.0) * w64[:, None, None]).sum(0).astype(F)
            r = CS.reduced(name, "all", wname)
            assert ((r["count"] > 1) & (CS.bits(s64) != CS.bits(r["wsum"]))).sum() >= 20, (name, wname)
        perm = CS.shuffle_of(name)
        assert np.array_equal(CS.levels(name, "shuffled"), CS.levels(name, "ascending")[perm])
        fa, va = CS.grid_answers(name, "all_ascending")
        fs, vs = CS.grid_answers(name, "all")
        assert np.array_equal(fs, fa[perm]) and np.array_equal(CS.bits(vs), CS.bits(va[perm]))
        w = CS.weights("mixed", len(perm))
        asc = irt.column_reduce(va, fa, w[np.argsort(perm)], CS.MISS)  # level perm[k] carries w[k] in both orders
        shuf = CS.reduced(name, "all", "mixed")
        assert np.array_equal(asc["count"], shuf["count"]) and np.array_equal(CS.bits(asc["vmax"]), CS.bits(shuf["vmax"]))
        assert (CS.bits(asc["wsum"]) != CS.bits(shuf["wsum"])).sum() >= 20, name
        plain = CS.reduced(name, "all_ascending", "none")["wsum"]
        assert (CS.bits(plain) != CS.bits(CS.reduced(name, "all", "none")["wsum"])).sum() >= 20, name


def test_census_weights_hold_a_zero_and_a_negative_value():
    for n in (5, CS.levels("flat", "shuffled").size, CS.levels("flat", "render").size):
        w = CS.weights("mixed", n)
        assert (w == 0).any() and (w < 0).any() and (w > 0).any() and np.isfinite(w).all()
    assert CS.weights("none", 5) is None and (CS.weights("ones", 5) == 1).all()


@pytest.mark.parametrize("case", CS.FRAMES, ids=CS.frame_id)
def test_census_every_frame_has_something_to_show(case):
    """The restatement's frames: pixels without a live hit (outside camera), pixels whose column
    found nothing though the hit is live, many found columns, several colours, and a product that
    is not one number."""
    name, view_name, size, accum_id, product, wname = case
    r = CS.expected_frame(*case)
    s = r.samples
    n = r.columns["count"]
    assert (n > 0).sum() >= 30 and np.unique(r.value[n > 0]).size >= 10 and np.unique(r.fb).size > 8
    assert (r.value[n == 0] == F(CS.MISS)).all() and (r.colour[n == 0] == 0).all()
    lo, hi = CS.VALUE_RANGE
    assert lo < r.value[n > 0].min() and r.value[n > 0].max() < hi
    if view_name == "outside":
        assert s.near[s.live].all() and s.live.any()
        assert size == "packet" or 20 <= (~s.live).sum()  # rays past the globe: no live hit
    else:
        assert s.live.all() and not s.near.any()  # inside the sphere: every ray leaves through it
    if name == "terrain":
        inside = int(np.isin(CS.levels(name, "render"), CS._parts(name).mids).sum())
        assert ((n > 0) & (n < inside)).sum() >= 10


def test_census_frames_differ_by_product_and_weights():
    a = CS.expected_frame("flat", "outside", "odd", 0, "wsum", "mixed")
    for other in (("max", "mixed"), ("min", "mixed"), ("wsum", "none")):
        b = CS.expected_frame("flat", "outside", "odd", 0, *other)
        assert not np.array_equal(a.fb, b.fb) and not np.array_equal(CS.bits(a.value), CS.bits(b.value))


def test_views_and_surface_are_where_the_frames_need_them():
    for name in ("flat", "terrain"):
        p = CS._parts(name)
        dist = lambda v: float(np.linalg.norm(np.array(LS.view(name, v)[0], np.float64)))  # noqa: E731
        assert float(p.h0) < dist("inside") < float(CS.surface(name)) < float(p.top) < dist("outside")
        r = CS.levels(name, "render")
        assert r.size == 12 and np.unique(r).size == 11 and (r < p.h0).any() and (r > p.top).any()


# ------------------------------------------------------------------ the host side
def test_column_reduce_refusals():
    L = irt.lib()
    v, f = np.ones((2, 4), F), np.ones((2, 4), np.uint8)
    out = {k: np.full(4, 77, t) for k, t in irt.COLUMN_OUTPUTS.items()}
    o = irt.ColumnOut(**{k: a.ctypes.data for k, a in out.items()})

    def refused(rc, word):
        assert rc == irt.E_INVALID and word in L.irt_last_error().decode(), L.irt_last_error()

    refused(L.irt_column_reduce(v.ctypes.data, f.ctypes.data, 0, 4, None, 0.0, o), "levels")
    refused(L.irt_column_reduce(v.ctypes.data, f.ctypes.data, -1, 4, None, 0.0, o), "levels")
    refused(L.irt_column_reduce(None, f.ctypes.data, 2, 4, None, 0.0, o), "null value or found")
    refused(L.irt_column_reduce(v.ctypes.data, None, 2, 4, None, 0.0, o), "null value or found")
    assert all((a == 77).all() for a in out.values())  # nothing written
    assert L.irt_column_reduce(None, None, 2, 0, None, 0.0, o) == 0  # no columns: no work
    assert L.irt_column_reduce(v.ctypes.data, f.ctypes.data, 2, 4, None, 0.0, irt.ColumnOut()) == 0
    assert all((a == 77).all() for a in out.values())
    only = irt.ColumnOut(count=out["count"].ctypes.data)
    assert L.irt_column_reduce(v.ctypes.data, f.ctypes.data, 2, 4, None, 0.0, only) == 0
    assert (out["count"] == 2).all() and (out["wsum"] == 77).all()
    with pytest.raises(irt.IrtError):
        irt.column_reduce(v, f[:1])
    with pytest.raises(irt.IrtError, match="weights"):
        irt.column_reduce(v, f, [1.0, 2.0, 3.0])
    assert C.sizeof(irt.ColumnOut) == 6 * C.sizeof(C.c_void_p)
    assert (irt.COLUMN_WSUM, irt.COLUMN_MAX, irt.COLUMN_MIN) == (0, 1, 2)


def test_column_reduce_under_the_sanitizers(tmp_path):
    """host/irt_column.cpp and tests/column_reduce_main.cpp as one program of their own, built with
    -fsanitize=address,undefined and run here (no code loaded into python is involved)."""
    cxx = shutil.which(os.environ.get("CXX", "g++"))
    assert cxx, "no C++ compiler"
    repo = os.path.dirname(os.path.abspath(irt.PKG_DIR))
    exe = str(tmp_path / "column_reduce_main")
    # (the sanitizers' runtimes linked into the program: nothing depends on the order of the
    # process's shared libraries)
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-static-libasan", "-static-libubsan",
           "-ffp-contract=off", "-I" + os.path.join(repo, "include"), "-I" + os.path.join(irt.PKG_DIR, "csrc"),
           os.path.join(irt.PKG_DIR, "host", "irt_column.cpp"),
           os.path.join(os.path.dirname(os.path.abspath(__file__)), "column_reduce_main.cpp"), "-o", exe]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "column_reduce_main: ok" in run.stdout
