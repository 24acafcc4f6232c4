"""The field's histogram without a GPU: irt_histogram_cells (host/irt_histogram.cpp, the definition of
csrc/irt_histogram.h) against a NumPy restatement on every input of tests/histogram_scenes.py, the
conservation identity, the census of those inputs by the helper alone (so that the device comparison
of tests/test_gpu_histogram.py cannot pass on inputs that take no branch), the helper's refusals, and
the helper under the address and undefined-behaviour sanitizers in a stand-alone program
(tests/histogram_main.cpp)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import histogram_scenes as HS
import irt

F = np.float32
ALL_SCENES = HS.SCENE_NAMES + tuple(f"hand{n}" for n in HS.COUNTS) + ("large",)


def total(r):
    return int(r["bins"].sum(dtype=np.uint64)) + int(r["tails"].sum(dtype=np.uint64)) + int(r["outside"][0])


# ------------------------------------------------------------------ the helper against NumPy
@pytest.mark.parametrize("name", ALL_SCENES)
def test_histogram_cells_is_the_numpy_restatement(name):
    """Every (range, bins, band set, weighting) of the scene: the same integers, and the sum of bins,
    tails and outside is the sum of the weights (count mode without bands: the sum of numLayers)."""
    cells = HS.scene(name)
    cases = HS.cases(name) if name != "large" else [("data", 300, "none", "count"), ("inner", 7, "three", "thickness")]
    for rk, bins, bk, w in cases:
        want = HS.numpy_histogram(cells, HS.value_range(name, rk), bins, w, HS.band_edges(name, bk))
        got = HS.expected(name, rk, bins, bk, w)
        bands = 1 if bk == "none" else len(HS.band_edges(name, bk)) - 1
        assert got["bins"].shape == (bands, bins) and got["tails"].shape == (bands, 3) and got["bins"].dtype == np.uint64
        assert HS.differs(got, want) is None, (name, rk, bins, bk, w, HS.differs(got, want))
        assert total(got) == want["weight_sum"], (name, rk, bins, bk, w)
        if w == "count":
            assert total(got) == int(cells["numLayers"].sum())


@pytest.mark.parametrize("name", HS.SCENE_NAMES)
def test_the_data_range_leaves_the_value_tails_empty(name):
    for w in HS.WEIGHTINGS:
        r = HS.expected(name, "data", 300, "none", w)
        assert np.isfinite(HS.scene(name)["value"]).all()
        assert r["tails"].sum() == 0
        assert w != "count" or (r["bins"][0, 0] > 0 and r["bins"][0, -1] > 0)  # the minimum and, by the clamp, the maximum
        inner = HS.expected(name, "inner", 300, "none", w)
        assert inner["tails"][0, 0] > 0 and inner["tails"][0, 1] > 0 and inner["tails"][0, 2] == 0


# ------------------------------------------------------------------ the census
def test_census_every_tail_and_outside_are_reached():
    r = HS.expected("hand257", "data", 7, "three", "count")
    assert (r["tails"].sum(0) > 0).all() and r["outside"][0] > 0
    one = HS.expected("hand1", "data", 7, "none", "count")  # record 0 alone holds every special value
    # under: -0.0 and the float below lower; over: the float above upper; not finite: NaN and both infinities
    assert (one["tails"][0] == [2, 1, 3]).all() and total(one) == 31
    for name in HS.SCENE_NAMES:
        r = HS.expected(name, "inner", 7, "three", "thickness")
        assert r["outside"][0] > 0 and r["tails"][:, :2].sum() > 0, name


def test_census_the_last_bin_by_equality_and_by_the_clamp():
    """t == 1 (v == upper) reaches bin numBins - 1 only through the clamp of k = numBins; a value
    inside the last bin reaches it without.  Both are among record 0's values."""
    lo, hi = HS.HAND_RANGE
    for nb in (2, 7, 300, 4096):
        sp = HS.special_values()
        t = ((sp - lo) / (hi - lo)).astype(F)
        with np.errstate(invalid="ignore"):
            k = (t * F(nb)).astype(F)
        ok = np.isfinite(sp) & (t >= 0) & (t <= 1)
        assert (k[ok] == nb).sum() == 1 and ((k[ok] >= nb - 1) & (k[ok] < nb)).sum() >= 1, nb
        r = HS.expected("hand1", "data", nb, "none", "count")
        assert r["bins"][0, -1] >= 2
    # -0.0 is under the hand-made range; with lower = 0 it is t = -0.0, not < 0: bin 0
    cells = np.array(HS.scene("hand1"), copy=True)
    cells["value"][0][:] = F(-0.0)
    r = irt.histogram_cells(cells, (0.0, 1.0), 7, "count")
    assert r["bins"][0, 0] == 31 and r["tails"].sum() == 0


def test_census_weightless_items_are_dropped_and_thickness_differs_from_count():
    cells = HS.scene("terrain")
    h0, h1, _ = HS.layers(cells)
    d = h1 - h0
    assert (d <= 0).sum() > 0  # inverted first layers, zero-thickness records
    cnt, thk = HS.expected("terrain", "data", 7, "none", "count"), HS.expected("terrain", "data", 7, "none", "thickness")
    assert total(cnt) == d.size
    assert total(thk) == int((np.where(d > 0, d, F(0)) * F(64)).astype(np.uint64).sum(dtype=np.uint64))
    c, t = [int(x) for x in cnt["bins"][0]], [int(x) for x in thk["bins"][0]]
    assert any(a * sum(t) != b * sum(c) for a, b in zip(c, t))  # another distribution, not a scaled copy
    hand = HS.scene("hand257")
    assert (hand["numLayers"] == 0).sum() >= 1 and (hand["numLayers"] == 1).sum() >= 1 and (hand["numLayers"] == 31).sum() >= 1
    zero = HS.expected("hand4", "data", 7, "none", "thickness")
    part = irt.histogram_cells(HS.scene("hand4")[:3], HS.HAND_RANGE, 7, "thickness")
    assert HS.differs(zero, part) is None  # the zero-thickness record 3 adds nothing


@pytest.mark.parametrize("name", HS.SCENE_NAMES + ("hand257",))
def test_census_three_bands_one_empty_one_edge_on_a_layer(name):
    e = HS.band_edges(name, "three")
    m = HS.mids(HS.scene(name))
    assert e.size == 4 and (np.diff(e) > 0).all()
    assert (m == e[1]).sum() > 0 and (m < e[1]).sum() > 0        # both sides of `<=` / `<` at an edge
    assert ((m >= e[2]) & (m < e[3])).sum() == 0 and (m >= e[3]).sum() > 0
    r = HS.expected(name, "data", 7, "three", "count")
    assert r["bins"][2].sum() + r["tails"][2].sum() == 0 and r["outside"][0] == (m >= e[3]).sum()
    assert r["bins"][1].sum() + r["tails"][1].sum() == ((m >= e[1]) & (m < e[2])).sum()
    many = HS.expected(name, "data", 64, "sixtyfour", "count")
    assert many["outside"][0] == 0 and ((many["bins"].sum(1) + many["tails"].sum(1)) > 0).sum() >= 8


# ------------------------------------------------------------------ the host side
def test_histogram_cells_refusals():
    L = irt.lib()
    cells = np.array(HS.scene("hand65"), copy=True)
    out = {"bins": np.full(4096, 77, np.uint64), "tails": np.full(192, 77, np.uint64), "outside": np.full(1, 77, np.uint64)}
    o = irt.HistogramOut(**{k: a.ctypes.data for k, a in out.items()})
    edges = np.array([6.3e6, 6.4e6, 6.5e6, 6.6e6], F)

    def call(rng=(0.0, 1.0), bins=7, w=0, e=None, bands=1, cells=cells, n=None, o=o):
        return L.irt_histogram_cells(cells.ctypes.data if cells is not None else None, cells.size if n is None else n,
                                     irt.box1(*rng), bins, w, e.ctypes.data if e is not None else None, bands, o)

    def refused(rc, word):
        assert rc == irt.E_INVALID and word in L.irt_last_error().decode(), L.irt_last_error()

    for bins in (0, -1, 4097):
        refused(call(bins=bins), "bins are outside")
    for bands in (0, -3, 65):
        refused(call(e=edges, bands=bands), "bands are outside")
    refused(call(bins=2048, e=edges, bands=3), "more than 4096 counters")
    refused(call(bins=65, e=np.linspace(6.3e6, 6.5e6, 65).astype(F), bands=64), "more than 4096 counters")
    for rng in ((1.0, 1.0), (2.0, 1.0), (np.nan, 1.0), (0.0, np.nan), (-np.inf, 1.0), (0.0, np.inf)):
        refused(call(rng=rng), "valueRange")
    for w in (-1, 2):
        refused(call(w=w), "weighting")
    refused(call(bands=3), "null bandEdges")
    for k, bad in ((0, np.nan), (1, np.inf), (3, -np.inf), (2, 6.4e6), (2, 6.3e6)):
        e = edges.copy()
        e[k] = bad
        refused(call(e=e, bands=3), "bandEdges[")
    refused(call(cells=None, n=5), "null cells")
    wrong = cells.copy()
    wrong["numLayers"][7] = 32
    assert call(cells=wrong) == irt.E_DATA and "numLayers" in L.irt_last_error().decode()
    assert all((a == 77).all() for a in out.values())  # nothing written
    assert call(o=irt.HistogramOut()) == 0 and call(cells=None, n=0) == 0
    assert out["bins"][:7].sum() == 0 and out["bins"][7] == 77 and out["outside"][0] == 0  # no records: zeroes
    for k in out:  # each output alone
        out[k][:] = 77
    assert call(o=irt.HistogramOut(tails=out["tails"].ctypes.data)) == 0
    whole = irt.histogram_cells(cells, (0.0, 1.0), 7)
    assert (out["tails"][:3] == whole["tails"][0]).all() and whole["tails"].sum() + whole["bins"].sum() == cells["numLayers"].sum()
    assert (out["bins"] == 77).all() and out["tails"][3] == 77
    assert call(e=edges, bands=3) == 0 and call(bins=4096) == 0 and call(bins=64, e=np.linspace(6.3e6, 6.5e6, 65).astype(F), bands=64) == 0
    with pytest.raises(irt.IrtError, match="weighting"):
        irt.histogram_cells(cells, (0, 1), 7, "volume")
    with pytest.raises(irt.IrtError, match="band edges"):
        irt.histogram_cells(cells, (0, 1), 7, "count", [6.4e6])
    assert C.sizeof(irt.HistogramOut) == 3 * C.sizeof(C.c_void_p) and (irt.HIST_COUNT, irt.HIST_THICKNESS) == (0, 1)


def test_histogram_cells_under_the_sanitizers(tmp_path):
    """host/irt_histogram.cpp and tests/histogram_main.cpp as one program of their own, built with
    -fsanitize=address,undefined and run here (no code loaded into python is involved)."""
    cxx = shutil.which(os.environ.get("CXX", "g++"))
    assert cxx, "no C++ compiler"
    repo = os.path.dirname(os.path.abspath(irt.PKG_DIR))
    exe = str(tmp_path / "histogram_main")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-static-libasan", "-static-libubsan",
           "-ffp-contract=off", "-I" + os.path.join(repo, "include"), "-I" + os.path.join(irt.PKG_DIR, "csrc"),
           os.path.join(irt.PKG_DIR, "host", "irt_histogram.cpp"),
           os.path.join(os.path.dirname(os.path.abspath(__file__)), "histogram_main.cpp"), "-o", exe]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "histogram_main: ok" in run.stdout
