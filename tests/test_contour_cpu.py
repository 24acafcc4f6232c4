"""The isolines' host side (host/irt_contour.cpp, include/icon_rt_hip.h "isolines") without a GPU:
irt_contour_cells against the float64 NumPy restatement of tests/contour_scenes.py byte for byte, a
census of the fields (so that the device comparison of tests/test_gpu_contour.py cannot pass on empty
output or untaken branches), the properties of closed isolines on the wrapped smooth field, every
refusal, and the helper under the address and undefined-behaviour sanitizers in a stand-alone program
(tests/contour_main.cpp)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import contour_scenes as CS
import irt

F = np.float32
D = np.float64


@pytest.mark.parametrize("name,wrap", CS.CASES, ids=CS.CASE_IDS)
def test_cells_equal_the_restatement(name, wrap):
    seg, per = CS.host(name, wrap)
    want = CS.restate(name, wrap)
    print(f"{name} wrap={wrap}: {seg.size} segments, per threshold {per.tolist()}, {want.dropped} dropped")
    assert per.tolist() == want.per.tolist() and seg.size == want.per.sum()
    CS.same_bytes(seg, want.segments, f"{name} wrap={wrap}")
    assert (seg["pad"] == 0).all()
    # the order: threshold, then cell, then within the cell
    start = 0
    for n in want.per:
        assert (np.diff(want.cell[start:start + n]) >= 0).all()
        start += n


def test_census_of_the_fields():
    masks = set()
    for name, wrap in CS.CASES:
        f, r = CS.field(name), CS.restate(name, wrap)
        masks |= r.masks
        finite = f.value[np.isfinite(f.value)]
        for c, n in zip(f.thresholds, r.per):
            if finite.min() < c < finite.max():
                assert n >= 1, f"{name} wrap={wrap}: no segment at {c}"
    assert CS.restate("checker", False).saddles == {(5, True), (5, False), (10, True), (10, False)}
    assert CS.restate("checker", False).masks == {5, 10} and (CS.restate("checker", False).per == 2 * 11 * 15).all()
    assert CS.restate("oncorner", False).dropped >= 1
    assert CS.restate("poles", False).dropped >= 1 and CS.restate("poles", True).dropped >= 1
    assert CS.restate("holes", False).suppressed >= 1 and CS.restate("holes", True).suppressed >= 1
    # the hole in the wrap column takes segments away that the wrapped smooth field has
    assert CS.restate("holes", True).per.sum() < CS.restate("smooth", True).per.sum()
    assert masks == set(range(1, 15))
    # the sizes the kernels' paths turn on (contour_scenes' docstring)
    cells = lambda n, w: (CS.field(n).lat.size - 1) * CS.restate(n, w).cells_lon  # noqa: E731
    assert cells("smooth", True) == 2412 and cells("smooth", True) % 64 and cells("smooth", True) > 4 * 256
    assert cells("tiny1", False) == 1 and cells("tiny3x5", False) == 8
    assert -(-cells("wide", True) // 256) > 256 and CS.field("wide").thresholds.size == 16


# ------------------------------------------------------------------ properties on smooth, wrapped
def test_isolines_of_the_wrapped_smooth_field_are_closed_chains_on_the_field():
    """Every end point appears exactly twice among a threshold's segments (once as an a, once as a b:
    the shared-edge rule); the field at each end point is within 1e-5 of the threshold; every arc is at
    most 0.2 rad.  "The field" is the grid's: linear along a cell edge in the chord parameter, which is
    what an isoline of gridded data follows (the analytic z + 0.3 x y differs from its own interpolant
    by the square of the 0.09 rad step, 1e-3).  The check finds the edge and the parameter from the
    end point alone."""
    f, r = CS.field("smooth"), CS.restate("smooth", True)
    seg, per = CS.host("smooth", True)
    P = CS.corners(f.lat, f.lon)
    nlon = f.lon.size
    start = 0
    for c, n in zip(f.thresholds, per):
        s, cell = seg[start:start + n], r.cell[start:start + n]
        start += n
        ends = np.concatenate([s["a"], s["b"]]).view(np.uint32).reshape(-1, 3)
        _, counts = np.unique(ends, axis=0, return_counts=True)
        assert (counts == 2).all(), f"threshold {c}: {np.bincount(counts)} end points by multiplicity"
        assert len(np.unique(s["a"].view(np.uint32).reshape(-1, 3), axis=0)) == n  # each once as a, once as b
        worst = 0.0
        for which in ("a", "b"):
            for p, cl in zip(s[which].astype(D), cell):
                j, i = divmod(int(cl), nlon)
                i1 = (i + 1) % nlon
                at = ((j, i), (j, i1), (j + 1, i1), (j + 1, i))
                best = None
                for ca, cb in CS.EDGES:
                    A, B = P[at[ca]], P[at[cb]]
                    nrm = np.cross(A, B)
                    off = abs(p @ nrm) / np.linalg.norm(nrm)      # the distance from the edge's great circle
                    pa, pb = np.linalg.norm(np.cross(p, A)), np.linalg.norm(np.cross(p, B))
                    t = pa / (pa + pb)
                    inside = pa + pb <= np.linalg.norm(np.cross(A, B)) * 1.01  # (sines of the two parts: a little over)
                    if inside and (best is None or off < best[0]):
                        best = (off, float(f.value[at[ca]]) + t * (float(f.value[at[cb]]) - float(f.value[at[ca]])))
                assert best is not None and best[0] < 1e-6, "an end point off every edge of its cell"
                worst = max(worst, abs(best[1] - float(c)))
        print(f"threshold {c}: {n} segments, field at the end points within {worst:.2e}")
        assert worst <= 1e-5
    arc = 2 * np.arcsin(seg["sinHalf"].astype(D))
    chord = np.linalg.norm(seg["b"].astype(D) - seg["a"].astype(D), axis=1)
    assert arc.max() <= 0.2 and np.abs(2 * seg["sinHalf"] - chord).max() < 1e-6
    # unit fields, n normal to both ends, t along the chord, the high side on the left
    for k in ("a", "b", "n", "t"):
        assert np.abs(np.linalg.norm(seg[k].astype(D), axis=1) - 1).max() < 1e-6
    assert max(np.abs((seg["n"] * seg["a"]).sum(1)).max(), np.abs((seg["n"] * seg["b"]).sum(1)).max()) < 1e-5
    mid = seg["a"].astype(D) + seg["b"].astype(D)
    left = mid / np.linalg.norm(mid, axis=1, keepdims=True) + 0.02 * seg["n"]  # n = a x b points to the left
    left /= np.linalg.norm(left, axis=1, keepdims=True)
    high = left[:, 2] + 0.3 * left[:, 0] * left[:, 1]
    assert (high > np.repeat(f.thresholds, per)).all()


def test_the_overlay_accepts_the_segments():
    for name, wrap in (("smooth", True), ("poles", True), ("oncorner", False)):
        seg, _ = CS.host(name, wrap)
        assert seg["style"].min() >= 0 and seg["style"].max() < irt.OVERLAY_MAX_STYLES  # overlay_segments_ok
        assert np.isfinite(np.concatenate([seg[k].ravel() for k in ("a", "b", "n", "t", "sinHalf")])).all()
        start, lists = irt.overlay_bins(seg, 0.01, 8)
        assert start[-1] == lists.size >= seg.size
        # a segment's own midpoint is covered by it or by an earlier one
        mid = seg["a"] + seg["b"]
        mid = (mid / np.linalg.norm(mid, axis=1, keepdims=True)).astype(F)
        styles = [((1, 1, 1, 1), 0.01)] * irt.OVERLAY_MAX_STYLES
        got = irt.overlay_cover(seg, styles, mid, (start, lists), 8)
        assert (got >= 0).all() and (got <= np.arange(seg.size)).all()


def test_repeated_and_unordered_thresholds():
    f = CS.field("smooth")
    one = irt.contour_cells(f.value, None, f.lat, f.lon, [0.35], [3], True)
    other = irt.contour_cells(f.value, None, f.lat, f.lon, [-0.6], [1], True)
    seg, per = irt.contour_cells(f.value, None, f.lat, f.lon, [0.35, -0.6, 0.35], [3, 1, 3], True, return_counts=True)
    assert per.tolist() == [one.size, other.size, one.size] and one.size > 0 and other.size > 0
    CS.same_bytes(seg, np.concatenate([one, other, one]), "a threshold given twice")


# ------------------------------------------------------------------ refusals
def test_refusals_write_nothing():
    L = irt.lib()
    f = CS.field("smooth")
    p = lambda a: C.c_void_p(a.ctypes.data) if a is not None else None  # noqa: E731
    guard = 4
    out = np.zeros(1024 + 2 * guard, irt.SEGMENT_DTYPE)
    out["style"] = 77
    n = C.c_size_t(12345)
    per = np.full(16, 999, np.uintp)
    thr, sty = np.array(CS.SMOOTH_T, F), np.arange(4, dtype=np.int32)

    def call(value=f.value, found=None, lat=f.lat, nlat=None, lon=f.lon, nlon=None, thr=thr, sty=sty, T=None, flags=1,
             out=out, cap=1024, count=n, per=per):
        o = C.c_void_p(out.ctypes.data + 64 * guard) if out is not None else None
        return L.irt_contour_cells(p(value), p(found), p(lat), lat.size if nlat is None else nlat, p(lon),
                                   lon.size if nlon is None else nlon, p(thr), p(sty), thr.size if T is None else T,
                                   flags, o, cap, C.byref(count) if count is not None else None, p(per))

    def refused(rc, word):
        assert rc == irt.E_INVALID and word in L.irt_last_error().decode(), L.irt_last_error()
        assert (out["style"] == 77).all() and n.value == 12345 and (per == 999).all()

    refused(call(count=None), "null count")
    for flags in (2, 3, -1, 1 << 20):
        refused(call(flags=flags), "unknown flag bits")
    refused(call(nlat=1), "at least 2 x 2")
    refused(call(nlon=1), "at least 2 x 2")
    refused(call(nlat=1 << 14, nlon=1 << 13), "2^27")
    refused(call(T=0), "thresholds are outside")
    refused(call(T=17, thr=np.zeros(17, F), sty=np.zeros(17, np.int32)), "thresholds are outside")
    for k in ("value", "lat", "lon", "thr", "sty"):
        refused(call(**{k: None, **({"nlat": 37} if k == "lat" else {}), **({"nlon": 67} if k == "lon" else {}),
                        **({"T": 4} if k in ("thr", "sty") else {})}), "null")
    for bad in (np.nan, np.inf):
        refused(call(thr=np.array([0.0, bad], F), sty=sty[:2]), "not finite")
        lat = f.lat.copy()
        lat[3] = bad
        refused(call(lat=lat), "not finite")
    for style in (-1, irt.OVERLAY_MAX_STYLES):
        refused(call(sty=np.array([0, 1, style, 0], np.int32)), "style[2]")
    lat = f.lat.copy()
    lat[5] = lat[4]
    refused(call(lat=lat), "ascend")
    refused(call(lat=f.lat[::-1].copy()), "ascend")
    refused(call(lat=(f.lat * F(1.3)).astype(F)), "ascend by at most")  # steps of 0.108 rad
    lon = f.lon.copy()
    lon[7] = lon[9]
    refused(call(lon=lon), "ascend")
    # wrap: the 53 columns of smooth53 leave a closing step of 1.09 rad; a grid past the full circle
    g = CS.field("smooth53")
    refused(call(value=g.value, lon=g.lon), "closing step")
    assert call(value=g.value, lon=g.lon, flags=0, out=None) == 0 and n.value == CS.host("smooth53", False)[0].size
    n.value, per[:] = 12345, 999
    over = (np.arange(70) * 0.0999 - 3.4).astype(F)  # spans 6.89 rad
    refused(call(value=np.zeros((37, 70), F), lon=over), "closing step")
    # a short array: the count is set, nothing else written
    assert call(cap=10) == irt.E_INVALID and "capacity" in L.irt_last_error().decode()
    assert n.value == CS.host("smooth", True)[0].size and per[:4].tolist() == CS.host("smooth", True)[1].tolist()
    assert (out["style"] == 77).all()
    # ... and the same call with room writes exactly count segments between the guards
    assert call() == 0
    assert (out["style"][:guard] == 77).all() and (out["style"][guard + n.value:] == 77).all()
    CS.same_bytes(out[guard:guard + n.value], CS.host("smooth", True)[0], "into a guarded buffer")
    assert call(per=None) == 0 and call(out=None, per=None) == 0
    assert irt.CONTOUR_WRAP == 1 and irt.CONTOUR_MAX_THRESHOLDS == 16


def test_two_to_the_24_segments_are_refused():
    """A checkerboard of 727 x 727 points at 16 thresholds: 2 * 16 * 726^2 = 16,866,432 >= 2^24."""
    L = irt.lib()
    N = 727
    lat = np.linspace(-0.5, 0.5, N).astype(F)
    lon = np.linspace(-0.5, 0.5, N).astype(F)
    j, i = np.meshgrid(np.arange(N), np.arange(N), indexing="ij")
    v = np.where((i + j) % 2 == 0, 1.0, -1.0).astype(F)
    thr, sty = np.linspace(-0.5, 0.5, 16).astype(F), np.zeros(16, np.int32)
    n, per = C.c_size_t(12345), np.full(16, 999, np.uintp)
    p = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    rc = L.irt_contour_cells(p(v), None, p(lat), N, p(lon), N, p(thr), p(sty), 16, 0, None, 0, C.byref(n), p(per))
    assert rc == irt.E_INVALID and "2^24" in L.irt_last_error().decode()
    assert n.value == 12345 and (per == 999).all()
    # 15 thresholds stay below: 15,812,280 segments
    rc = L.irt_contour_cells(p(v), None, p(lat), N, p(lon), N, p(thr), p(sty), 15, 0, None, 0, C.byref(n), p(per))
    assert rc == 0 and n.value == 2 * 15 * 726 * 726 and (per[:15] == 2 * 726 * 726).all()


# ------------------------------------------------------------------ sanitizers
def test_contour_helper_under_the_sanitizers(tmp_path):
    """host/irt_contour.cpp and tests/contour_main.cpp as one program of their own, built with
    -fsanitize=address,undefined and run here (no code loaded into python is involved)."""
    cxx = shutil.which(os.environ.get("CXX", "g++"))
    assert cxx, "no C++ compiler"
    repo = os.path.dirname(os.path.abspath(irt.PKG_DIR))
    exe = str(tmp_path / "contour_main")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-static-libasan", "-static-libubsan",
           "-ffp-contract=off", "-I" + os.path.join(repo, "include"), "-I" + os.path.join(irt.PKG_DIR, "csrc"),
           os.path.join(irt.PKG_DIR, "host", "irt_contour.cpp"),
           os.path.join(os.path.dirname(os.path.abspath(__file__)), "contour_main.cpp"), "-o", exe]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "contour_main: ok" in run.stdout
