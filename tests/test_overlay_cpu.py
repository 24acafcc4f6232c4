"""The overlay without a GPU: irt_overlay_segments and irt_graticule against a float64 NumPy
restatement, the axis convention against irt_latlon_points, irt_overlay_cover against the true angular
distance to the arcs, the bins against the all-segments scan integer for integer, the census of the
inputs of tests/overlay_scenes.py by the helpers alone (so that the device comparison of
tests/test_gpu_overlay.py cannot pass on inputs that take no branch), every refusal, and the four
helpers under the address and undefined-behaviour sanitizers in a stand-alone program
(tests/overlay_main.cpp)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import irt
import overlay_scenes as OS

F = np.float32
TOL = 3e-7   # a float's rounding of a unit vector's component (6e-8) and of the restatement's libm
BAND = 1e-3  # the share of W left undecided on either side of the line's edge


# ------------------------------------------------------------------ segments against float64
def check_fields(seg, want):
    assert seg.size == len(want)
    for k, name in enumerate(("a", "b", "n", "t")):
        ref = np.array([w[k] for w in want])
        got = seg[name].astype(np.float64)
        assert np.abs(got - ref).max() <= TOL, name
        assert np.abs(np.linalg.norm(got, axis=1) - 1).max() <= TOL, name
    n, a, b, t = (seg[k].astype(np.float64) for k in ("n", "a", "b", "t"))
    for x, y in ((n, a), (n, b), (t, n)):
        assert np.abs((x * y).sum(1)).max() <= TOL
    assert np.abs(seg["sinHalf"] - np.array([w[4] for w in want])).max() <= 1e-7
    assert (seg["style"] == [w[5] for w in want]).all() and (seg["pad"] == 0).all()


@pytest.mark.parametrize("name", [n for n in OS.SET_NAMES if n not in ("none", "graticule")])
def test_segments_are_the_float64_restatement(name):
    want = []
    for lat, lon, arc, style in OS.polylines(name):
        want += OS.restate_segments(lat, lon, arc, style)
    check_fields(OS.segments(name), want)


def test_piece_counts_and_merging():
    deg = OS.RAD
    lat, lon = np.array([0, 0, 0, 10, 10], F) * F(deg), np.array([0, 0, 12.5, 12.5, 12.5], F) * F(deg)
    seg = irt.overlay_segments(lat, lon, None, 5 * deg, 1)
    assert seg.size == 3 + 2  # 12.5 degrees in 3 pieces, 10 in 2; the repeated points are merged away
    check_fields(seg, OS.restate_segments(lat, lon, 5 * deg, 1))
    assert np.allclose(seg["sinHalf"][:3], np.sin(0.5 * 12.5 * deg / 3), atol=1e-7)
    assert np.array_equal(seg["b"][0], seg["a"][1]) and np.array_equal(seg["b"][2], seg["a"][3])
    # two lines: no segment joins them; a line of one point, or of equal points, gives none
    two = irt.overlay_segments(lat, lon, [0, 3, 5], 0.2, 0)
    assert two.size == 2 and np.array_equal(two["a"][0], seg["a"][0])  # 12.5 degrees in 2 pieces of at most 0.2 rad
    assert irt.overlay_segments(lat[:1], lon[:1]).size == 0 and irt.overlay_segments([], []).size == 0
    # points whose float unit vectors are equal although their angles differ
    tiny = irt.overlay_segments(np.array([0.5, 0.5 + 1e-9], F), np.array([1.0, 1.0], F))
    assert tiny.size == 0


def test_graticule_is_the_restatement():
    deg = OS.RAD
    seg = OS.segments("graticule")
    mer, par = int(np.ceil(np.pi / (5 * deg * 0.9999))), int(np.ceil(2 * np.pi / (5 * deg * 0.9999)))
    assert (mer, par) == (37, 73) and seg.size == 12 * mer + 5 * par
    want = []
    for m in range(12):
        lat = (-0.5 * np.pi + np.pi * np.arange(mer + 1) / mer).astype(F)
        want += OS.restate_segments(lat, np.full(mer + 1, m * float(F(30 * deg)), F), 5 * deg, 0)
    for k in range(-2, 3):
        lon = (2 * np.pi * (np.arange(par + 1) % par) / par).astype(F)
        want += OS.restate_segments(np.full(par + 1, k * float(F(30 * deg)), F), lon, 5 * deg, 0)
    check_fields(seg, want)
    # the chord of a parallel leaves it by (arc^2 / 8) sin cos at most: the header's figure at 1 degree
    one = irt.graticule(45 * deg, 90 * deg, 1 * deg)
    p45 = one[np.abs(np.arcsin(one["a"][:, 2]) - 45 * deg) < 1e-6]
    p45 = p45[np.abs(np.arcsin(p45["b"][:, 2]) - 45 * deg) < 1e-6]
    mid = p45["a"].astype(np.float64) + p45["b"]
    lat_mid = np.arcsin(mid[:, 2] / np.linalg.norm(mid, axis=1))
    assert p45.size >= 360 and 1.8e-5 < (lat_mid - 45 * deg).max() < 1.95e-5


def test_axis_convention_a_graticule_node_is_covered():
    """(lat, lon) = (30N, 60E) through irt_latlon_points, normalised, lies on the graticule."""
    deg = OS.RAD
    lat, lon = np.array([30 * deg, -60 * deg], F), np.array([60 * deg, 150 * deg, 270 * deg], F)
    p = irt.latlon_points(lat, lon, np.array([6.371e6], F)).reshape(-1, 3).astype(np.float64)
    u = (p / np.linalg.norm(p, axis=1, keepdims=True)).astype(F)
    got = irt.overlay_cover(OS.segments("graticule"), [((1, 1, 1, 1), 1e-4)], u)
    assert (got >= 0).all()
    off = irt.latlon_points(lat + F(1 * deg), lon + F(1 * deg), np.array([1.0], F)).reshape(-1, 3)
    assert (irt.overlay_cover(OS.segments("graticule"), [((1, 1, 1, 1), 1e-4)], off) == -1).all()


# ------------------------------------------------------------------ cover against the true distance
def judge(seg, pts, got):
    """Per point: must (some segment nearer than W (1 - BAND)), may (some segment nearer than
    W (1 + BAND)); the answer's own distance, and the lowest index that must cover."""
    w = OS.widths_of(seg)
    must = np.zeros(len(pts), bool)
    may = np.zeros(len(pts), bool)
    lowest_must = np.full(len(pts), -1)
    own_ok = np.ones(len(pts), bool)
    nearest = np.full(len(pts), -1)
    for lo in range(0, len(pts), 512):
        d = OS.arc_distance(seg, pts[lo:lo + 512])
        m = d < w * (1 - BAND)
        must[lo:lo + 512] = m.any(1)
        may[lo:lo + 512] = (d < w * (1 + BAND)).any(1)
        lowest_must[lo:lo + 512] = np.where(m.any(1), m.argmax(1), -1)
        nearest[lo:lo + 512] = d.argmin(1)
        g = got[lo:lo + 512]
        rows = np.flatnonzero(g >= 0)
        own_ok[lo + rows] = d[rows, g[rows]] < w[g[rows]] * (1 + BAND)
    return must, may, lowest_must, own_ok, nearest


@pytest.mark.parametrize("name", OS.SET_NAMES)
def test_cover_agrees_with_the_true_angular_distance(name):
    seg, pts, got = OS.segments(name), OS.judged_points(name), OS.scan(name)
    assert got.shape == (len(pts),) and got.min() >= -1 and got.max() < max(seg.size, 1)
    if seg.size == 0:
        assert (got == -1).all()
        return
    must, may, lowest_must, own_ok, _ = judge(seg, pts, got)
    undecided = may & ~must
    print(f"{name}: {len(pts)} points, {int(must.sum())} inside, {int(undecided.sum())} undecided")
    assert undecided.mean() <= 0.02
    assert (got[must] >= 0).all() and (got[~may] == -1).all() and own_ok.all()
    # lowest index wins: no lower segment surely covers the point
    sure = must & (got >= 0)
    assert (got[sure] <= lowest_must[sure]).all()


# ------------------------------------------------------------------ bins against the scan
@pytest.mark.parametrize("N", [1, 4, 64, 256])
def test_bins_equal_the_scan(N):
    for name in OS.SET_NAMES:
        seg = OS.segments(name)
        pts = np.concatenate([OS.judged_points(name), OS.border_points(N)])
        start, lists = irt.overlay_bins(seg, OS.MAX_W, N) if seg.size else (np.zeros(6 * N * N + 1, np.uint32), None)
        assert start.size == 6 * N * N + 1 and start[0] == 0 and (np.diff(start.astype(np.int64)) >= 0).all()
        if lists is not None:
            assert start[-1] == lists.size and lists.max() < seg.size
            inner = np.ones(lists.size, bool)
            inner[start[1:-1][start[1:-1] < lists.size]] = False
            assert (np.diff(lists.astype(np.int64))[inner[1:]] > 0).all(), "a bin's list must ascend"
        want = np.concatenate([OS.scan(name), irt.overlay_cover(seg, OS.STYLES, OS.border_points(N))])
        got = irt.overlay_cover(seg, OS.STYLES, pts, (start, lists), N)
        assert np.array_equal(got, want), (name, N, int((got != want).sum()))


# ------------------------------------------------------------------ the census
def test_census_of_the_inputs():
    """On the frames' pixels alone (the points the device sees), by the helper and the true distances."""
    hit_styles, multi, lowest_not_nearest, body_only, cap_only = set(), {}, {}, 0, 0
    for name in OS.SET_NAMES:
        seg = OS.segments(name)
        if seg.size == 0:
            continue
        pts = OS.frame_subset(name)
        got = OS.scan(name)[:len(pts)]
        hit_styles |= set(seg["style"][got[got >= 0]].tolist())
        if name != "coast":
            must, _, _, _, nearest = judge(seg, pts, got)
            w = OS.widths_of(seg)
            multi[name] = 0
            for lo in range(0, len(pts), 512):
                d = OS.arc_distance(seg, pts[lo:lo + 512])
                multi[name] += int(((d < w * (1 - BAND)).sum(1) >= 2).sum())
            lowest_not_nearest[name] = int(((got >= 0) & must & (got != nearest)).sum())
        # which test of the definition makes the hit: restated in float32 for the answer's segment
        rows = np.flatnonzero(got >= 0)[:4000]
        s, u = seg[got[rows]], pts[rows]
        dot = lambda x, y: (x[:, 0] * y[:, 0] + x[:, 1] * y[:, 1]) + x[:, 2] * y[:, 2]  # noqa: E731
        sin_w = np.sin(OS.widths_of(s)).astype(F)
        chord2 = ((2 * np.sin(0.5 * OS.widths_of(s))) ** 2).astype(F)
        body = (np.abs(dot(u, s["n"])) <= sin_w) & (np.abs(dot(u, s["t"])) <= s["sinHalf"]) & \
            (dot(u, s["a"]) + dot(u, s["b"]) > 0)
        cap = (dot(u - s["a"], u - s["a"]) <= chord2) | (dot(u - s["b"], u - s["b"]) <= chord2)
        assert (body | cap).all()
        body_only += int((body & ~cap).sum())
        cap_only += int((cap & ~body).sum())
        # the antipode of an arc's midpoint is on its great circle and between its tangent cuts, yet the
        # arc alone does not cover it
        anti = -(seg["a"].astype(np.float64) + seg["b"])[:20]
        anti = (anti / np.linalg.norm(anti, axis=1, keepdims=True)).astype(F)
        for i in range(len(anti)):
            assert irt.overlay_cover(seg[i:i + 1], OS.STYLES, anti[i:i + 1])[0] == -1, (name, i)
            assert irt.overlay_cover(seg[i:i + 1], OS.STYLES, -anti[i:i + 1])[0] == 0, (name, i)
    print(f"census on frame pixels: under two lines {multi}, lowest-not-nearest {lowest_not_nearest}, "
          f"{body_only} body-only, {cap_only} cap-only hits")
    assert hit_styles == {0, 1}
    assert body_only > 0 and cap_only > 0
    # the set built for it shows it to the device, in two views
    assert multi["overlap"] >= 10 and lowest_not_nearest["overlap"] >= 5
    for view in ("inside", "outside"):
        u = OS.frame_points(view, "square")
        s = irt.overlay_cover(OS.segments("overlap"), OS.STYLES, u[1][u[0]])
        assert (s >= 0).sum() >= 50 and len(set(OS.segments("overlap")["style"][s[s >= 0]])) == 2, view
    # the arcs across the cube-map corner and edge: both are hit, from bins of every face that meets there
    seg = OS.segments("cube-corner")
    live, u = OS.frame_points("inside", "square")
    s = irt.overlay_cover(seg, OS.STYLES, u[live])
    assert (s == 0).sum() >= 40 and (s == 1).sum() >= 8
    faces = lambda p: set((np.argmax(np.abs(p), axis=1) * 2 + (p[np.arange(len(p)), np.argmax(np.abs(p), axis=1)] < 0)).tolist())  # noqa: E731
    assert len(faces(u[live][s == 0])) == 3 and len(faces(u[live][s == 1])) == 2


def test_census_bins_and_frames():
    seg = OS.segments("coast")
    assert 4900 <= seg.size <= 5100 and np.arcsin(seg["sinHalf"]).max() * 2 < OS.W_THIN
    start4, _ = irt.overlay_bins(seg, OS.MAX_W, 4)
    start64, _ = irt.overlay_bins(seg, OS.MAX_W, 64)
    assert np.diff(start4.astype(np.int64)).max() > 64
    assert (np.diff(start4.astype(np.int64)) == 0).any() and (np.diff(start64.astype(np.int64)) == 0).any()
    # frames: the beside view has hit and missed pixels, the inside view takes the far hit
    live, _ = OS.frame_points("beside", "square")
    assert 0 < live.sum() < live.size
    assert OS.frame_points("inside", "square")[0].all() and OS.frame_points("outside", "square")[0].any()
    # every set shows in some frame, and leaves some pixel free
    for name in OS.SET_NAMES[1:]:
        n = len(OS.frame_subset(name))
        got = OS.scan(name)[:n]
        assert 0 < (got >= 0).sum() < n, name


# ------------------------------------------------------------------ refusals
def test_refusals_write_nothing():
    L = irt.lib()
    deg = OS.RAD
    lat, lon = np.array([0, 10], F) * F(deg), np.array([0, 20], F) * F(deg)
    first = np.array([0, 2], np.int32)
    out = np.zeros(64, irt.SEGMENT_DTYPE)
    out["style"] = 77
    n = C.c_size_t(12345)
    p = lambda a: C.c_void_p(a.ctypes.data) if a is not None else None  # noqa: E731

    def refused(rc, word):
        assert rc == irt.E_INVALID and word in L.irt_last_error().decode(), L.irt_last_error()

    def segs(lat=lat, lon=lon, first=first, lines=1, arc=0.1, style=0, out=out, cap=64):
        return L.irt_overlay_segments(p(lat), p(lon), p(first), lines, arc, style, p(out), cap, C.byref(n))

    for arc in (0.0, -1.0, 0.21, np.nan, np.inf):
        refused(segs(arc=arc), "maxArc")
    for style in (-1, 8):
        refused(segs(style=style), "style")
    refused(segs(lat=None), "null lat or lon")
    refused(segs(first=None), "null first")
    refused(segs(lines=-1), "lines")
    refused(segs(first=np.array([2, 0], np.int32)), "ascend")
    for bad in (np.nan, np.inf, -np.inf):
        refused(segs(lat=np.array([0, bad], F)), "not finite")
        refused(segs(lon=np.array([bad, 0], F)), "not finite")
    # (as floats +-pi/2 lie past the poles: with lon 0 and pi these two are antipodal to 4e-15)
    refused(segs(lat=np.array([np.pi / 2, -np.pi / 2], F), lon=np.array([0.0, np.pi], F)), "antipodal")
    refused(segs(arc=0.01, cap=3), "capacity")
    assert n.value == int(np.ceil(np.arccos(np.dot(*OS.unit_latlon(lat, lon))) / float(F(0.01))))  # the count needed
    assert (out["style"] == 77).all()
    for args in ((0.0, 0.5, 0.1), (0.5, 0.0, 0.1), (4.0, 0.5, 0.1), (0.5, 7.0, 0.1), (0.5, 0.5, 0.0), (0.5, 0.5, 0.3),
                 (np.nan, 0.5, 0.1)):
        rc = L.irt_graticule(*[float(a) for a in args], 0, p(out), 64, C.byref(n))
        assert rc == irt.E_INVALID
    refused(L.irt_graticule(0.5, 0.5, 0.1, 9, p(out), 64, C.byref(n)), "style")
    refused(L.irt_graticule(0.5, 0.5, 0.1, 0, p(out), 64, C.byref(n)), "capacity")
    assert (out["style"] == 77).all()

    seg = np.array(OS.segments("single"), copy=True)
    start, lists = np.full(6 * 16 + 1, 77, np.uint32), np.full(4096, 77, np.uint32)

    def bins(seg=seg, n_=None, w=0.03, N=4, start=start, lists=lists, cap=4096):
        return L.irt_overlay_bins(p(seg), seg.size if n_ is None else n_, w, N, p(start), p(lists), cap, C.byref(n))

    for w in (0.0, -0.01, 0.051, np.nan):
        refused(bins(w=w), "maxHalfWidth")
    for N in (0, -1, 257):
        refused(bins(N=N), "binsPerEdge")
    refused(bins(seg=None, n_=3), "null segments")
    refused(bins(n_=1 << 24), "2^24")
    refused(bins(start=None), "null count or binStart")
    refused(bins(cap=1), "capacity")
    bad = seg.copy()
    bad["style"][0] = 8
    refused(bins(seg=bad), "style 8")
    bad = seg.copy()
    bad["a"][0, 1] = np.nan
    refused(bins(seg=bad), "not finite")
    assert (start == 77).all() and (lists == 77).all()
    assert bins() == 0 and start[0] == 0 and start[-1] == n.value > 0

    st, ns = irt.overlay_styles(OS.STYLES)
    u = np.array(seg["a"][:1], F)
    got = np.full(1, 77, np.int32)

    def cover(seg=seg, n_=None, st=st, ns=ns, start=None, lists=None, N=0, u=u, m=1, got=got):
        return L.irt_overlay_cover(p(seg), seg.size if n_ is None else n_, st, ns, p(start), p(lists), N, p(u), m,
                                   p(got))

    refused(cover(ns=0), "styles are outside")
    refused(cover(ns=9), "styles are outside")
    refused(cover(st=None), "null styles")
    for w in (0.0, 0.06, -1.0, np.nan):
        refused(cover(st=irt.overlay_styles([((1, 1, 1, 1), w)])[0], ns=1), "halfWidth")
    refused(cover(st=irt.overlay_styles([((1, np.inf, 1, 1), 0.01)])[0], ns=1), "rgba")
    two = np.concatenate([seg, seg])
    two["style"][1] = 1
    refused(cover(seg=two, ns=1), "style 1 is outside the table of 1")
    refused(cover(seg=None, n_=2), "null segments")
    refused(cover(n_=1 << 24), "2^24")
    refused(cover(u=None), "null u or segment")
    refused(cover(got=None), "null u or segment")
    refused(cover(start=start, lists=lists, N=0), "binsPerEdge")
    assert got[0] == 77
    assert cover() == 0 and got[0] == 0 and cover(m=0, u=None, got=None) == 0 and cover(seg=None, n_=0) == 0
    assert got[0] == -1
    assert C.sizeof(irt.OverlayStyle) == 20 and irt.SEGMENT_DTYPE.itemsize == 64 and irt.OVERLAY_OVER == 1


def test_overlay_width_spans_the_pixels_asked_for():
    lp = OS.launch_params("outside", "square")
    R = OS.surface_radius()
    w = irt.overlay_width(lp, 64, R, 3.0)
    assert 0 < w <= irt.OVERLAY_MAX_HALF_WIDTH
    # the frame's centre column near the sub-camera point: a meridian of that half-width through it covers
    # about 3 pixels of the centre row
    live, u = OS.frame_points("outside", "square")
    seg = irt.overlay_segments(np.array([60, 90, 60], F) * F(OS.RAD), np.array([90, 90, 270], F) * F(OS.RAD), None, 0.1)
    row = irt.overlay_cover(seg, [((1, 1, 1, 1), w)], u[32])
    assert 2 <= (row >= 0).sum() <= 4
    assert irt.overlay_width(lp, 64, R, 1e6) == float(F(irt.OVERLAY_MAX_HALF_WIDTH))
    assert irt.overlay_width(lp, 64, R, 1.5) == pytest.approx(w / 2)
    for bad in ((0, R, 3.0), (64, 0.0, 3.0), (64, R, 0.0), (64, np.nan, 3.0), (64, R, np.inf)):
        with pytest.raises(irt.IrtError):
            irt.overlay_width(lp, *bad)


# ------------------------------------------------------------------ sanitizers
def test_overlay_helpers_under_the_sanitizers(tmp_path):
    """host/irt_overlay.cpp and tests/overlay_main.cpp as one program of their own, built with
    -fsanitize=address,undefined and run here (no code loaded into python is involved)."""
    cxx = shutil.which(os.environ.get("CXX", "g++"))
    assert cxx, "no C++ compiler"
    repo = os.path.dirname(os.path.abspath(irt.PKG_DIR))
    exe = str(tmp_path / "overlay_main")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-static-libasan", "-static-libubsan",
           "-ffp-contract=off", "-I" + os.path.join(repo, "include"), "-I" + os.path.join(irt.PKG_DIR, "csrc"),
           os.path.join(irt.PKG_DIR, "host", "irt_overlay.cpp"),
           os.path.join(os.path.dirname(os.path.abspath(__file__)), "overlay_main.cpp"), "-o", exe]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "overlay_main: ok" in run.stdout
