"""Census of tests/accel_scenes.py on the CPU (numpy and the oracle only): the scenes do hold what
tests/test_gpu_accel_edges.py relies on, so that no GPU comparison there passes vacuously."""
import functools

import numpy as np
import pytest

import accel_scenes as A
import irt
import oracle as O


@functools.lru_cache(maxsize=None)
def oracle(name, treated=True):
    """The oracle's scene (bounds, shell) of scene `name`; treated=False: of the untreated heights."""
    return O.OracleScene(A.scene(name) if treated else A.heights(False))


def sb_of(S):
    return (S.sb.lower.y, S.sb.upper.y, S.sb.lower.z, S.sb.upper.z)


def test_mixed_rects_reaches_every_shell_path():
    cells = A.mixed_rects()
    n = cells.size
    assert n == 10240
    S = oracle("mixed_rects")
    # the untouched columns keep the bounds of the whole globe and shell
    assert sb_of(S) == A.lat_lon_bounds(irt.synth_grid(2, 3, 62))
    est = A.rect_macrocells(cells, sb_of(S))
    print("macrocells per record: <=16: %d, 17..60: %d, 61..199: %d, >=200: %d" % (
        (est <= 16).sum(), ((est >= 17) & (est <= 60)).sum(), ((est >= 61) & (est <= 199)).sum(), (est >= 200).sum()))
    assert (est <= 16).sum() >= 1000
    assert ((est >= 17) & (est <= 60)).sum() >= 1000
    assert (est >= 200).sum() > n // 8 + 4096  # the wide list overflows: "this lane does it"
    assert not ((est >= 61) & (est <= 199)).any()
    # the in-lane rectangles of 17..60 macrocells span several rows and columns
    ylo, yhi, zlo, zhi = A.rect_extent(cells["lat"], cells["lon"], sb_of(S))
    mid = (est >= 17) & (est <= 60)
    assert ((yhi > ylo) & (zhi > zlo))[mid].all()
    # all records of a column on the same corners
    assert np.array_equal(cells["lat"][0::2], cells["lat"][1::2]) and np.array_equal(cells["lon"][0::2], cells["lon"][1::2])
    # the antimeridian seam (rectangles nearly a row wide) and both poles
    lon, lat = cells["lon"].astype(np.float64), cells["lat"].astype(np.float64)
    assert ((lon.max(1) - lon.min(1)) > np.pi).sum() >= 16
    assert (lat.max(1) > np.pi / 2 - 1e-6).any() and (lat.min(1) < -np.pi / 2 + 1e-6).any()
    assert (zhi - zlo + 1 > 0.9 * A.SHELL).sum() >= 16


def test_heights_holds_every_treatment():
    cells, label = A.heights(), A.heights_labels()
    counts = np.bincount(label, minlength=len(A.TREATMENTS))
    print(dict(zip(A.TREATMENTS, counts.tolist())))
    assert (counts >= 10).all()
    nl = cells["numLayers"]
    for k in (0, 1, 2, 31):
        assert (nl[label == A.TREATMENTS.index(f"layers_{k}")] == k).all()
    h = cells["height"]
    assert np.isfinite(h).all() and np.isfinite(cells["lat"]).all() and np.isfinite(cells["lon"]).all()
    up = np.array([(np.diff(h[i, :nl[i] + 1]) >= 0).all() for i in range(cells.size)])
    for t in ("repeat_start", "repeat_middle", "repeat_end", "all_equal"):
        m = label == A.TREATMENTS.index(t)
        assert up[m].all(), t
        assert all((np.diff(h[i, :nl[i] + 1]) == 0).sum() >= 2 for i in np.flatnonzero(m)), t
    for t in ("unsorted_once", "reversed", "h0_above_top"):
        assert not up[label == A.TREATMENTS.index(t)].any(), t
    m = label == A.TREATMENTS.index("h0_above_top")
    assert (h[m, 0] > h[m, 31]).all()
    # distinct values per slot, unused slots included
    assert np.unique(cells["value"]).size == cells.size * 32 and cells["value"].min() == 100


def test_heights_treatments_change_the_oracle_shell():
    S, U = oracle("heights"), oracle("heights", treated=False)
    assert (S.sb.lower.x, S.sb.upper.x) == (U.sb.lower.x, U.sb.upper.x)  # the radial bounds stay
    assert sb_of(S) == sb_of(U)
    assert not np.array_equal(S.value_ranges, U.value_ranges)
    # value[31] (slot numLayers of a full record) reaches the shell through the unsorted heights
    v31 = A.heights()["value"][:, 31]
    assert np.isin(S.value_ranges[:, 1], v31).any() and not np.isin(U.value_ranges[:, 1], v31).any()


def test_nonfinite_values_reach_the_oracle_ranges():
    cells = A.nonfinite_values()
    placed = A.nonfinite_placed()
    assert (np.bincount(placed[placed >= 0], minlength=len(A.SPECIALS) * len(A.PLACES)) == 6).all()
    assert np.isfinite(cells["value"][:4]).all() and np.isfinite(cells["height"]).all()
    S = oracle("nonfinite_values")
    vr = S.value_ranges
    assert not np.isnan(vr).any()
    assert (vr[:, 0] == -np.inf).any() and (vr[:, 1] == np.inf).any()
    assert np.isneginf(S.data_range[0]) and np.isposinf(S.data_range[1])
    # a macrocell that only all-NaN records cover keeps initGrid's empty range
    hole, (y, z) = A.nonfinite_hole()
    ylo, yhi, zlo, zhi = A.rect_extent(cells["lat"], cells["lon"], sb_of(S))
    cover = (ylo <= y) & (y <= yhi) & (zlo <= z) & (z <= zhi) & (cells["numLayers"] > 0)
    assert cover.any() and hole[cover].all() and np.isnan(cells["value"][cover]).all()
    assert tuple(vr[z * A.SHELL + y]) == (A.FLT_MAX, -A.FLT_MAX)
    empty = (vr[:, 0] == A.FLT_MAX) & (vr[:, 1] == -A.FLT_MAX)
    print("empty macrocells:", int(empty.sum()), "records in the hole:", int(hole.sum()))
    # the grid's oracle takes them as well
    g = S.build_grid()
    assert not np.isnan(g).any() and (g[:, 0] == -np.inf).any() and (g[:, 1] == np.inf).any()


def test_tails_are_slices_with_sound_bounds():
    assert [n % 4 for n in A.TAIL_SIZES].count(0) == 1
    for n in A.TAIL_SIZES:
        cells = A.tails(n)
        assert cells.size == n and cells.tobytes() == A.heights()[:n].tobytes()
        lo, hi = cells["height"][:, 0].min(), cells["height"][np.arange(n), cells["numLayers"]].max()
        sb = A.lat_lon_bounds(cells)
        assert hi > lo and sb[1] > sb[0] and sb[3] > sb[2]
        if n == 1:  # one record covers its own bounds: the whole shell
            vr = O.OracleScene(cells).value_ranges
            assert (vr[:, 1] >= vr[:, 0]).all()


@pytest.mark.parametrize("name", sorted(A.SCENES))
def test_builders_are_deterministic(name):
    first = A.scene(name).tobytes()
    for f in (A._mixed_rects, A._heights, A._nonfinite):
        f.cache_clear()
    assert A.scene(name).tobytes() == first
    assert not A.scene(name).flags.writeable


def test_range_value_sets_decide_the_fold():
    """The host fold (irt_compute_volume_info) over each set: min/max of the used slots without the
    NaNs, and a zero bound carries the sign of the last used zero in record order."""
    cells = A.range_scene()
    used = np.arange(32)[None, :] < cells["numLayers"][:, None]
    seen = set()
    for name, vals in A.range_value_sets().items():
        c = np.array(cells, copy=True)
        c["value"] = vals
        dr = irt.volume_info(c).dataRange
        u = vals[used]  # record order, slot order
        lo = np.float32(np.inf) if np.isnan(u).all() else np.nanmin(u)
        hi = np.float32(-np.inf) if np.isnan(u).all() else np.nanmax(u)
        assert (dr.lower, dr.upper) == (lo, hi), name
        zeros = u[u == 0]
        for b in (dr.lower, dr.upper):
            if b == 0:
                assert zeros.size >= 1 and np.signbit(b) == np.signbit(zeros[-1]), name
                seen.add((name.split("_")[0], bool(np.signbit(b))))
        if "unused" in name:
            assert (vals[~used] == 0).any()
        if name == "zero_in_unused_slots_only":
            assert zeros.size == 0 and dr.lower >= 1
    assert seen == {("min", False), ("min", True), ("max", False), ("max", True), ("zero", False), ("zero", True),
                    ("unused", False)}
    v = A.range_value_sets()["nan_wave"]
    assert np.isnan(v[64:128]).all() and not np.isnan(v[:64]).any() and not np.isnan(v[128:]).any()


def test_edge_lut_alphas_are_distinct():
    for size in (1, 2, 7, 300, 1024):
        lut = A.edge_lut(size)
        assert lut.shape == (size, 4) and np.isfinite(lut).all()
        assert np.unique(lut[:, 3]).size == size and lut[:, 3].min() > 0 and lut[:, 3].max() < 1
