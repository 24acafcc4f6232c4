"""The unstructured samplers (CUBQL_MODE wedges, TRIANGLE_MODE) point by point on the CPU, on the
edge records and points of tests/sampler_scenes.py: the oracle's brute-force scans against the
reference's own wedge sampleVolume (tests/golden/kats_wedge_edges.npz), and the product's host
twins (host/irt_scene.cpp wedge_locate_host, triangle_locate_host) against the oracle.  The device
side of the same comparison is tests/test_gpu_samplers.py.

TRIANGLE_MODE has no reference-made fixture: OptiX's own triangle intersection test is not
reproducible, so the oracle and the product share one definition (irt_common.h ray_triangle) and
its parity with the reference stays unpinned."""
import ctypes as C
import os

import numpy as np
import pytest

import irt
import oracle as O
import sampler_scenes as S

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "kats_wedge_edges.npz")
FIXTURE_SCENES = ("heights", "nonfinite", "convert_icon")


def _host_lib():
    L = irt.lib()
    P = C.c_void_p
    L.irt_debug_scene_build.argtypes = [P, C.c_size_t, C.POINTER(P)]
    L.irt_debug_scene_build_wedges.argtypes = [P, P, C.c_size_t]
    L.irt_debug_scene_locate_wedge.argtypes = [P, irt.Vec3, C.POINTER(C.c_float)]
    L.irt_debug_scene_locate_triangle.argtypes = [P, irt.Vec3, C.POINTER(C.c_float), C.POINTER(C.c_uint32)]
    L.irt_debug_scene_free.argtypes = [P]
    return L


def _host_twins(cells, pts):
    """((found, value) of irt_debug_scene_locate_wedge, of irt_debug_scene_locate_triangle)."""
    L = _host_lib()
    cells = np.ascontiguousarray(cells)
    h = C.c_void_p()
    assert L.irt_debug_scene_build(cells.ctypes.data, cells.size, C.byref(h)) == 0
    assert L.irt_debug_scene_build_wedges(h, cells.ctypes.data, cells.size) == 0
    out = [(np.zeros(len(pts), np.int32), np.zeros(len(pts), np.float32)) for _ in range(2)]
    # the float goes through a c_float array: c_float.value would widen a NaN to a Python float
    v = (C.c_float * 1)()
    vb = np.frombuffer(v, np.float32)
    rec = C.c_uint32(0)
    for k, p in enumerate(pts):
        q = irt.Vec3(*p.tolist())
        hit = L.irt_debug_scene_locate_wedge(h, q, v)
        out[0][0][k] = hit
        out[0][1][k] = vb[0] if hit else 0.0
        hit = L.irt_debug_scene_locate_triangle(h, q, v, C.byref(rec))
        out[1][0][k] = hit
        out[1][1][k] = vb[0] if hit else 0.0
    L.irt_debug_scene_free(h)
    return out


@pytest.mark.parametrize("name", FIXTURE_SCENES)
def test_wedge_oracle_matches_reference_on_edge_records(name):
    """oracle_wedge_sample_points equals the reference's ref_wedge_sample (kats_wedge_edges.npz),
    hit for hit and bit for bit, on unsorted, reversed, repeated and short records, non-finite
    values and the convert_icon layout; the fixture's records and points are those of
    sampler_scenes, so the oracle answers the other tests compare with are the pinned ones."""
    npz = np.load(GOLDEN)
    z = {k: npz[k] for k in npz.files}
    cells = np.ascontiguousarray(z["cells_" + name].T).view(irt.CELL_DTYPE).ravel()
    pts, idx = z["points_" + name], z["index_" + name]
    assert cells.tobytes() == S.scene(name).tobytes()
    ps = S.points(name)
    assert np.array_equal(pts.view(np.uint32), ps.points[idx].view(np.uint32))
    sub = S.PointSet(pts, ps.record[idx], ps.kind[idx])
    want = (z["hit_" + name], z["value_" + name])
    S.assert_same_samples(name, sub, O.wedge_sample_points(cells, pts), want, "wedge oracle vs reference")
    (fw, vw), _ = S.oracle_answers(name)
    S.assert_same_samples(name, sub, (fw[idx], vw[idx]), want, "wedge oracle (whole set) vs reference")
    hits = want[0] != 0
    assert hits.sum() >= 0.15 * len(pts) and (~hits).sum() >= 0.15 * len(pts)
    if name == "nonfinite":
        v = want[1][hits]
        assert np.isnan(v).any() and np.isinf(v).any() and (np.abs(v[np.isfinite(v)]) > 1e38).any()


@pytest.mark.parametrize("name", S.SCENE_NAMES)
def test_host_samplers_match_oracle(name):
    """irt_debug_scene_locate_wedge against oracle_wedge_sample_points and
    irt_debug_scene_locate_triangle against oracle_triangle_sample_points on every scene and
    point of sampler_scenes (sampler_scenes.first_difference: flags equal, values equal as bits,
    NaN equal to NaN); and the point set reaches its recorded share of hits."""
    cells, ps = S.scene(name), S.points(name)
    ow, ot = S.oracle_answers(name)
    hw, ht = _host_twins(cells, ps.points)
    S.assert_same_samples(name, ps, hw, ow, "host wedge locator vs oracle")
    S.assert_same_samples(name, ps, ht, ot, "host triangle locator vs oracle")
    n, nw, nt = S.MEASURED[name]
    assert len(ps.points) == n
    share = (ow[0].mean(), ot[0].mean())
    print(f"{name}: {n} points, wedge found {int(ow[0].sum())} (recorded {nw}), "
          f"triangle found {int(ot[0].sum())} (recorded {nt})")
    for got, rec in zip(share, S.CENSUS[name]):
        assert got >= rec
        assert rec >= S.FLOOR or cells.size == 1


def test_point_sets_cover_the_edges():
    """What the point sets are for: every TREATMENTS label and SPECIALS x PLACES combination has
    structured points, each |p| is the float32 radius asked for, and the sets are read-only."""
    import accel_scenes as A
    for name in S.SCENE_NAMES:
        ps = S.points(name)
        assert not ps.points.flags.writeable and np.isfinite(ps.points).all()
        assert len(ps.points) <= 6000
    st = S.points("heights")
    recs = np.unique(st.record[st.kind == S.STRUCTURED])
    assert set(A.heights_labels()[recs]) == set(range(len(A.TREATMENTS)))
    sn = S.points("nonfinite")
    recs = np.unique(sn.record[sn.kind == S.STRUCTURED])
    assert set(A.nonfinite_placed()[recs]) >= set(range(len(A.SPECIALS) * len(A.PLACES)))
    assert A.nonfinite_hole()[0][recs].any()
    # exactly on height[0] and height[numLayers] of the sampled records (TRIANGLE_MODE's limits)
    cells = S.scene("heights")
    p = st.points[st.kind == S.STRUCTURED].astype(np.float32)
    r = np.sqrt((p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1] + p[:, 2] * p[:, 2]).astype(np.float32))
    rec = st.record[st.kind == S.STRUCTURED]
    h0 = cells["height"][rec, 0]
    hn = cells["height"][rec, cells["numLayers"][rec]]
    assert (r == h0).sum() >= 4 * 20 and (r == hn).sum() >= 4 * 20
    for name in ("convert_icon", "terrain"):
        assert (S.points(name).kind == S.VOID).sum() >= 80  # 40 records x 2 directions at least


def test_batched_oracle_entries_equal_single_point_ones():
    """oracle_*_sample_points against oracle_wedge_sample / oracle_triangle_sample, which the
    earlier tests use, on a sample of two scenes' points."""
    L = O.olib()
    for name in ("nonfinite", "terrain"):
        cells, ps = np.ascontiguousarray(S.scene(name)), S.points(name)
        (fw, vw), (ft, vt) = S.oracle_answers(name)
        pick = np.random.default_rng(1).choice(len(ps.points), 150, replace=False)
        one = [(np.zeros(len(pick), np.int32), np.zeros(len(pick), np.float32)) for _ in range(2)]
        for j, k in enumerate(pick):
            for m, entry in enumerate((L.oracle_wedge_sample, L.oracle_triangle_sample)):
                v = (C.c_float * 1)()
                one[m][0][j] = entry(O._p(cells), cells.size, O.v3(ps.points[k]), v)
                one[m][1][j] = np.frombuffer(v, np.float32)[0] if one[m][0][j] else 0.0
        sub = S.PointSet(ps.points[pick], ps.record[pick], ps.kind[pick])
        S.assert_same_samples(name, sub, (fw[pick], vw[pick]), one[0], "batched vs single wedge oracle")
        S.assert_same_samples(name, sub, (ft[pick], vt[pick]), one[1], "batched vs single triangle oracle")
        assert one[0][0].any() and one[1][0].any()


def test_comparison_helper():
    """first_difference: flags, bits, and NaN equal to NaN whatever its sign and payload."""
    f = np.array([1, 1, 0, 1], np.int32)
    a = np.array([1.0, np.nan, 5.0, -0.0], np.float32)
    b = a.copy()
    b.view(np.uint32)[1] = 0xFFC00001  # another NaN
    b[2] = 7.0  # not found: the value does not count
    assert S.first_difference(f, a, f, b) == -1
    b[3] = 0.0
    assert S.first_difference(f, a, f, b) == 3  # -0 and +0 differ as bits
    g = f.copy()
    g[2] = 1
    assert S.first_difference(f, a, g, a) == 2
    c = a.copy()
    c[1] = np.inf
    assert S.first_difference(f, a, f, c) == 1
