"""Interior packets on the host (host/irt_void.cpp section 4 through irt_debug_interior_packets): the
8x8 packets whose rays k_render sets up without the box test and the range guards.

Soundness: every ray of every flagged packet -- the four jitter corners, 64 seeded jitters and the
LCG's own jitters of accumIDs 0, 1 and 1000 per pixel -- in a float32 restatement of generateRay,
boxTest and intersectSphere, operation for operation as oracle/icon_oracle.cpp evaluates them (and
pinned to oracle_box_test / oracle_intersect_sphere on a sample of the same rays): the box test
passes, both spheres hit, the range selection takes the front-and-back case and recip_ok holds for
len, A and both q.  The cameras and modes that must classify nothing; the coverage at the framing
camera at 1024^2; no packet both interior and void.  Grid: synth_grid(2, 2, 47).
"""
import ctypes as C
import functools

import numpy as np
import pytest

import irt
import oracle as O
from classifier_cameras import WINDOW_EYE, _box32, _lcg_jitters, _packet_rects, _rays32, _recip_ok, _sphere32
from helpers import FRAMING

F = np.float32
ONE_BELOW = float(np.nextafter(F(1), F(0)))
R_EARTH = 6.371229e6


@functools.lru_cache(maxsize=None)
def _cells():
    c = irt.synth_grid(2, 2, 47)
    c.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def _info(filtered=False):
    c = _cells()
    if filtered:  # a lat/lon window of the grid: its box does not contain the sphere
        c = c[(c["lat"].min(1) > 0.2) & (c["lat"].max(1) < 1.0) & (c["lon"].min(1) > -0.5) & (c["lon"].max(1) < 0.6)]
        assert len(c) > 0
    return irt.volume_info(np.ascontiguousarray(c))


def _check_packets(lp, info, W, H, flagged):
    cam = lp.camera12()
    org = cam[0:3]
    lo, hi = np.array(info.bounds.lower.tolist(), F), np.array(info.bounds.upper.tolist(), F)
    rIn, rOut = info.sphericalBounds.lower.x, info.sphericalBounds.upper.x
    x0, y0, x1, y1 = _packet_rects(W, H)
    rng = np.random.default_rng(20240611)
    sj = rng.random((64, 2)).astype(F)
    sj = np.minimum(sj, F(ONE_BELOW))
    corners = np.array([(0, 0), (0, ONE_BELOW), (ONE_BELOW, 0), (ONE_BELOW, ONE_BELOW)], F)
    fixed = np.concatenate([corners, sj])  # (68, 2)
    sample = []
    for p in np.nonzero(flagged)[0]:
        assert x0[p] < W and y0[p] < H, "a packet without active pixels is flagged"
        Y, X = np.mgrid[y0[p]:y1[p], x0[p]:x1[p]]
        jus = [np.broadcast_to(fixed[:, 0], X.shape + (68,))]
        jvs = [np.broadcast_to(fixed[:, 1], X.shape + (68,))]
        for aid in (0, 1, 1000):
            ju, jv = _lcg_jitters(aid, W, H, X, Y)
            jus.append(ju[..., None])
            jvs.append(jv[..., None])
        ju, jv = np.concatenate(jus, -1), np.concatenate(jvs, -1)
        ln, d = _rays32(cam, X[..., None], Y[..., None], ju, jv)
        hit, t0, _ = _box32(org, d, lo, hi)
        assert hit.all(), (p, "boxTest")
        dO, A, qO, st1, st4 = _sphere32(org, d, rOut)
        dI, _, qI, st2, st3 = _sphere32(org, d, rIn)
        assert (dO >= 0).all() and (dI >= 0).all(), (p, "a sphere is missed")
        assert (t0 < st2).all() and not (st4 < t0).any(), (p, "not the front-and-back case")
        assert _recip_ok(ln).all() and _recip_ok(A).all() and _recip_ok(qO).all() and _recip_ok(qI).all(), p
        assert (np.abs(A - F(1)) < 1e-4).all()
        sample.append((d[0, 0, 0], t0[0, 0, 0], st1[0, 0, 0], st4[0, 0, 0], st2[0, 0, 0], st3[0, 0, 0]))
    # the restatement itself, against the oracle's functions on one ray per packet
    L = O.olib()
    box = O.b3(lo.tolist(), hi.tolist())
    for d, t0, st1, st4, st2, st3 in sample[:200]:
        a, b = C.c_float(), C.c_float()
        assert L.oracle_box_test(O.v3(org), O.v3(d), 0.0, 1e10, box, C.byref(a), C.byref(b)) == 1 and F(a.value) == t0
        assert L.oracle_intersect_sphere(O.v3(org), O.v3(d), rOut, C.byref(a), C.byref(b)) == 1
        assert F(a.value) == st1 and F(b.value) == st4
        assert L.oracle_intersect_sphere(O.v3(org), O.v3(d), rIn, C.byref(a), C.byref(b)) == 1
        assert F(a.value) == st2 and F(b.value) == st3


OFF_AXIS = ((1.0e7, 4.0e6, 9.0e6), (3.0e6, 2.0e6, 0.0), (0.0, 1.0, 0.0), 40.0)
CAMERAS = [
    ("framing 64x64", FRAMING, 64, 64, False, True),
    ("framing 96x72", FRAMING, 96, 72, False, True),
    ("eye at 1.05 R", ((0.0, 0.0, 1.05 * R_EARTH), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 60.0), 96, 72, False, True),
    ("eye at 60 R", ((0.0, 0.0, 60 * R_EARTH), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 2.5), 96, 72, False, True),
    ("off axis", OFF_AXIS, 96, 72, False, True),
    ("lat/lon window", WINDOW_EYE, 96, 72, True, True),
]


@pytest.mark.parametrize("name,camera,W,H,filtered,some", CAMERAS, ids=[c[0] for c in CAMERAS])
def test_flagged_packets_are_interior_in_float32(name, camera, W, H, filtered, some):
    info = _info(filtered)
    lp = irt.setup_frame(_cells(), W, H, camera=camera, info=info).lp
    flagged = irt.interior_packets(lp, info, W, H)
    void = irt.void_packets(lp, info, W, H)
    print(f"{name}: {int(flagged.sum())} interior, {int(void.sum())} void of {len(flagged)} packets")
    assert not (flagged & void).any()
    if some:
        assert flagged.any() and not flagged.all()
    _check_packets(lp, info, W, H, flagged)


def test_window_box_does_not_contain_the_sphere():
    """... and the window camera's eye lies beyond box sides that are nearer the centre than the inner
    sphere (x and z): the packets flagged there are certified by the rectangle's own bounds."""
    info = _info(True)
    r = info.sphericalBounds.lower.x
    assert info.bounds.lower.x > -r and info.bounds.lower.z > -r
    eye = WINDOW_EYE[0]
    assert info.bounds.upper.x < r and eye[0] > info.bounds.upper.x
    assert info.bounds.upper.z < r and eye[2] > info.bounds.upper.z


def test_refusals():
    cells, info = _cells(), _info()
    W, H = 96, 80
    setup = irt.setup_frame(cells, W, H, camera=FRAMING)
    assert irt.interior_packets(setup.lp, info, W, H).any()
    inside = 0.5 * (info.sphericalBounds.lower.x + info.sphericalBounds.upper.x)
    for eye in ((0.0, 0.0, inside), (0.0, 0.0, 6.0e6), (0.0, 0.0, 1e10)):
        lp = irt.setup_frame(cells, W, H, camera=(eye, (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 60.0)).lp
        assert not irt.interior_packets(lp, info, W, H).any(), eye
    for raygen, accel in ((irt.RAYGEN_AE, 0), (irt.RAYGEN_WITH_ACCEL, 1)):
        lp = irt.setup_frame(cells, W, H, camera=FRAMING, raygen=raygen).lp
        lp.accelMode = accel
        assert not irt.interior_packets(lp, info, W, H).any(), (raygen, accel)
    for field in ("org", "dir_00", "dir_du", "dir_dv"):
        lp = irt.setup_frame(cells, W, H, camera=FRAMING).lp
        getattr(lp, field).y = float("nan")
        assert not irt.interior_packets(lp, info, W, H).any(), field


def test_coverage_at_the_framing_camera():
    """At least 85 % of the live packets of the 1024^2 framing frame are interior (the geometry gives
    about 91 %: a disc of radius 453 px less the ring the silhouette crosses)."""
    W = H = 1024
    info = _info()
    lp = irt.setup_frame(_cells(), W, H, camera=FRAMING, info=info).lp
    flagged = irt.interior_packets(lp, info, W, H)
    void = irt.void_packets(lp, info, W, H)
    live = int((~void).sum())
    print(f"1024^2 framing: {int(flagged.sum())} interior of {live} live packets ({flagged.sum() / live:.3f})")
    assert not (flagged & void).any()
    assert flagged.sum() >= 0.85 * live


def test_cache_computes_both_bitmaps_once():
    info = _info()
    lp = irt.setup_frame(_cells(), 96, 72, camera=FRAMING, info=info).lp
    cache = irt.VoidCache()
    a = irt.interior_packets(lp, info, 96, 72, cache=cache)
    cache.packets(lp, info, 96, 72)
    b = irt.interior_packets(lp, info, 96, 72, cache=cache)
    assert cache.computations == 1 and np.array_equal(a, b)
    assert np.array_equal(a, irt.interior_packets(lp, info, 96, 72))
