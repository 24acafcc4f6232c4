"""Void packets on the host (host/irt_void.cpp through irt_debug_void_packets): the 8x8 packets a
chained launch of progressive frames renders once, because each of their rays, whatever the jitter,
passes boxTest and misses the shell's outer sphere.

Soundness against a float64 restatement of the rays and against the oracle's frames; coverage against
the float64 restatement with no margin (so an empty bitmap cannot pass); the cameras and modes that
must classify nothing; the cache.  Grids: synth_grid(2, 2, 47), flat and terrain.
"""
import functools

import numpy as np
import pytest

import irt
import oracle as O
from helpers import FRAMING, bits

SENTINEL = 0xDEADBEEF
VIEW_ALL = None


@functools.lru_cache(maxsize=None)
def _cells(terrain=0.0):
    c = irt.synth_grid(2, 2, 47, terrain=terrain)
    c.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def _info(terrain=0.0):
    return irt.volume_info(_cells(terrain))


def _packet_rects(W, H):
    """Per packet of a whole-frame launch (4 * block + wave): x0, y0, x1, y1 of its active pixels
    (x1, y1 one past the last; x1 <= x0: none), as irt_raygen.h pixel_of maps them."""
    tx, ty = (W + 63) // 64, (H + 63) // 64
    p = np.arange(tx * ty * 64)
    blk, wave = p >> 2, p & 3
    k, sub = blk >> 4, blk & 15
    x0 = (k % tx) * 64 + ((sub & 3) << 4) + ((wave & 1) << 3)
    y0 = (k // tx) * 64 + ((sub >> 2) << 4) + ((wave >> 1) << 3)
    return x0, y0, np.minimum(x0 + 8, W), np.minimum(y0 + 8, H)


JITTERS = np.unique(np.concatenate([np.linspace(0.0, 1.0, 9)[:-1], [float(np.nextafter(np.float32(1), np.float32(0)))]]))


def _rays64(lp, xs, ys, ju, jv):
    """float64 restatement of generateRay for pixel arrays xs, ys and jitters (ju, jv): unit
    directions (..., 3) with the 1e-5 clamp."""
    c = lp.camera12().astype(np.float64)
    a = (xs + 0.5) + ju
    b = (ys + 0.5) + jv
    d = c[3:6] + a[..., None] * c[6:9] + b[..., None] * c[9:12]
    d = d / np.linalg.norm(d, axis=-1, keepdims=True)
    return np.where(np.abs(d) < 1e-5, 1e-5, d)


def _miss_and_in_box(lp, info, xs, ys, ju, jv):
    """(closest approach of each ray's line to the centre, whether the ray passes through the box)
    in float64."""
    org = lp.camera12().astype(np.float64)[0:3]
    d = _rays64(lp, xs, ys, ju, jv)
    dn = d / np.linalg.norm(d, axis=-1, keepdims=True)
    t = -(dn @ org)
    closest = np.linalg.norm(org + t[..., None] * dn, axis=-1)
    lo = np.array(info.bounds.lower.tolist()) - org
    hi = np.array(info.bounds.upper.tolist()) - org
    with np.errstate(divide="ignore", invalid="ignore"):
        l, h = lo / d, hi / d
    t0 = np.maximum(0.0, np.minimum(l, h).max(-1))
    t1 = np.maximum(l, h).min(-1)
    return closest, t0 < t1


def _f64_void(lp, info, W, H):
    """The float64 restatement with no margin: packets all of whose sampled rays (JITTERS^2 per
    active pixel) miss the outer sphere and hit the box."""
    x0, y0, x1, y1 = _packet_rects(W, H)
    R = info.sphericalBounds.upper.x
    out = np.zeros(len(x0), bool)
    ju, jv = np.meshgrid(JITTERS, JITTERS)
    # the rays that can come closest or leave the box are those of the packet's corner pixels
    for p in np.nonzero((x0 < W) & (y0 < H))[0]:
        xs = np.array([x0[p], x1[p] - 1], np.float64)
        ys = np.array([y0[p], y1[p] - 1], np.float64)
        X, Y = np.meshgrid(xs, ys)
        closest, inbox = _miss_and_in_box(lp, info, X[..., None, None], Y[..., None, None], ju, jv)
        out[p] = bool((closest > R).all() and inbox.all())
    return out


SIZES = ((64, 64), (203, 71), (1024, 1024))


@pytest.mark.parametrize("terrain", [0.0, 4000.0])
@pytest.mark.parametrize("W,H", [(64, 64), (67, 33), (203, 71)])
def test_flagged_packets_miss_in_float64(W, H, terrain):
    """Every ray of every flagged packet, over a dense set of jitters with 0 and the largest float
    below 1, passes outside the outer radius and through the box; unflagged packets without active
    pixels only."""
    lp, info = irt.setup_frame(_cells(terrain), W, H, camera=FRAMING).lp, _info(terrain)
    void = irt.void_packets(lp, info, W, H)
    x0, y0, x1, y1 = _packet_rects(W, H)
    assert void.any() and not void[(x0 >= W) | (y0 >= H)].any()
    ju, jv = np.meshgrid(JITTERS, JITTERS)
    R = info.sphericalBounds.upper.x
    for p in np.nonzero(void)[0]:
        X, Y = np.meshgrid(np.arange(x0[p], x1[p], dtype=np.float64), np.arange(y0[p], y1[p], dtype=np.float64))
        closest, inbox = _miss_and_in_box(lp, info, X[..., None, None], Y[..., None, None], ju, jv)
        assert closest.min() > R and inbox.all(), p


@pytest.mark.parametrize("terrain", [0.0, 4000.0])
@pytest.mark.parametrize("W,H", [(64, 64), (203, 71)])
def test_flagged_packets_are_zero_in_the_oracle(W, H, terrain):
    """The oracle's frames for three accumIDs over a sentinel: at every pixel of a flagged packet the
    box test passes (the pixel is written), nothing is sampled (colour and alpha zero: accum stays
    +0 from +0) and the launch's sampleVolume calls all belong to other packets."""
    cells = _cells(terrain)
    lp, info = irt.setup_frame(cells, W, H, camera=FRAMING).lp, _info(terrain)
    void = irt.void_packets(lp, info, W, H)
    x0, y0, x1, y1 = _packet_rects(W, H)
    mask = np.zeros((H, W), bool)
    for p in np.nonzero(void)[0]:
        mask[y0[p]:y1[p], x0[p]:x1[p]] = True
    S = O.OracleScene(cells)
    lut, vr = S.default_lut()
    S.set_transfunc(lut, vr)
    cam = S.camera(W, H, FRAMING)
    for aid in (0, 1, 7):
        fb = np.full((H, W), SENTINEL, np.uint32)
        accum = np.zeros((H, W, 4), np.float32)
        _, fb, st = S.render(S.params(cam, accum_id=aid), W, H, accum=accum, fb=fb)
        assert np.all(fb[mask] == 0), "a void pixel was not written, or not with the zero colour"
        assert np.all(bits(accum)[mask] == 0)
        # the same frame restricted to the other pixels samples as often: no sampleVolume call in a void packet
        ys, xs = np.nonzero(~mask)
        if len(ys):
            calls = 0
            for y in np.unique(ys):
                row = xs[ys == y]
                _, _, s2 = S.render(S.params(cam, accum_id=aid), W, H, rect=(int(row.min()), int(y), int(row.max()) + 1, int(y) + 1))
                calls += s2.locate_calls
            # rows' bounding spans may include void pixels; they add no calls if the claim holds
            assert calls == st.locate_calls


@pytest.mark.parametrize("W,H", SIZES)
def test_coverage(W, H):
    """At least 90 % of the packets the float64 restatement (no margin) finds wholly outside."""
    lp, info = irt.setup_frame(_cells(), W, H, camera=FRAMING).lp, _info()
    void = irt.void_packets(lp, info, W, H)
    ref = _f64_void(lp, info, W, H)
    print(f"void packets {W}x{H}: classifier {int(void.sum())}, float64 no margin {int(ref.sum())}, "
          f"of {len(void)}")
    assert not (void & ~ref).any()
    assert ref.sum() > 0 and void.sum() >= 0.9 * ref.sum()


def test_refusals():
    cells, info = _cells(), _info()
    W, H = 96, 80
    setup = irt.setup_frame(cells, W, H, camera=FRAMING)
    assert irt.void_packets(setup.lp, info, W, H).any()
    for eye in ((0.0, 0.0, 6.0e6), (0.0, 0.0, 1e10)):  # inside the globe; too far for the float bound
        lp = irt.setup_frame(cells, W, H, camera=(eye, (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 60.0)).lp
        assert not irt.void_packets(lp, info, W, H).any(), eye
    for raygen, accel in ((irt.RAYGEN_AE, 0), (irt.RAYGEN_WITH_ACCEL, 1)):
        lp = irt.setup_frame(cells, W, H, camera=FRAMING, raygen=raygen).lp
        lp.accelMode = accel
        assert not irt.void_packets(lp, info, W, H).any(), (raygen, accel)


def test_view_all_box_silhouette():
    """The fovy-90 view-all camera: a packet holding a pixel that misses the box in some frame is
    never flagged (the oracle's box test over a sentinel, frames 0..7)."""
    W, H = 96, 80
    cells, info = _cells(), _info()
    lp = irt.setup_frame(cells, W, H, camera=VIEW_ALL).lp
    void = irt.void_packets(lp, info, W, H)
    S = O.OracleScene(cells)
    lut, vr = S.default_lut()
    S.set_transfunc(lut, vr)
    cam = S.camera(W, H, VIEW_ALL)
    missed = np.zeros((H, W), bool)
    for aid in range(8):
        fb = np.full((H, W), SENTINEL, np.uint32)
        _, fb, _ = S.render(S.params(cam, accum_id=aid), W, H, fb=fb)
        missed |= fb == SENTINEL
    assert missed.any()
    x0, y0, x1, y1 = _packet_rects(W, H)
    for p in np.nonzero(void)[0]:
        assert not missed[y0[p]:y1[p], x0[p]:x1[p]].any(), p
    print(f"view-all {W}x{H}: {int(void.sum())} void packets of {len(void)}")


def test_cache():
    """The same request computes nothing; changing any one key field computes anew."""
    W, H = 203, 71
    info = irt.VolumeInfo.from_buffer_copy(_info())
    lp = irt.LaunchParams.from_buffer_copy(irt.setup_frame(_cells(), W, H, camera=FRAMING).lp)
    vc = irt.VoidCache()
    first = vc.packets(lp, info, W, H)
    assert vc.computations == 1
    lp.accumID = 17  # not part of the key: a progressive sequence computes once
    assert np.array_equal(vc.packets(lp, info, W, H), first) and vc.computations == 1
    n = 1

    def changed(**kw):
        nonlocal n
        vc.packets(lp, info, **{"w": W, "h": H, **kw})
        n += 1
        assert vc.computations == n, kw

    for field in ("org", "dir_00", "dir_du", "dir_dv"):
        for axis in "xyz":
            v = getattr(lp, field)
            setattr(v, axis, float(np.nextafter(np.float32(getattr(v, axis)), np.float32(np.inf))))
            changed()
    changed(w=W + 1)
    changed(h=H + 1)
    changed()  # back to W x H
    changed(tiles=[0, 1, 2])
    changed(tiles=[0, 2, 1])
    assert np.array_equal(vc.packets(lp, info, W, H, tiles=np.array([0, 2, 1])), vc.packets(lp, info, W, H, tiles=[0, 2, 1]))
    assert vc.computations == n
    changed(tile_begin=1)
    changed(tile_begin=1, tile_stride=2)
    for corner in (info.bounds.lower, info.bounds.upper):
        for axis in "xyz":
            setattr(corner, axis, getattr(corner, axis) + 1000.0)
            changed(tile_begin=1, tile_stride=2)
    info.sphericalBounds.upper.x += 1000.0
    changed(tile_begin=1, tile_stride=2)
    info.sphericalBounds.lower.x -= 1000.0
    changed(tile_begin=1, tile_stride=2)
    lp.raygen = irt.RAYGEN_AE
    changed(tile_begin=1, tile_stride=2)
    lp.accelMode = 1
    changed(tile_begin=1, tile_stride=2)
    lp.mode = irt.MODE_CUBQL
    changed(tile_begin=1, tile_stride=2)


def test_tile_forms_follow_pixel_of():
    """A tile list and a strided launch flag the packets the whole frame flags, at their own index."""
    W, H = 203, 71
    lp, info = irt.setup_frame(_cells(), W, H, camera=FRAMING).lp, _info()
    whole = irt.void_packets(lp, info, W, H).reshape(-1, 64)
    tiles = [5, 0, 7, 2]
    assert np.array_equal(irt.void_packets(lp, info, W, H, tiles=tiles).reshape(-1, 64), whole[tiles])
    assert np.array_equal(irt.void_packets(lp, info, W, H, tile_begin=1, tile_stride=3).reshape(-1, 64), whole[1::3])
