"""The work-item lists of a chained launch that dispatches no workgroups for its void packets' later
frames (host/irt_void.cpp through irt_debug_void_lists; no device).

Such a launch of F frames runs F grid rows of Lp live items -- the same in every row -- and Vr void
items.  Here: a packet (4 * block + wave) is LIVE when it has an active pixel and is not void; packets
without an active pixel (past the frame's right or bottom edge) are in neither part, no workgroup is
dispatched for them.  Checked against the bitmap of irt_debug_void_packets for the frames of
ragged_scenes, 64x64, 67x33, 203x71 and a 1024^2 FRAMING request, F in {2, 3, 8, 33}, over whole
frames, a packed tile list and strided tiles.
"""
import functools

import numpy as np
import pytest

import irt
import ragged_scenes as RS
from helpers import FRAMING

EMPTY = 0xFFFFFFFF
FRAMES = (2, 3, 8, 33)


@functools.lru_cache(maxsize=None)
def _cells():
    c = irt.synth_grid(2, 2, 47)
    c.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def _info():
    return irt.volume_info(_cells())


def _tile_ids(W, H, tile_begin, tile_stride, tiles):
    total = irt.num_tiles(W, H)
    return np.asarray(tiles, np.int64) if tiles is not None else np.arange(tile_begin, total, tile_stride)


def _active(W, H, ids):
    """bool per packet of the launch: any pixel inside the frame (irt_raygen.h pixel_of)."""
    tx = (W + 63) // 64
    p = np.arange(len(ids) * 64)
    blk, wave = p >> 2, p & 3
    tid, sub = ids[blk >> 4], blk & 15
    x0 = (tid % tx) * 64 + ((sub & 3) << 4) + ((wave & 1) << 3)
    y0 = (tid // tx) * 64 + ((sub >> 2) << 4) + ((wave >> 1) << 3)
    return (x0 < W) & (y0 < H)


def _check(lp, info, W, H, F, tile_begin=0, tile_stride=1, tiles=None, need_live=True):
    ids = _tile_ids(W, H, tile_begin, tile_stride, tiles)
    void = irt.void_packets(lp, info, W, H, tile_begin, tile_stride, tiles)
    live_set = np.nonzero(_active(W, H, ids) & ~void)[0]
    void_set = np.nonzero(void)[0]
    assert len(void_set) > 0, "precondition: the request has void packets"
    assert len(live_set) > 0 or not need_live, "precondition: the request has live packets"
    lists = irt.void_lists(lp, info, W, H, F, tile_begin, tile_stride, tiles)
    assert lists is not None
    live, rows = lists
    Lp, Vr, V = live.size, rows.shape[1], len(void_set)
    assert rows.shape[0] == F
    assert Lp % 8 == 0 and Vr % 8 == 0 and Vr > 0
    assert Vr == (-(-V // F) + 7) // 8 * 8
    # every live packet exactly once in the live part, every void packet exactly once over the rows
    lv = live[live != EMPTY]
    assert np.array_equal(np.sort(lv), live_set), "live part"
    vv = rows.reshape(-1)
    assert np.array_equal(vv[:V], void_set), "void part: each void packet once, ascending"
    assert np.all(vv[V:] == EMPTY), "void part: padding past the last packet"
    assert not np.intersect1d(lv, vv[:V]).size
    # empty items only as padding: a residue's items, then its padding to the longest residue
    assert Lp == 8 * max((np.bincount((live_set >> 2) & 7, minlength=8).max() if len(live_set) else 0), 0)
    for x in range(8):
        res = live[x::8]
        n = int((res != EMPTY).sum())
        assert np.all(res[:n] != EMPTY) and np.all(res[n:] == EMPTY), ("padding inside residue", x)
        blk = res[:n] >> 2
        assert np.all((blk & 7) == x), "block b's items at indices = b mod 8"
        # a block's items consecutive within its residue (blocks ascending, waves ascending)
        assert np.all(np.diff(res[:n].astype(np.int64)) > 0)
    # the launch's workgroups, from the live and void sets alone: F rows of the longest residue x 8
    # and of the void packets' share of a row, rounded up to 8
    longest = max(int(((live_set >> 2) & 7 == x).sum()) for x in range(8))
    assert F * live.size + rows.size == F * 8 * longest + F * 8 * -(-(-(-V // F)) // 8)
    assert len(lv) + V == int(_active(W, H, ids).sum())
    if F > V:  # more rows than void packets: rows whose void part is all padding
        assert np.all(rows[V:] == EMPTY) and np.all(rows[-1] == EMPTY)
    return Lp, Vr, V


@pytest.mark.parametrize("F", FRAMES)
@pytest.mark.parametrize("W,H", [(64, 64), (67, 33), (203, 71)])
def test_whole_frames(W, H, F):
    """At 64x64 the rows are longer than the plain grid's (72 against 64 workgroups): 56 live and 8 void
    packets, the live part padded to 64 and 8 void items per row -- with both counts multiples of 8 no
    list of such a frame is shorter --, so that launch keeps the bitmap on the plain grid
    (test_gpu_void_compact.py).  The other frames' rows are shorter than the plain grid's."""
    lp = irt.setup_frame(_cells(), W, H, camera=FRAMING).lp
    Lp, Vr, V = _check(lp, _info(), W, H, F)
    if (W, H) == (64, 64):
        assert (Lp, Vr, V) == (64, 8, 8)
    else:
        assert Lp + Vr < 64 * irt.num_tiles(W, H), (Lp, Vr)


@pytest.mark.parametrize("F", FRAMES)
def test_more_frames_than_void_packets(F):
    """64x64 FRAMING has 8 void packets: at F = 33 most rows' void parts are padding."""
    W = H = 64
    lp = irt.setup_frame(_cells(), W, H, camera=FRAMING).lp
    Lp, Vr, V = _check(lp, _info(), W, H, F)
    assert V == 8 and Vr == 8


@pytest.mark.parametrize("F", FRAMES)
def test_ragged_scene_frames(F):
    """Every frame size of ragged_scenes under its framing camera that has void packets."""
    seen = 0
    for size in RS.SIZES:
        s = RS.setup("flat", "framing", size)
        W, H = size
        if not irt.void_packets(s.lp, s.info, W, H).any():
            assert irt.void_lists(s.lp, s.info, W, H, F) is None
            continue
        _check(s.lp, s.info, W, H, F)
        seen += 1
    assert seen >= 3


@pytest.mark.parametrize("F", FRAMES)
def test_framing_1024(F):
    W = H = 1024
    lp = irt.setup_frame(_cells(), W, H, camera=FRAMING).lp
    Lp, Vr, V = _check(lp, _info(), W, H, F)
    assert F * (Lp + Vr) < F * 64 * irt.num_tiles(W, H)


@pytest.mark.parametrize("F", FRAMES)
def test_tile_list_and_strided_tiles(F):
    W, H = 203, 71
    lp = irt.setup_frame(_cells(), W, H, camera=FRAMING).lp
    _check(lp, _info(), W, H, F, tiles=np.array([7, 0, 5, 2, 3], np.int32))
    _check(lp, _info(), W, H, F, tile_begin=1, tile_stride=2)


def test_no_void_packet_no_list():
    """A camera inside the shell classifies nothing: no list, the launch runs the plain grid."""
    W, H = 203, 71
    inside = ((0.0, 0.0, 1.0e6), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 60.0)
    lp = irt.setup_frame(_cells(), W, H, camera=inside).lp
    assert not irt.void_packets(lp, _info(), W, H).any()
    for F in FRAMES:
        assert irt.void_lists(lp, _info(), W, H, F) is None


def _all_void_camera(W, H):
    """FRAMING's eye aimed at a corner of the world box, small fovy: every packet certified void."""
    info = _info()
    b = info.bounds.upper
    return ((0.0, 0.0, 1.4e7), (0.93 * b.x, 0.93 * b.y, 0.0), (0.0, 1.0, 0.0), 2.0)


def test_all_void_frame():
    """Lp = 0: every packet of the frame is void."""
    W = H = 64
    lp = irt.setup_frame(_cells(), W, H, camera=_all_void_camera(W, H)).lp
    void = irt.void_packets(lp, _info(), W, H)
    assert void.all(), int(void.sum())
    for F in FRAMES:
        Lp, Vr, V = _check(lp, _info(), W, H, F, need_live=False)
        assert Lp == 0 and V == 64
