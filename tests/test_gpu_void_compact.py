"""Chained launches that dispatch no workgroups for their void packets' later frames: the flat
kernel's launch with void packets runs F grid rows of Lp live and Vr void work items
(irt.void_lists) instead of the plain grid.

test_gpu_void.py's comparison (one render_accumulate of F frames against F single renders: accum and
fb byte for byte over the seeded prior with -0, a subnormal, +inf and NaN in void pixels, the event
counts against the singles' sums, chain health), and the dispatched-workgroup query.

A launch takes the list only where its rows are shorter than the plain grid's: every launch that does
is asserted to dispatch strictly fewer workgroups.  At 64x64 FRAMING the rows would be longer (72
against 64: see test_void_list_cpu.py), so that launch keeps the bitmap on the plain grid, with the
plain grid's count and the same frames.

The terrain kernels keep the bitmap on the plain grid at every size (their list form needs 8 B of
scratch, which the resource gate rules out), so they run the parent's path, which test_gpu_void.py
covers at every size, F and first accumID; here two of its cases are repeated only to pin their
workgroup count to the plain grid's.
"""
import numpy as np
import pytest

import irt
import test_gpu_void as TV
from helpers import FRAMING
from test_void_list_cpu import _all_void_camera

pytestmark = pytest.mark.gpu


def _expect_wg(lp, info, W, H, F, **kw):
    live, rows = irt.void_lists(lp, info, W, H, F, **kw)
    return F * live.size + F * rows.shape[1]


@pytest.mark.parametrize("first", [0, 5])
@pytest.mark.parametrize("F", [2, 3, 8])
@pytest.mark.parametrize("W,H", [(64, 64), (67, 33), (203, 71)])
def test_compact_launch_equals_single_frames(W, H, F, first):
    ctx = TV._ctx()
    lp = irt.setup_frame(TV._cells(), W, H, camera=FRAMING).lp
    mask, n = TV._void_mask(lp, ctx.info, W, H)
    assert n > 0 and (~mask).any()
    TV._compare(ctx, lp, W, H, F, first, *TV._prior(W, H, mask), n)
    got, plain = ctx.last_workgroups(), irt.num_tiles(W, H) * 64 * F
    if (W, H) == (64, 64):  # rows of 64 + 8 items: the bitmap on the plain grid
        assert _expect_wg(lp, ctx.info, W, H, F) == 72 * F and got == plain
    else:
        assert got == _expect_wg(lp, ctx.info, W, H, F) < plain


def test_more_frames_than_void_packets():
    """F = 33, not a power of two, and more frames than void packets: at 64x64 (8 void packets, the
    bitmap on the plain grid) and at 67x33 (11 void packets: a list whose rows 2 .. 32 have void parts
    that are all padding)."""
    F = 33
    ctx = TV._ctx()
    for W, H in ((64, 64), (67, 33)):
        lp = irt.setup_frame(TV._cells(), W, H, camera=FRAMING).lp
        mask, n = TV._void_mask(lp, ctx.info, W, H)
        assert 0 < n < F
        TV._compare(ctx, lp, W, H, F, 0, *TV._prior(W, H, mask), n)
        plain = irt.num_tiles(W, H) * 64 * F
        if (W, H) == (64, 64):
            assert ctx.last_workgroups() == plain
        else:
            assert ctx.last_workgroups() == _expect_wg(lp, ctx.info, W, H, F) < plain


@pytest.mark.parametrize("F,first", [(2, 5), (8, 0)])
def test_terrain_kernel_keeps_the_plain_grid(F, first):
    W, H = 203, 71
    ctx = TV._ctx(4000.0)
    assert irt.default_kernel_id(ctx) & 262144 == 0, "not the miss-mode kernel"
    lp = irt.setup_frame(TV._cells(4000.0), W, H, camera=FRAMING).lp
    mask, n = TV._void_mask(lp, ctx.info, W, H)
    assert n > 0
    TV._compare(ctx, lp, W, H, F, first, *TV._prior(W, H, mask), n)
    assert ctx.last_workgroups() == irt.num_tiles(W, H) * 64 * F


def test_workgroup_query_of_other_launches():
    """The plain grid's count for a request's first launch, a single frame and a slot-table context."""
    W, H, F = 203, 71, 3
    cells = TV._cells()
    plain = irt.num_tiles(W, H) * 64
    for slots in (False, True):
        mp = pytest.MonkeyPatch()
        if slots:
            mp.setenv("IRT_SLOTS", "1")
        try:
            ctx = irt.Context(cells, 0)
        finally:
            mp.undo()
        lut, vr = irt.default_transfunc((ctx.info.dataRange.lower, ctx.info.dataRange.upper))
        ctx.set_transfunc(lut, vr)
        lp = irt.setup_frame(cells, W, H, camera=FRAMING).lp
        fb, acc = TV._upload(np.zeros((H, W, 4), np.float32), np.zeros((H, W), np.uint32))
        ctx.render_accumulate(lp, W, H, F, fb.data_ptr(), acc.data_ptr())
        assert ctx.void_use() == 0 and ctx.last_workgroups() == plain * F, "first launch"
        ctx.render_accumulate(lp, W, H, F, fb.data_ptr(), acc.data_ptr())
        if slots:
            assert ctx.void_use() == 0 and ctx.last_workgroups() == plain * F
        else:
            assert ctx.void_use() > 0 and ctx.last_workgroups() == _expect_wg(lp, ctx.info, W, H, F) < plain * F
        ctx.render(lp, W, H, fb.data_ptr(), acc.data_ptr())
        assert ctx.last_workgroups() in (plain, plain + ctx.sched_split()[0])
        assert ctx.chain_errors() == 0
        ctx.close()


def test_two_consecutive_compact_launches():
    """accumID continuing: the second launch reads what the first's void waves stored, in whichever
    row carried them, against 2F single frames."""
    W, H, F = 203, 71, 3
    ctx = TV._ctx()
    lp = irt.setup_frame(TV._cells(), W, H, camera=FRAMING).lp
    mask, n = TV._void_mask(lp, ctx.info, W, H)
    accum0, fb0 = TV._prior(W, H, mask)
    fb, acc = TV._upload(accum0, fb0)
    for aid in range(2 * F):
        lp.accumID = aid
        ctx.render(lp, W, H, fb.data_ptr(), acc.data_ptr())
    ref = TV._host(fb, acc)
    lp.accumID = 0
    fb, acc = TV._upload(accum0, fb0)
    ctx.render_accumulate(lp, W, H, F, fb.data_ptr(), acc.data_ptr())  # (the request's first, or not)
    fb, acc = TV._upload(accum0, fb0)
    for k in range(2):
        lp.accumID = k * F
        ctx.render_accumulate(lp, W, H, F, fb.data_ptr(), acc.data_ptr())
        assert ctx.void_use() == n and ctx.last_workgroups() == _expect_wg(lp, ctx.info, W, H, F)
    got = TV._host(fb, acc)
    assert np.array_equal(got[1], ref[1]) and np.array_equal(got[0], ref[0])
    assert ctx.chain_errors() == 0


def _packed_prior(lp, info, W, H, nt, **sel):
    """A random packed prior (ragged_scenes' words) with -0, a subnormal, +inf and NaN in the first
    pixel of void packets."""
    accum, fb = TV.RS.prior(64, 64 * nt, 5)
    accum, fb = accum.copy().reshape(nt, 64, 64, 4), fb.copy().reshape(nt, 64, 64)
    specials = np.array([-0.0, 1e-41, np.inf, np.nan], np.float32)
    void = np.nonzero(irt.void_packets(lp, info, W, H, **sel))[0]
    assert len(void) >= 4
    for j, p in enumerate(void):
        blk, wave = p >> 2, p & 3
        k, sub = blk >> 4, blk & 15
        accum[k, ((sub >> 2) << 4) + ((wave >> 1) << 3), ((sub & 3) << 4) + ((wave & 1) << 3), j % 4] = specials[(j // 4) % 4]
    return accum, fb


@pytest.mark.parametrize("F,first", [(3, 0), (8, 5)])
@pytest.mark.parametrize("form", ["list", "strided"])
def test_tile_list_and_strided_tiles(form, F, first):
    """The packed outputs and event counts of a chained launch over a tile list, and over strided
    tiles, against F single-frame launches of the same request, over the seeded prior."""
    W, H = 203, 71
    ctx = TV._ctx()
    lp = irt.setup_frame(TV._cells(), W, H, camera=FRAMING).lp
    tiles = np.array([7, 0, 5, 2, 3], np.int32) if form == "list" else np.arange(1, 8, 2, dtype=np.int32)
    sel = dict(tiles=tiles) if form == "list" else dict(tile_begin=1, tile_stride=2)

    def launch(frames, fb, acc):
        if form == "list":
            ctx.render_tile_list(lp, W, H, tiles, frames, fb.data_ptr(), acc.data_ptr())
        else:
            ctx.render_tiles_accumulate(lp, W, H, 1, 2, frames, fb.data_ptr(), acc.data_ptr())

    accum0, fb0 = _packed_prior(lp, ctx.info, W, H, len(tiles), **sel)
    fb, acc = TV._upload(accum0, fb0)
    sums = np.zeros(5, np.int64)
    for aid in range(first, first + F):
        lp.accumID = aid
        launch(1, fb, acc)
        assert ctx.void_use() == 0
        sums += TV._counts(ctx.stats())
    ref = TV._host(fb, acc)
    lp.accumID = first
    for frames in (2, F):  # (the request's first launch, if it is, has no list yet)
        fb, acc = TV._upload(accum0, fb0)
        launch(frames, fb, acc)
    assert ctx.void_use() == int(irt.void_packets(lp, ctx.info, W, H, **sel).sum()) > 0
    assert ctx.last_workgroups() == _expect_wg(lp, ctx.info, W, H, F, **sel) < len(tiles) * 64 * F
    got = TV._host(fb, acc)
    assert tuple(sums) == TV._counts(ctx.stats()), "event counts"
    assert np.array_equal(got[1], ref[1]), "accum"
    assert np.array_equal(got[0], ref[0]), "fb"
    assert ctx.chain_errors() == 0


def test_all_void_frame():
    """Lp = 0: every packet void, the launch is F rows of void items alone."""
    W = H = 64
    F = 3
    ctx = TV._ctx()
    lp = irt.setup_frame(TV._cells(), W, H, camera=_all_void_camera(W, H)).lp
    mask, n = TV._void_mask(lp, ctx.info, W, H)
    assert n == 64 and mask.all()
    TV._compare(ctx, lp, W, H, F, 0, *TV._prior(W, H, mask), n)
    assert ctx.last_workgroups() == F * 24 < F * 64
