"""Void packets on the device: a chained launch of progressive frames renders the packets that miss
the globe in every frame once (frame 0's wave applies every frame's lerp of the zero colour; the
later frames' waves return at once).

fb and accum after one irt_render_accumulate launch against F single irt_render launches, byte for
byte, over prior buffer contents with -0, a subnormal, +inf and NaN in void pixels; the launch's
event counts against the singles' sums; the use query; chain health.
"""
import functools

import numpy as np
import pytest

import irt
import ragged_scenes as RS
from helpers import FRAMING, bits

pytestmark = pytest.mark.gpu

VIEW_ALL = None


@functools.lru_cache(maxsize=None)
def _cells(terrain=0.0):
    c = irt.synth_grid(2, 2, 47, terrain=terrain)
    c.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def _ctx(terrain=0.0):
    ctx = irt.Context(_cells(terrain), 0)
    lut, vr = irt.default_transfunc((ctx.info.dataRange.lower, ctx.info.dataRange.upper))
    ctx.set_transfunc(lut, vr)
    return ctx


def _void_mask(lp, info, W, H):
    """(H, W) bool: the pixels of the whole frame's void packets."""
    void = irt.void_packets(lp, info, W, H)
    tx = (W + 63) // 64
    mask = np.zeros((H, W), bool)
    for p in np.nonzero(void)[0]:
        blk, wave = p >> 2, p & 3
        k, sub = blk >> 4, blk & 15
        x0 = (k % tx) * 64 + ((sub & 3) << 4) + ((wave & 1) << 3)
        y0 = (k // tx) * 64 + ((sub >> 2) << 4) + ((wave >> 1) << 3)
        mask[y0:y0 + 8, x0:x0 + 8] = True
    return mask, int(void.sum())


def _prior(W, H, mask):
    """ragged_scenes' random prior (random words, -0, a subnormal, +inf, NaN), with the four specials
    also put into void pixels."""
    accum, fb = RS.prior(W, H, 5)
    accum = accum.copy()
    ys, xs = np.nonzero(mask)
    specials = np.array([-0.0, 1e-41, np.inf, np.nan], np.float32)
    for j in range(min(len(ys), 64)):
        accum[ys[j * (len(ys) // 64 or 1) % len(ys)], xs[j * (len(ys) // 64 or 1) % len(ys)], j % 4] = specials[(j // 4) % 4]
    return accum, fb


def _upload(accum, fb):
    import torch
    a = torch.from_numpy(np.ascontiguousarray(accum).reshape(-1)).cuda()
    f = torch.from_numpy(np.ascontiguousarray(fb).view(np.int32).reshape(-1)).cuda()
    return f, a


def _host(fb, acc):
    import torch
    torch.cuda.synchronize()
    return fb.cpu().numpy().view(np.uint32).copy(), bits(acc.cpu().numpy())


def _counts(st):
    return (st.raysLaunched, st.raysInBox, st.locateCalls, st.samplesFound, st.candidatesTested)


def _compare(ctx, lp, W, H, F, first, accum0, fb0, expect_void):
    fb, acc = _upload(accum0, fb0)
    sums = np.zeros(5, np.int64)
    for aid in range(first, first + F):
        lp.accumID = aid
        ctx.render(lp, W, H, fb.data_ptr(), acc.data_ptr())
        assert ctx.void_use() == 0, "a single frame took the void path"
        sums += _counts(ctx.stats())
    ref = _host(fb, acc)
    # the bitmap is computed when a request comes a second time: a launch of the same camera and
    # frame first (it may be the first of this request, or not: other cases share the context)
    fb, acc = _upload(accum0, fb0)
    ctx.render_accumulate(lp, W, H, 2, fb.data_ptr(), acc.data_ptr())
    assert ctx.void_use() in (0, expect_void)
    fb, acc = _upload(accum0, fb0)
    lp.accumID = first
    ctx.render_accumulate(lp, W, H, F, fb.data_ptr(), acc.data_ptr())
    assert ctx.void_use() == expect_void
    got = _host(fb, acc)
    assert tuple(sums) == _counts(ctx.stats()), "event counts"
    assert np.array_equal(got[1], ref[1]), "accum"
    assert np.array_equal(got[0], ref[0]), "fb"
    assert ctx.chain_errors() == 0


@pytest.mark.parametrize("first", [0, 5])
@pytest.mark.parametrize("F", [2, 3, 8])
@pytest.mark.parametrize("W,H", [(64, 64), (67, 33), (203, 71)])
def test_chained_launch_equals_single_frames(W, H, F, first):
    """The flat (hole-free) kernel, FRAMING."""
    ctx = _ctx()
    lp = irt.setup_frame(_cells(), W, H, camera=FRAMING).lp
    mask, n = _void_mask(lp, ctx.info, W, H)
    assert n > 0
    accum0, fb0 = _prior(W, H, mask)
    assert all(np.any(bits(accum0)[mask] == b) for b in bits(np.array([-0.0, 1e-41, np.inf], np.float32)))
    assert np.isnan(accum0[mask]).any()
    _compare(ctx, lp, W, H, F, first, accum0, fb0, n)


@pytest.mark.parametrize("F,first", [(2, 5), (8, 0)])
def test_terrain_kernel(F, first):
    W, H = 203, 71
    ctx = _ctx(4000.0)
    assert irt.default_kernel_id(ctx) & 262144 == 0, "not the miss-mode kernel"
    lp = irt.setup_frame(_cells(4000.0), W, H, camera=FRAMING).lp
    mask, n = _void_mask(lp, ctx.info, W, H)
    assert n > 0
    _compare(ctx, lp, W, H, F, first, *_prior(W, H, mask), n)


@pytest.mark.parametrize("F,first", [(3, 0), (8, 5)])
def test_view_all_camera(F, first):
    """Camera::viewAll, fovy 90: the box's silhouette crosses the frame; whatever is flagged there
    (possibly nothing) must leave the frames what they were."""
    W, H = 203, 71
    ctx = _ctx()
    lp = irt.setup_frame(_cells(), W, H, camera=VIEW_ALL).lp
    mask, n = _void_mask(lp, ctx.info, W, H)
    _compare(ctx, lp, W, H, F, first, *_prior(W, H, mask if n else np.ones((H, W), bool)), n)


@pytest.mark.parametrize("F,first", [(3, 0), (8, 5)])
def test_packed_tile_list(F, first):
    """irt_render_tile_list, chained: the listed tiles' packed fb and accum against the frame of F
    single launches, over a sentinel prior."""
    W, H = 203, 71  # 4 x 2 tiles, right column and bottom row cut
    ctx = _ctx()
    lp = irt.setup_frame(_cells(), W, H, camera=FRAMING).lp
    tiles = np.array([7, 0, 5, 2, 3], np.int32)
    n = int(irt.void_packets(lp, ctx.info, W, H, tiles=tiles).sum())
    assert n > 0
    accum0, fb0 = RS.prior(W, H, RS.TILE)
    fb, acc = _upload(accum0, fb0)
    for aid in range(first, first + F):
        lp.accumID = aid
        ctx.render(lp, W, H, fb.data_ptr(), acc.data_ptr())
    rfb, racc = _host(fb, acc)
    rfb, racc = rfb.reshape(H, W), racc.reshape(H, W, 4)
    import torch
    pa = torch.full((len(tiles) * 4096 * 4,), -7.25, dtype=torch.float32, device="cuda")
    pf = torch.full((len(tiles) * 4096,), int(np.uint32(0xDEADBEEF).view(np.int32)), dtype=torch.int32, device="cuda")
    lp.accumID = first
    scratch = torch.zeros(len(tiles) * 4096 * 5, dtype=torch.float32, device="cuda")
    ctx.render_tile_list(lp, W, H, tiles, 2, scratch.data_ptr(), scratch[len(tiles) * 4096:].data_ptr())
    ctx.render_tile_list(lp, W, H, tiles, F, pf.data_ptr(), pa.data_ptr())
    assert ctx.void_use() == n
    gfb, gacc = _host(pf, pa)
    gfb, gacc = gfb.reshape(len(tiles), 64, 64), gacc.reshape(len(tiles), 64, 64, 4)
    for k, tid in enumerate(tiles):
        x0, y0 = (tid % 4) * 64, (tid // 4) * 64
        h, w = min(64, H - y0), min(64, W - x0)
        assert np.array_equal(gacc[k, :h, :w], racc[y0:y0 + h, x0:x0 + w]), ("accum", tid)
        assert np.array_equal(gfb[k, :h, :w], rfb[y0:y0 + h, x0:x0 + w]), ("fb", tid)
        outside = np.ones((64, 64), bool)
        outside[:h, :w] = False
        assert np.all(gfb[k][outside] == 0xDEADBEEF), "a pixel outside the frame was written"
    assert ctx.chain_errors() == 0


def test_use_query():
    """> 0 for FRAMING's chained launch; 0 for a sequence of views, a single frame, a one-frame
    accumulate and a context with the chain hook set."""
    W, H = 96, 80
    cells = _cells()
    ctx = irt.Context(cells, 0)
    lut, vr = irt.default_transfunc((ctx.info.dataRange.lower, ctx.info.dataRange.upper))
    ctx.set_transfunc(lut, vr)
    lp = irt.setup_frame(cells, W, H, camera=FRAMING).lp
    zero = lambda: _upload(np.zeros((H, W, 4), np.float32), np.zeros((H, W), np.uint32))  # noqa: E731
    fb, acc = zero()
    ctx.render_accumulate(lp, W, H, 4, fb.data_ptr(), acc.data_ptr())
    assert ctx.void_use() == 0, "a request's first launch computed the bitmap"
    fb, acc = zero()
    ctx.render_accumulate(lp, W, H, 4, fb.data_ptr(), acc.data_ptr())
    n = ctx.void_use()
    assert n > 0 and n == int(irt.void_packets(lp, ctx.info, W, H).sum())
    ctx.render(lp, W, H, fb.data_ptr(), acc.data_ptr())
    assert ctx.void_use() == 0
    ctx.render_accumulate(lp, W, H, 1, fb.data_ptr(), acc.data_ptr())
    assert ctx.void_use() == 0
    lps = [irt.LaunchParams.from_buffer_copy(lp) for _ in range(3)]
    ctx.render_sequence(lps, W, H, fb.data_ptr(), acc.data_ptr())
    assert ctx.void_use() == 0
    ctx.render_accumulate(lp, W, H, 4, fb.data_ptr(), acc.data_ptr())
    assert ctx.void_use() == n
    ref = _host(fb, acc)
    # the chain hook set (no frame withheld here: a huge frame index), frames unchanged
    ctx.set_chain_fault(0, 1 << 20)
    fb2, acc2 = zero()
    ctx.render_accumulate(lp, W, H, 4, fb2.data_ptr(), acc2.data_ptr())
    assert ctx.void_use() == 0
    ctx.render(lp, W, H, fb2.data_ptr(), acc2.data_ptr())
    ctx.render_accumulate(lp, W, H, 1, fb2.data_ptr(), acc2.data_ptr())
    ctx.render_sequence(lps, W, H, fb2.data_ptr(), acc2.data_ptr())
    ctx.render_accumulate(lp, W, H, 4, fb2.data_ptr(), acc2.data_ptr())
    got = _host(fb2, acc2)
    assert np.array_equal(got[1], ref[1]) and np.array_equal(got[0], ref[0])
    assert ctx.chain_errors() == 0
    ctx.close()


def test_a_new_camera_waits_for_its_second_launch():
    """Every new camera's first chained launch runs without a bitmap (nothing is computed for a
    camera that gets one launch); its second takes the path; going back to an earlier camera is a
    new request again."""
    W, H = 96, 80
    cells = _cells()
    ctx = irt.Context(cells, 0)
    lut, vr = irt.default_transfunc((ctx.info.dataRange.lower, ctx.info.dataRange.upper))
    ctx.set_transfunc(lut, vr)
    fb, acc = _upload(np.zeros((H, W, 4), np.float32), np.zeros((H, W), np.uint32))
    near = ((0.0, 0.0, 1.2e7), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 60.0)
    for cam in (FRAMING, near, FRAMING):
        lp = irt.setup_frame(cells, W, H, camera=cam).lp
        n = int(irt.void_packets(lp, ctx.info, W, H).sum())
        assert n > 0
        got = []
        for _ in range(3):
            ctx.render_accumulate(lp, W, H, 3, fb.data_ptr(), acc.data_ptr())
            got.append(ctx.void_use())
        assert got == [0, n, n], (cam, got)
    assert ctx.chain_errors() == 0
    ctx.close()


@pytest.mark.parametrize("F,first", [(3, 0), (8, 5)])
def test_strided_tiles(F, first):
    """irt_render_tiles_accumulate: every second tile from tile 1, packed, against the frame of F
    single launches."""
    import torch
    W, H = 203, 71
    ctx = _ctx()
    lp = irt.setup_frame(_cells(), W, H, camera=FRAMING).lp
    n = int(irt.void_packets(lp, ctx.info, W, H, tile_begin=1, tile_stride=2).sum())
    assert n > 0
    tiles = list(range(1, 8, 2))
    fb, acc = _upload(np.zeros((H, W, 4), np.float32), np.zeros((H, W), np.uint32))
    for aid in range(first, first + F):
        lp.accumID = aid
        ctx.render(lp, W, H, fb.data_ptr(), acc.data_ptr())
    rfb, racc = _host(fb, acc)
    rfb, racc = rfb.reshape(H, W), racc.reshape(H, W, 4)
    lp.accumID = first
    for frames in (2, F):  # (the request's first launch, if it is, computes no bitmap)
        pa = torch.zeros(len(tiles) * 4096 * 4, dtype=torch.float32, device="cuda")
        pf = torch.zeros(len(tiles) * 4096, dtype=torch.int32, device="cuda")
        ctx.render_tiles_accumulate(lp, W, H, 1, 2, frames, pf.data_ptr(), pa.data_ptr())
    assert ctx.void_use() == n
    gfb, gacc = _host(pf, pa)
    gfb, gacc = gfb.reshape(len(tiles), 64, 64), gacc.reshape(len(tiles), 64, 64, 4)
    for k, tid in enumerate(tiles):
        x0, y0 = (tid % 4) * 64, (tid // 4) * 64
        h, w = min(64, H - y0), min(64, W - x0)
        assert np.array_equal(gacc[k, :h, :w], racc[y0:y0 + h, x0:x0 + w]), ("accum", tid)
        assert np.array_equal(gfb[k, :h, :w], rfb[y0:y0 + h, x0:x0 + w]), ("fb", tid)
    assert ctx.chain_errors() == 0


def test_slot_table_context_keeps_its_kernels(monkeypatch):
    """A context whose launches start from the slot table (IRT_SLOTS=1: the OPT_SLOT kernels, which
    have no void-packet form) never takes the path, and its chained launch equals single frames."""
    monkeypatch.setenv("IRT_SLOTS", "1")
    W, H, F = 203, 71, 8
    cells = _cells()
    ctx = irt.Context(cells, 0)
    lut, vr = irt.default_transfunc((ctx.info.dataRange.lower, ctx.info.dataRange.upper))
    ctx.set_transfunc(lut, vr)
    assert irt.default_kernel_id(ctx) & 128, "no slot table"
    lp = irt.setup_frame(cells, W, H, camera=FRAMING).lp
    mask, n = _void_mask(lp, ctx.info, W, H)
    accum0, fb0 = _prior(W, H, mask)
    fb, acc = _upload(accum0, fb0)
    for aid in range(F):
        lp.accumID = aid
        ctx.render(lp, W, H, fb.data_ptr(), acc.data_ptr())
    ref = _host(fb, acc)
    lp.accumID = 0
    for _ in range(2):
        fb, acc = _upload(accum0, fb0)
        ctx.render_accumulate(lp, W, H, F, fb.data_ptr(), acc.data_ptr())
        assert ctx.void_use() == 0
    got = _host(fb, acc)
    assert np.array_equal(got[1], ref[1]) and np.array_equal(got[0], ref[0])
    assert ctx.chain_errors() == 0
    ctx.close()
