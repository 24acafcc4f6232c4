"""Interior packets on the device: a chained launch that carries void data sets the rays of its
interior packets up without the box test, the d < 0 exits, the range selection and the fallback
divisions (irt_raygen.h; host/irt_void.cpp section 4).

Three irt_render_accumulate launches of 8 frames of one camera (the classification applies from the
second) against a second context that renders the same accumIDs one irt_render per frame, which
never classifies: accum bits, fb bytes and the event counts after every launch; the use query.
synth_grid(2, 2, 10), flat and over terrain, FRAMING (interior, limb and void packets in one frame),
whole frames and a tile list of half the tiles.
"""
import functools

import numpy as np
import pytest

import irt
from helpers import FRAMING, bits

pytestmark = pytest.mark.gpu

F = 8
LAUNCHES = 3


@functools.lru_cache(maxsize=None)
def _cells(terrain=0.0):
    c = irt.synth_grid(2, 2, 10, terrain=terrain)
    c.setflags(write=False)
    return c


def _context(terrain):
    ctx = irt.Context(_cells(terrain), 0)
    lut, vr = irt.default_transfunc((ctx.info.dataRange.lower, ctx.info.dataRange.upper))
    ctx.set_transfunc(lut, vr)
    return ctx


def _buffers(pixels):
    import torch
    return torch.zeros(pixels, dtype=torch.int32).cuda(), torch.zeros(pixels * 4, dtype=torch.float32).cuda()


def _host(fb, acc):
    import torch
    torch.cuda.synchronize()
    return fb.cpu().numpy().view(np.uint32).copy(), bits(acc.cpu().numpy())


def _counts(st):
    return np.array((st.raysLaunched, st.raysInBox, st.locateCalls, st.samplesFound, st.candidatesTested), np.int64)


def _run(terrain, W, H, tiles=None):
    lp = irt.setup_frame(_cells(terrain), W, H, camera=FRAMING).lp
    chained, single = _context(terrain), _context(terrain)
    sel = {} if tiles is None else {"tiles": tiles}
    interior = irt.interior_packets(lp, chained.info, W, H, **sel)
    void = irt.void_packets(lp, chained.info, W, H, **sel)
    assert interior.any() and void.any() and not (interior | void).all(), "interior, limb and void packets"
    pixels = W * H if tiles is None else len(tiles) * 4096

    def launch(ctx, frames, fb, acc):
        if tiles is None:
            if frames == 1:
                ctx.render(lp, W, H, fb.data_ptr(), acc.data_ptr())
            else:
                ctx.render_accumulate(lp, W, H, frames, fb.data_ptr(), acc.data_ptr())
        else:
            ctx.render_tile_list(lp, W, H, tiles, frames, fb.data_ptr(), acc.data_ptr())

    fb_c, acc_c = _buffers(pixels)
    fb_s, acc_s = _buffers(pixels)
    for k in range(LAUNCHES):
        sums = np.zeros(5, np.int64)
        for aid in range(k * F, (k + 1) * F):
            lp.accumID = aid
            launch(single, 1, fb_s, acc_s)
            assert single.interior_use() == 0 and single.void_use() == 0, "a single frame classified"
            sums += _counts(single.stats())
        lp.accumID = k * F
        launch(chained, F, fb_c, acc_c)
        if k == 0:
            assert chained.interior_use() == 0, "classified at the request's first launch"
        else:
            assert chained.void_use() == int(void.sum())
            assert chained.interior_use() == int(interior.sum()) > 0
        got, ref = _host(fb_c, acc_c), _host(fb_s, acc_s)
        assert np.array_equal(_counts(chained.stats()), sums), f"event counts, launch {k}"
        assert np.array_equal(got[1], ref[1]), f"accum, launch {k}"
        assert np.array_equal(got[0], ref[0]), f"fb, launch {k}"
        assert ref[0].any()
    assert chained.chain_errors() == 0
    # a single frame of the classifying context: the parent's kernel, nothing classified
    lp.accumID = LAUNCHES * F
    launch(chained, 1, fb_c, acc_c)
    launch(single, 1, fb_s, acc_s)
    assert chained.interior_use() == 0
    got, ref = _host(fb_c, acc_c), _host(fb_s, acc_s)
    assert np.array_equal(got[1], ref[1]) and np.array_equal(got[0], ref[0])
    chained.close()
    single.close()


@pytest.mark.parametrize("terrain", [0.0, 4000.0])
@pytest.mark.parametrize("W,H", [(96, 72), (64, 64)])
def test_chained_launches_equal_single_frames(W, H, terrain):
    _run(terrain, W, H)


@pytest.mark.parametrize("terrain", [0.0, 4000.0])
def test_tile_list_of_half_the_tiles(terrain):
    _run(terrain, 96, 72, tiles=np.array([3, 0], np.int32))
