"""The plan of real launches (irt_debug_last_plan): the kernel and grid each kind of launch ran,
against literal expectations, and the dispatched-workgroup query against the same grid.

Every case is a 128 x 128 frame (4 tiles, 64 blocks, 256 packets) of the R2B02 x 47 grid, FRAMING.
Kernel ids (k_render<id>; irt_kernels.h OPT_*): FLAT the hole-free form of the default, TERRAIN its
form for scenes with holes, | 8 work items, | 128 slot table, | 16 void bitmap, | 16 | 64 void
work-item list; GRID_ID and WEDGE_ID the grid accelerator's and the samplers' kernels.  The last
three cases also compare the frame with single-frame launches of the same request, bit for bit.
"""
import numpy as np
import pytest

import irt
import test_gpu_void as TV
from helpers import FRAMING
from test_gpu_void_compact import _expect_wg

pytestmark = pytest.mark.gpu

W = H = 128
F = 3
FLAT, TERRAIN = 73663776, 1147143456
GRID_ID, WEDGE_ID = 67118112, 67125280
ENV = ("IRT_SCHED", "IRT_SLOTS", "IRT_CHAIN", "IRT_QUEUE", "IRT_RENDER_VARIANT", "IRT_SPLIT_FACTOR", "IRT_SPLIT_LG",
       "IRT_PROBE_EXIT", "IRT_COUNTERS")


def _context(terrain=0.0, **env):
    """A context of its own (its void cache and schedule start empty), created under `env` alone."""
    mp = pytest.MonkeyPatch()
    for k in ENV:
        mp.delenv(k, raising=False)
    for k, v in env.items():
        mp.setenv(k, v)
    try:
        ctx = irt.Context(TV._cells(terrain), 0)
    finally:
        mp.undo()
    lut, vr = irt.default_transfunc((ctx.info.dataRange.lower, ctx.info.dataRange.upper))
    ctx.set_transfunc(lut, vr)
    return ctx


def _lp(terrain=0.0):
    return irt.setup_frame(TV._cells(terrain), W, H, camera=FRAMING).lp


def _buffers(pixels=W * H):
    return TV._upload(np.zeros((pixels, 4), np.float32), np.zeros(pixels, np.uint32))


def _check(ctx, want):
    plan = ctx.last_plan()
    assert plan == want
    assert ctx.last_workgroups() == plan[2] * plan[3]


def test_single_frame():
    ctx = _context()
    fb, acc = _buffers()
    ctx.render(_lp(), W, H, fb.data_ptr(), acc.data_ptr())
    _check(ctx, (FLAT, 64, 256, 1, 64))
    ctx.close()


@pytest.mark.parametrize("terrain", [0.0, 4000.0])
def test_chained_frames_first_and_second_launch(terrain):
    """A request's first launch: the plain grid, F rows.  The same request again: the flat kernel runs
    the rows of work items, the terrain kernel the bitmap on the plain grid."""
    ctx = _context(terrain)
    lp = _lp(terrain)
    kid = TERRAIN if terrain else FLAT
    fb, acc = _buffers()
    ctx.render_accumulate(lp, W, H, F, fb.data_ptr(), acc.data_ptr())
    assert ctx.void_use() == 0
    _check(ctx, (kid, 64, 256, F, 64))
    ctx.render_accumulate(lp, W, H, F, fb.data_ptr(), acc.data_ptr())
    assert ctx.void_use() > 0
    if terrain:
        _check(ctx, (kid | 16, 64, 256, F, 64))
    else:
        rows = _expect_wg(lp, ctx.info, W, H, F) // F  # voidLive + voidRow
        assert rows < 256
        _check(ctx, (kid | 16 | 64, 64, rows, F, 64))
    assert ctx.chain_errors() == 0
    ctx.close()


def test_slot_table():
    ctx = _context(IRT_SLOTS="1")
    fb, acc = _buffers()
    ctx.render(_lp(), W, H, fb.data_ptr(), acc.data_ptr())
    _check(ctx, (FLAT | 128, 64, 256, 1, 64))
    ctx.close()


def test_work_items():
    """Single frames in measured-cost order until one splits packets: the work items come first."""
    import torch
    ctx = _context(IRT_SCHED="1", IRT_SPLIT_FACTOR="1e-6")
    lp = _lp()
    fb, acc = _buffers()
    for aid in range(64):
        lp.accumID = aid
        ctx.render(lp, W, H, fb.data_ptr(), acc.data_ptr())
        torch.cuda.synchronize()
        if ctx.sched_split()[0] > 0:
            break
    ns = ctx.sched_split()[0]
    assert ns > 0 and ns % 8 == 0
    _check(ctx, (FLAT | 8, 64, 256 + ns, 1, 64))
    ctx.close()


def test_unchained_frames():
    ctx = _context(IRT_CHAIN="0")
    fb, acc = _buffers()
    ctx.render_accumulate(_lp(), W, H, F, fb.data_ptr(), acc.data_ptr())
    _check(ctx, (FLAT, 64, 256, F, 64))
    ctx.close()


def _against_single_frames(ctx, launch, pixels, want):
    """launch(frames, fb, acc) of F frames: its plan, and its frame against F single-frame launches."""
    fb, acc = _buffers(pixels)
    lp = launch.lp
    for aid in range(F):
        lp.accumID = aid
        launch(1, fb, acc)
        _check(ctx, want[:3] + (1,) + want[4:])
    ref = TV._host(fb, acc)
    assert ref[0].any(), "an empty frame"
    lp.accumID = 0
    fb, acc = _buffers(pixels)
    launch(F, fb, acc)
    _check(ctx, want)
    got = TV._host(fb, acc)
    assert np.array_equal(got[1], ref[1]), "accum"
    assert np.array_equal(got[0], ref[0]), "fb"
    assert ctx.chain_errors() == 0


def test_tile_list():
    ctx = _context()
    tiles = np.array([2, 1], np.int32)

    def launch(frames, fb, acc):
        ctx.render_tile_list(launch.lp, W, H, tiles, frames, fb.data_ptr(), acc.data_ptr())

    launch.lp = _lp()
    _against_single_frames(ctx, launch, 2 * 4096, (FLAT, 64, 128, F, 32))
    ctx.close()


@pytest.mark.parametrize("mode,accel,kid", [(irt.MODE_USER_GEOM, 1, GRID_ID), (irt.MODE_CUBQL, 0, WEDGE_ID)])
def test_grid_accelerator_and_sampler(mode, accel, kid):
    ctx = _context()
    if mode != irt.MODE_USER_GEOM:
        ctx.build_wedge_accel(TV._cells())

    def launch(frames, fb, acc):
        ctx.render_accumulate(launch.lp, W, H, frames, fb.data_ptr(), acc.data_ptr())

    launch.lp = _lp()
    launch.lp.mode, launch.lp.accelMode = mode, accel
    _against_single_frames(ctx, launch, W * H, (kid, 256, 64, F, 64))
    ctx.close()
