"""The launch plan (irt_render.hip plan_render, through irt_debug_plan: no device): which k_render
instantiation and which grid a launch gets, for every compiled variant.

The selection rules are restated here over the OPT_* bits (irt_kernels.h), independently of the
library's table of forms:

  * a sampler other than the user geometry runs the wedge kernel -- the default at 256-thread
    workgroups with full LDS and no waves-per-SIMD floor, | OPT_WEDGE --, over the grid accelerator
    | OPT_GRID; the grid accelerator alone the same base at 4 waves/SIMD | OPT_GRID; each carries the
    variant's OPT_SERIAL over;
  * else, in this order: the persistent queue (| OPT_QUEUE: the A/B library only, and no variant with
    OPT_WAVEWG, OPT_SERIAL, OPT_STATS or OPT_TIMING), the void work-item list (| OPT_VOID | OPT_VLIST:
    the hole-free form of the default only), the void bitmap (| OPT_VOID), the slot table (| OPT_SLOT,
    | OPT_SPLIT with work items), work items alone (| OPT_SPLIT) -- the last three for the default
    and its two scene forms only --, else the variant's own kernel.  Arguments asking for a form the
    variant lacks are passed over: that form's test falls through to the next.

The grid follows from the form: the queue kernel (queueWG, 1) at 256 threads; the list kernel
(voidLive + voidRow, frames); every other 16 blocks per tile x 256 / threads workgroups per block,
behind the work items, by frames.  Flag combinations no real launch has (void with slots, void with
work items, work items with several frames) are planned by the same precedence.
"""
import itertools
import os
import subprocess
import sys

import pytest

import irt

MONO, WAVEWG, LEAN, SERIAL, STATS, TIMING = 4096, 4194304, 2097152, 65536, 32768, 524288
QUEUE, SPLIT, SLOT, VOID, VLIST, WEDGE, GRID = 16777216, 8, 128, 16, 64, 16384, 8192
NOMISS, VOIDLOC = 262144, 1073741824
DEFAULT = 73405728
MAX_SPLIT = 4096  # kMaxSplit
LIVE, ROW, QUEUE_WG = 16, 8, 5
AB = irt.LIB_PATH == irt.ALL_LIB_PATH


def expected(variant, sampler, accel, flags, tiles, frames, num_split):
    """(id, threads, grid x, grid y) by the rules above."""
    k, d = variant & ~MONO, DEFAULT & ~MONO
    base = d & ~(0xF00 | WAVEWG | LEAN)
    family = k in (d, d | NOMISS, d | VOIDLOC)
    if sampler != irt.MODE_USER_GEOM:
        kid = base | WEDGE | (k & SERIAL) | (GRID if accel == 1 else 0)
    elif accel == 1:
        kid = base | 0x400 | GRID | (k & SERIAL)
    elif flags & irt.PLAN_QUEUE and AB and not k & (WAVEWG | SERIAL | STATS | TIMING):
        return k | QUEUE, 256, QUEUE_WG, 1
    elif flags & irt.PLAN_VOID_LIST and k == d | NOMISS:
        return k | VOID | VLIST, 64, LIVE + ROW, frames
    elif flags & irt.PLAN_VOID_BITS and family:
        kid = k | VOID
    elif flags & irt.PLAN_SLOTS and family:
        kid = k | SLOT | (SPLIT if num_split else 0)
    elif num_split and family:
        kid = k | SPLIT
    else:
        kid = k
    threads = 64 if kid & WAVEWG else 256
    return kid, threads, tiles * 16 * (256 // threads) + num_split, frames


def test_plan_rules():
    variants = irt.compiled_variants()
    assert DEFAULT in variants and DEFAULT | NOMISS in variants and DEFAULT | VOIDLOC in variants
    assert (5120 | SERIAL in variants) == AB, "the one-lane-per-ray variant: the A/B library's"
    n = 0
    for v, sampler, accel, flags, tiles, frames, ns in itertools.product(
            variants, (irt.MODE_USER_GEOM, irt.MODE_TRIANGLES, irt.MODE_CUBQL), (0, 1), range(32), (1, 3), (1, 3), (0, 8)):
        got = irt.plan(v, sampler, accel, flags, tiles, frames, ns, LIVE, ROW, QUEUE_WG)
        want = expected(v, sampler, accel, flags, tiles, frames, ns) + (tiles * 16,)
        assert got == want, (v, sampler, accel, flags, tiles, frames, ns)
        n += 1
    assert n == len(variants) * 3 * 2 * 32 * 2 * 2 * 2


def test_forms_each_variant_has():
    """The forms by name, for the variants whose launches use them."""
    d = DEFAULT & ~MONO
    for v in (DEFAULT, DEFAULT | NOMISS, DEFAULT | VOIDLOC):
        k = v & ~MONO
        assert irt.plan(v)[:2] == (k, 64)
        assert irt.plan(v, num_split=8)[:3] == (k | SPLIT, 64, 64 + 8)
        assert irt.plan(v, flags=irt.PLAN_SLOTS)[0] == k | SLOT
        assert irt.plan(v, flags=irt.PLAN_SLOTS, num_split=8)[0] == k | SLOT | SPLIT
        assert irt.plan(v, flags=irt.PLAN_VOID_BITS | irt.PLAN_CHAIN, frames=3)[:4] == (k | VOID, 64, 64, 3)
        # void outranks the slot table and the work items
        assert irt.plan(v, flags=irt.PLAN_VOID_BITS | irt.PLAN_SLOTS, num_split=8)[:3] == (k | VOID, 64, 72)
        want = (k | VOID | VLIST, 64, LIVE + ROW, 3) if v == DEFAULT | NOMISS else (k, 64, 64, 3)
        assert irt.plan(v, flags=irt.PLAN_VOID_LIST | irt.PLAN_CHAIN, frames=3, void_live=LIVE, void_row=ROW)[:4] == want
    for v in (5376, 36864):  # four-wave workgroups; the statistics variant: their own kernel whatever is asked
        for flags, ns in ((0, 0), (irt.PLAN_SLOTS, 8), (irt.PLAN_VOID_BITS | irt.PLAN_VOID_LIST, 0)):
            assert irt.plan(v, flags=flags, tiles=3, num_split=ns, void_live=LIVE, void_row=ROW)[:4] == \
                (v & ~MONO, 256, 48 + ns, 1)
    base = d & ~(0xF00 | WAVEWG | LEAN)
    assert irt.plan(DEFAULT, sampler=irt.MODE_CUBQL)[:3] == (base | WEDGE, 256, 16)
    assert irt.plan(DEFAULT, sampler=irt.MODE_TRIANGLES, accel=1)[:3] == (base | WEDGE | GRID, 256, 16)
    assert irt.plan(DEFAULT, accel=1)[:3] == (base | 0x400 | GRID, 256, 16)
    queued = irt.plan(5376, flags=irt.PLAN_QUEUE, tiles=3, frames=3, queue_wg=QUEUE_WG)
    assert queued == ((5376 & ~MONO | QUEUE, 256, QUEUE_WG, 1, 48) if AB else (5376 & ~MONO, 256, 48, 3, 48))
    if AB:
        assert irt.plan(5120 | SERIAL, accel=1)[0] == base | 0x400 | GRID | SERIAL
        assert irt.plan(5120 | SERIAL, sampler=irt.MODE_CUBQL)[0] == base | WEDGE | SERIAL
        assert irt.plan(DEFAULT, flags=irt.PLAN_QUEUE)[0] == d, "one-wave workgroups: no persistent form"
    with pytest.raises(irt.IrtError):
        irt.plan(12345)  # not compiled


def test_workgroup_bound_covers_every_grid_launch():
    """irt_debug_launch_workgroups' figure (here without a context: irt_debug_variant_workgroups) is
    at least the grid of every non-queued plan at the same tiles and frames -- with work items only
    where a launch can have them: a single frame of a context with scheduling on whose variant has a
    split form (the default and its scene forms)."""
    flags = [f for f in range(32) if not f & irt.PLAN_QUEUE]
    for v, tiles, frames, sched in itertools.product(irt.compiled_variants(), (1, 3), (1, 3), (False, True)):
        bound = irt.variant_workgroups(v, sched, tiles, frames)
        per = 4 if v & WAVEWG else 1
        family = v in (DEFAULT, DEFAULT | NOMISS, DEFAULT | VOIDLOC)
        assert bound == tiles * 16 * per * frames + (MAX_SPLIT if sched and frames == 1 and per == 4 else 0)
        for sampler, accel, f, ns in itertools.product((irt.MODE_USER_GEOM, irt.MODE_CUBQL), (0, 1), flags,
                                                       (0, 8) if sched and frames == 1 and family else (0,)):
            p = irt.plan(v, sampler, accel, f, tiles, frames, ns, LIVE, ROW, 0)
            assert p[2] * p[3] <= bound, (v, sampler, accel, f, tiles, frames, ns)


@pytest.mark.skipif(not os.path.exists(irt.ALL_LIB_PATH), reason="make VARIANTS=all not built")
def test_launch_plan_ab_library():
    """The tests above on the A/B library (every variant, the persistent form, the OPT_SERIAL
    carry-over), in a child process: one HIP library per process (IRT_LIB_PATH selects it at load)."""
    env = dict(os.environ, IRT_LIB_PATH=irt.ALL_LIB_PATH)
    r = subprocess.run([sys.executable, "-u", "-m", "pytest", "-x", "-q", "-p", "no:cacheprovider"] +
                       [f"{__file__}::{t}" for t in ("test_plan_rules", "test_forms_each_variant_has",
                                                     "test_workgroup_bound_covers_every_grid_launch")],
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "3 passed" in r.stdout
