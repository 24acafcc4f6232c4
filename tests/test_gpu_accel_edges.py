"""The majorant accelerators on edge records, against the oracle that rasterises layer by layer
(oracle_build_shell, oracle_build_grid, oracle_max_opacities): the shell's in-lane rectangles, the
wide list and its overflow, the running findHeight index on repeated heights and the literal
search on unsorted ones, the 256-record staging batches' tails, NaN / +-inf / +-FLT_MAX / +-0
values, the update path (k_shell_rebuild and its data-range fold) and transfer functions whose
range misses the data.  Scenes: tests/accel_scenes.py; tests/test_accel_scenes_cpu.py shows
that they hold what is relied on here.

Every comparison is exact: value ranges equal as numbers (the sign of a zero bound follows the
atomics' arrival order, in the reference too; ranges never hold NaN), majorants and the grid's
empty-space bitmap bit for bit.  Transfer functions are explicit and finite (the data range of
these scenes may not be).
"""
import functools

import numpy as np
import pytest

import accel_scenes as A
import irt
import oracle as O
from helpers import bits

pytestmark = pytest.mark.gpu

LUT = A.edge_lut(16)
GRID = 256
GRID_BLOCK = 8  # irt_common.h kGridBlock


def tf_range(name):
    """An explicit finite range over the scene's finite values."""
    return (0.0, 1.0) if name == "mixed_rects" else (50.0, 100.0 + 640 * 32)


def build_oracle(cells):
    S = O.OracleScene(cells)
    S.build_grid()
    return S


@functools.lru_cache(maxsize=None)
def oracle(name):
    """The yardstick of a named scene (shell and grid value ranges), shared and never changed."""
    S = build_oracle(A.scene(name))
    S.value_ranges.setflags(write=False)
    S.grid_vr.setflags(write=False)
    return S


def oracle_majorants(vr, lut, value_range):
    lut = np.ascontiguousarray(lut, dtype=np.float32).reshape(-1, 4)
    out = np.zeros(vr.shape[0], np.float32)
    O.olib().oracle_max_opacities(O._p(vr), vr.shape[0], O._p(lut), lut.shape[0], float(value_range[0]),
                                  float(value_range[1]), O._p(out))
    return out


def grid_bits_of(mo):
    """k_grid_bits restated: bit b (block b of 8^3 cells, x fastest) is set iff any of the block's
    majorants is not <= 0; 32 blocks per word, least significant bit first."""
    nb = GRID // GRID_BLOCK
    m = ~(mo.reshape(nb, GRID_BLOCK, nb, GRID_BLOCK, nb, GRID_BLOCK) <= 0)
    any_ = m.any(axis=(1, 3, 5)).reshape(-1)  # (bz, by, bx) row-major: b = (bz * nb + by) * nb + bx
    return np.packbits(any_, bitorder="little").view(np.uint32)


def same_ranges(got, want, what):
    assert not np.isnan(got).any(), f"{what}: NaN in the value ranges"
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, (f"{what}: {bad.size} macrocells differ, first {bad[0]}: "
                           f"{got[bad[0]].tolist()} for {want[bad[0]].tolist()}")


def same_majorants(got, want, what):
    bad = np.flatnonzero(bits(got) != bits(want))
    assert bad.size == 0, f"{what}: {bad.size} majorants differ, first {bad[0]}: {got[bad[0]]!r} for {want[bad[0]]!r}"


def assert_accel(ctx, S, lut, value_range, what, shell=True, grid=True):
    """The context's shell and grid against the oracle's ranges of S and the oracle's majorants
    over them for (lut, value_range) -- the transfer function the context holds."""
    if shell:
        vr, mo = ctx.shell()
        same_ranges(vr, S.value_ranges, f"{what}: shell")
        same_majorants(mo, oracle_majorants(S.value_ranges, lut, value_range), f"{what}: shell")
    if grid:
        vr, mo = ctx.grid()
        same_ranges(vr, S.grid_vr, f"{what}: grid")
        same_majorants(mo, oracle_majorants(S.grid_vr, lut, value_range), f"{what}: grid")
        got = ctx.array("grid_bits").view(np.uint32)
        assert np.array_equal(got, grid_bits_of(mo)), f"{what}: grid bitmap"


def with_values(cells, vals):
    out = np.array(cells, copy=True)
    out["value"] = vals
    return out


def updated_context(name, grid_first):
    """A context created from scene(name)'s records with the synthetic grid's values, then
    updated in place to the scene's own value[]."""
    cells = A.scene(name)
    ctx = irt.Context(with_values(cells, A.untreated_values(name)), 0)
    ctx.set_transfunc(LUT, tf_range(name))
    if grid_first:
        ctx.grid()  # built from the old values: the commit has to rebuild it
    ctx.update_values(np.ascontiguousarray(cells["value"]))
    ctx.end_update()
    return ctx


def assert_same_as_fresh(ctx, fresh, what):
    """The fresh-context yardstick of tests/test_gpu_update_values.py, beside the oracle."""
    assert np.array_equal(ctx.array("blocks"), fresh.array("blocks")), f"{what}: blocks"
    (vr, mo), (fvr, fmo) = ctx.shell(), fresh.shell()
    same_ranges(vr, fvr, f"{what}: shell against a fresh context")
    same_majorants(mo, fmo, f"{what}: shell against a fresh context")
    assert bytes(ctx.info)[:-8] == bytes(fresh.info)[:-8], f"{what}: volume info"  # all but deviceBytes


# ------------------------------------------------------------------ 1. creation
@pytest.fixture(scope="module")
def mixed_ctx():
    ctx = irt.Context(A.mixed_rects(), 0)
    yield ctx
    ctx.close()


def test_mixed_rects_match_oracle(mixed_ctx):
    """In-lane rectangles of a few and of 28..56 macrocells, and more wide ones than the list
    holds (k_shell_build, k_shell_rects); the grid's merged and deferred boxes."""
    name = "mixed_rects"
    mixed_ctx.set_transfunc(LUT, tf_range(name))
    assert_accel(mixed_ctx, oracle(name), LUT, tf_range(name), name)


@pytest.mark.parametrize("name", ["heights", "nonfinite_values"])
def test_created_context_matches_oracle(name):
    ctx = irt.Context(A.scene(name), 0)
    ctx.set_transfunc(LUT, tf_range(name))
    assert_accel(ctx, oracle(name), LUT, tf_range(name), name)
    assert bytes(ctx.info.dataRange) == bytes(irt.volume_info(A.scene(name)).dataRange)
    ctx.close()


@pytest.mark.parametrize("n", A.TAIL_SIZES)
def test_batch_tails_match_oracle(n):
    """n records around the 256-record staging batches of k_shell_build and k_shell_rebuild,
    n % 4 != 0 among them: created, and updated in place."""
    name = f"tails_{n}"
    cells = A.scene(name)
    S = build_oracle(cells)
    ctx = irt.Context(cells, 0)
    ctx.set_transfunc(LUT, tf_range(name))
    assert_accel(ctx, S, LUT, tf_range(name), name)
    upd = updated_context(name, grid_first=True)
    assert_accel(upd, S, LUT, tf_range(name), f"{name} updated")
    assert_same_as_fresh(upd, ctx, name)
    ctx.close()
    upd.close()


# ------------------------------------------------------------------ 2. the update path
@pytest.mark.parametrize("grid_first", [True, False], ids=["grid_rebuilt", "grid_built_after"])
@pytest.mark.parametrize("name", ["heights", "nonfinite_values"])
def test_updated_context_matches_oracle(name, grid_first):
    """irt_update_values_end against the oracle of the treated records, not only against a
    context that ran the same shell_record_range at creation."""
    ctx = updated_context(name, grid_first)
    assert_accel(ctx, oracle(name), LUT, tf_range(name), f"{name} updated")
    fresh = irt.Context(A.scene(name), 0)
    fresh.set_transfunc(LUT, tf_range(name))
    assert_same_as_fresh(ctx, fresh, name)
    ctx.close()
    fresh.close()


# ------------------------------------------------------------------ 3. the data-range fold
def test_data_range_fold():
    """ctx.info.dataRange after the commit, byte for byte: a fresh context's and the host fold's
    (irt.volume_info), on value sets that decide the zero-sign rule, the unused slots, waves and
    workgroups without a value, and +-inf.  In sequence on one context, so each commit also has
    to forget the previous one's range."""
    cells = A.range_scene()
    ctx = irt.Context(cells, 0)
    for name, vals in A.range_value_sets().items():
        ctx.update_values(vals)
        ctx.end_update()
        treated = with_values(cells, vals)
        want = irt.volume_info(treated).dataRange
        fresh = irt.Context(treated, 0)
        got = ctx.info.dataRange
        print(f"{name}: updated ({got.lower!r}, {got.upper!r}), host fold ({want.lower!r}, {want.upper!r})")
        assert bytes(got) == bytes(want), name
        assert bytes(got) == bytes(fresh.info.dataRange), name
        same_ranges(ctx.shell()[0], fresh.shell()[0], name)
        fresh.close()
    ctx.close()


# ------------------------------------------------------------------ 4. transfer-function edges
TF_RANGES = {  # the data of mixed_rects lies in [0, 1]
    "narrower": (0.3, 0.7), "below": (-2.0, -1.0), "above": (2.0, 3.0), "reversed": (0.8, 0.2), "equal": (0.5, 0.5)}


@pytest.mark.parametrize("size", [1, 2, 7, 300, 1024])
def test_transfer_function_edges(mixed_ctx, size):
    """k_max_opacities and k_grid_bits with LUTs of 1 .. 1024 entries over value ranges narrower
    than the data, beside it, reversed and empty, on the shell and on the built grid."""
    S = oracle("mixed_rects")
    assert S.data_range[0] < 0.3 and S.data_range[1] > 0.7
    lut = A.edge_lut(size)
    mixed_ctx.grid()
    for what, value_range in TF_RANGES.items():
        mixed_ctx.set_transfunc(lut, value_range)
        assert_accel(mixed_ctx, S, lut, value_range, f"{size} entries, {what}")
