"""The raygen from cameras inside, under, south of and beside the globe (helpers.view_battery).

Every other GPU frame test looks at the globe from outside, on or near the +z axis.  The views
here take the ray setup of render_pixel / render_pixel_coop (irt_render.hip: box_test,
intersect_spheres, the range selection of ShellAccel.h:87-111) through all of its branches --
tests/test_views_cpu.py::test_battery_reaches_every_range_case counts them -- including ranges
that start behind the camera (a first leaf [lower < 0, 0], then zero-length leaves at t = 0),
entry points at negative latitudes, frames whose rays all miss the box (nothing may be written)
or all find no range, and the host's cost model (irt_deal_tiles, measured-cost scheduling) on
such frames.  Every comparison is of accum bit patterns, fb words and the counts raysLaunched,
raysInBox, locateCalls and samplesFound; the oracle is pinned to the reference at these views
by tests/test_views_cpu.py and the f9_view_* golden frames.

The oracle's figures at 88 x 72 (6336 rays), flat | terrain scene: raysInBox, locateCalls,
samplesFound, share of pixels with alpha > 0:
  south_oblique  5503  5069  5069 0.499 | 5492  5670  4521 0.497
  shell_down     6336 11842 11842 1.000 | 6336 25226  9897 1.000
  shell_horizon  6336  9822  9822 1.000 | 6336 47554  8400 1.000
  shell_up       6336  6866  6866 1.000 | 6336 28667  7582 1.000
  underground    6336 10176 10176 1.000 | 6336 12878 10236 1.000
  centre         6336  8678  8678 0.988 | 6336 11010  8752 0.988
  corner_away    6336     0     0 0     | 6336     0     0 0
  away              0     0     0 0     |    0     0     0 0
  graze          6336  5258  5258 0.449 | 6336 17031  3439 0.449
  framing        6336  6275  6272 0.631 | 6336  7298  5701 0.630
"""
import ctypes as C
import functools

import numpy as np
import pytest

import irt
import oracle as O
from helpers import VIEW_NAMES, bits, view_battery
from test_gpu_scale import host_threads

pytestmark = pytest.mark.gpu

W, H = 88, 72  # ragged against 16x16 blocks and 64x64 tiles, not against 8x8 packets (11 x 9 of them:
#                tests/test_gpu_ragged.py has the sizes that cut packets); not square
VIEWS = list(VIEW_NAMES)
NOT_FRAMING = [v for v in VIEWS if v != "framing"]
NOMISS, VOIDLOC = 262144, 1073741824


@functools.lru_cache(maxsize=None)
def _cells(scene):
    cells = {"flat": lambda: irt.synth_grid(2, 2, 47),
             "terrain": lambda: irt.synth_grid(2, 2, 65, terrain=4000.0),  # holes: miss mode, void walk
             "small": lambda: irt.synth_grid(2, 1, 20)}[scene]()
    cells.setflags(write=False)
    return cells


@functools.lru_cache(maxsize=None)
def _oracle_scene(scene):
    S = O.OracleScene(_cells(scene))
    lut, vr = S.default_lut()
    S.set_transfunc(lut, vr)
    return S


def _pattern(w, h):
    """A non-zero frame to render into: a pixel the raygen must leave alone shows if written."""
    i = np.arange(w * h, dtype=np.uint32).reshape(h, w)
    fb = (np.uint32(0xA5000000) | (i * np.uint32(2654435761) >> np.uint32(8))).astype(np.uint32)
    accum = (0.125 + (i[..., None] * 4 + np.arange(4, dtype=np.uint32)) % 61 / 64.0).astype(np.float32)
    return accum, fb


@functools.lru_cache(maxsize=None)
def _oracle(scene, view, form="frame", w=W, h=H):
    """The oracle's (accum, fb, per-frame counts) of one view, rendered over _pattern; forms:
    frame, ae, grid, triangles, cubql, progressive (accumIDs 0..3).  Shared: do not modify."""
    S = _oracle_scene(scene)
    kw = {"ae": dict(raygen=1), "grid": dict(accel_mode=1), "triangles": dict(mode=irt.MODE_TRIANGLES),
          "cubql": dict(mode=irt.MODE_CUBQL)}.get(form, {})
    cam = S.camera(w, h, view_battery(_cells(scene))[view])
    accum, fb = _pattern(w, h)
    counts = []
    for aid in (0, 1, 2, 3) if form == "progressive" else (0,):
        p = S.params(cam, accum_id=aid, **kw)
        _, _, st = S.render(p, w, h, accum=accum, fb=fb, threads=host_threads(),
                            fast=1 if "mode" in kw else 2)
        counts.append((st.rays_launched, st.rays_in_box, st.locate_calls, st.samples_found))
    accum.setflags(write=False)
    fb.setflags(write=False)
    return accum, fb, counts


def _context(scene):
    cells = _cells(scene)
    setup = irt.setup_frame(cells, W, H)
    ctx = irt.Context(cells, 0)
    ctx.set_transfunc(setup.lut, setup.value_range)
    return ctx


def _lp(scene, view, w=W, h=H, **kw):
    cells = _cells(scene)
    lp = irt.setup_frame(cells, w, h, camera=view_battery(cells)[view], raygen=kw.pop("raygen", 0)).lp
    for k, v in kw.items():
        setattr(lp, k, v)
    return lp


def _counts(st):
    return (st.raysLaunched, st.raysInBox, st.locateCalls, st.samplesFound)


class _Frame:
    """Device fb/accum holding _pattern."""

    def __init__(self, w=W, h=H):
        import torch
        self.torch, self.w, self.h = torch, w, h
        a, f = _pattern(w, h)
        self.accum = torch.from_numpy(a.reshape(-1).copy()).cuda()
        self.fb = torch.from_numpy(f.view(np.int32).reshape(-1).copy()).cuda()

    def host(self):
        self.torch.cuda.synchronize()
        return (self.accum.cpu().numpy().reshape(self.h, self.w, 4),
                self.fb.cpu().numpy().view(np.uint32).reshape(self.h, self.w))


def _render(ctx, lp, w=W, h=H):
    fr = _Frame(w, h)
    ctx.render(lp, w, h, fr.fb.data_ptr(), fr.accum.data_ptr())
    a, f = fr.host()
    return a, f, _counts(ctx.stats())


def _assert_same(got, want, label):
    a, f, n = got
    a_ref, f_ref, n_ref = want
    bad = np.any(bits(a) != bits(a_ref), axis=-1) | (f != f_ref)
    assert not bad.any(), (f"{label}: {int(bad.sum())} of {bad.size} pixels differ, first (y, x) "
                           f"{np.argwhere(bad)[:4].tolist()}; counts {n} vs {n_ref}")
    assert tuple(n) == tuple(n_ref), f"{label}: counts {n} vs {n_ref}"


@pytest.fixture(scope="module", params=["flat", "terrain"])
def scene(request):
    ctx = _context(request.param)
    yield request.param, ctx
    ctx.close()


# ---- 1. single frames, every view x both scenes
@pytest.mark.parametrize("view", VIEWS)
def test_view_matches_oracle(scene, view):
    """One frame over a non-zero pattern: pixels whose ray misses the box (all of `away`, the
    edge of `south_oblique`) must keep it; `corner_away` is in the box on every pixel and samples
    nothing."""
    name, ctx = scene
    a_ref, f_ref, n_ref = _oracle(name, view)
    if view == "corner_away":
        assert n_ref[0][1] == W * H and n_ref[0][2] == 0
    if view == "away":
        assert n_ref[0][1] == 0
        pa, pf = _pattern(W, H)
        assert np.array_equal(bits(a_ref), bits(pa)) and np.array_equal(f_ref, pf)
    got = _render(ctx, _lp(name, view))
    if view == "corner_away":
        assert got[2][1] == W * H and got[2][2] == 0
    if view == "away":
        assert got[2][1] == 0
    _assert_same(got, (a_ref, f_ref, n_ref[0]), f"{name} {view}")


# ---- 2. the other raygens and accelerators
@pytest.mark.parametrize("form", ["ae", "grid"])
@pytest.mark.parametrize("view", NOT_FRAMING)
def test_view_ae_and_grid_match_oracle(view, form):
    """woodcockTrackingAE (the box interval, from inside the box too) and GRID_ACCEL_MODE (dda3
    from a camera inside the grid), flat scene."""
    ctx = _context("flat")
    kw = dict(raygen=irt.RAYGEN_AE) if form == "ae" else dict(accelMode=irt.ACCEL_GRID)
    a_ref, f_ref, n_ref = _oracle("flat", view, form)
    _assert_same(_render(ctx, _lp("flat", view, **kw)), (a_ref, f_ref, n_ref[0]), f"{view} {form}")
    ctx.close()


@pytest.mark.parametrize("form", ["cubql", "triangles"])
@pytest.mark.parametrize("view", ["shell_down", "underground", "south_oblique"])
def test_view_sampler_modes_match_oracle(view, form):
    """MODE_CUBQL (wedges) and MODE_TRIANGLES on synth_grid(2, 1, 20) at 48 x 48."""
    w = 48
    cells = _cells("small")
    ctx = irt.Context(cells, 0)
    setup = irt.setup_frame(cells, w, w)
    ctx.set_transfunc(setup.lut, setup.value_range)
    ctx.build_wedge_accel(cells)
    mode = irt.MODE_CUBQL if form == "cubql" else irt.MODE_TRIANGLES
    a_ref, f_ref, n_ref = _oracle("small", view, form, w, w)
    _assert_same(_render(ctx, _lp("small", view, w, w, mode=mode), w, w), (a_ref, f_ref, n_ref[0]),
                 f"{view} {form}")
    ctx.close()


# ---- 3. progressive, chained
@pytest.mark.parametrize("view", ["shell_down", "shell_horizon", "underground"])
def test_view_progressive_chained(view):
    """irt_render_accumulate, frames 0..3 in one chained launch on the terrain scene == the
    oracle's four frames == the same launch unchained."""
    ctx = _context("terrain")
    a_ref, f_ref, n_ref = _oracle("terrain", view, "progressive")
    total = tuple(int(sum(n[k] for n in n_ref)) for k in range(4))
    out = {}
    for chain in (True, False):
        ctx.set_chain(chain)
        fr = _Frame()
        ctx.render_accumulate(_lp("terrain", view), W, H, 4, fr.fb.data_ptr(), fr.accum.data_ptr())
        a, f = fr.host()
        out[chain] = (a, f, _counts(ctx.stats()))
        _assert_same(out[chain], (a_ref, f_ref, total), f"{view} chain={chain}")
    _assert_same(out[True], out[False], f"{view} chained vs unchained")
    assert ctx.chain_errors() == 0
    ctx.close()


# ---- 4. the whole battery as one sequence
def test_battery_as_one_sequence(scene):
    """One camera per frame (accumID 0) in one chained launch: box-miss, zero-range and full
    frames side by side, the camera origin differing per wave.  == the views one launch each ==
    the oracle's frames rendered one over the other, with summed counts."""
    name, ctx = scene
    lps = [_lp(name, v) for v in VIEWS]
    S = _oracle_scene(name)
    accum, fb = _pattern(W, H)
    total = np.zeros(4, np.int64)
    for v in VIEWS:
        p = S.params(S.camera(W, H, view_battery(_cells(name))[v]))
        _, _, st = S.render(p, W, H, accum=accum, fb=fb, threads=host_threads(), fast=2)
        total += (st.rays_launched, st.rays_in_box, st.locate_calls, st.samples_found)
    want = (accum, fb, tuple(int(t) for t in total))
    ctx.set_chain(True)
    fr = _Frame()
    ctx.reset_stats_total()
    for q in lps:
        ctx.render(q, W, H, fr.fb.data_ptr(), fr.accum.data_ptr())
    a, f = fr.host()
    _assert_same((a, f, _counts(ctx.stats_total()[0])), want, f"{name}: one launch per view")
    fr = _Frame()
    ctx.render_sequence(lps, W, H, fr.fb.data_ptr(), fr.accum.data_ptr())
    a, f = fr.host()
    _assert_same((a, f, _counts(ctx.stats())), want, f"{name}: sequence")
    assert ctx.chain_errors() == 0


# ---- 5. the host cost model
@pytest.mark.parametrize("view", ["shell_down", "away", "corner_away", "graze"])
def test_dealt_tiles_of_view_match_full_frame(scene, view):
    """irt_deal_tiles on frames whose rays all hit, all miss the box or all find no range (an
    all-zero cost estimate): every tile dealt exactly once over 1, 3 and 8 ranks, and the dealt
    irt_render_tile_list + irt_unpack_tile_table assembly == the full frame."""
    import torch
    import irt_dist
    name, ctx = scene
    lp = _lp(name, view)
    fb = torch.zeros(W * H, dtype=torch.int32, device="cuda")
    acc = torch.zeros(W * H * 4, dtype=torch.float32, device="cuda")
    ctx.render(lp, W, H, fb.data_ptr(), acc.data_ptr())
    torch.cuda.synchronize()
    full, full_counts = fb.cpu().numpy(), _counts(ctx.stats())
    ntot = irt.num_tiles(W, H)
    for ranks in (1, 3, 8):
        table = irt.deal_tiles(lp, ctx.info, W, H, ranks)
        assert sorted(int(t) for t in table.ravel() if t >= 0) == list(range(ntot)), (ranks, table)
        splits = [irt_dist.TileSplit.dealt(W, H, r, ranks, lp, ctx.info) for r in range(ranks)]
        dealt = sorted(t for sp in splits for t in sp.tiles())
        assert dealt == list(range(ntot)), (ranks, dealt)
        maxt = splits[0].max_tiles
        gathered = torch.zeros(ranks * maxt * 4096, dtype=torch.int32, device="cuda")
        counts = np.zeros(4, np.int64)
        for r, sp in enumerate(splits):
            tacc = torch.zeros(maxt * 4096 * 4, dtype=torch.float32, device="cuda")
            sp.render(ctx, lp, 1, gathered[r * maxt * 4096:].data_ptr(), tacc.data_ptr())
            if sp.tiles():
                counts += _counts(ctx.stats())
        out = torch.zeros(W * H, dtype=torch.int32, device="cuda")
        splits[0].unpack(ctx, gathered.data_ptr(), out.data_ptr())
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy(), full), f"{name} {view}: {ranks} ranks"
        assert tuple(int(c) for c in counts) == full_counts, f"{name} {view}: {ranks} ranks"


def test_scheduled_frames_of_view_equal_unscheduled(monkeypatch):
    """Measured-cost scheduling with split packets (IRT_SCHED=1, IRT_SPLIT_FACTOR=1e-6) over 24
    frames of shell_horizon on the terrain scene == an IRT_SCHED=0 context frame for frame, and
    the later launches did split.  At 88 x 72: 30 blocks of 16 x 16, 120 packets, of which the
    costliest tenth splits, so the schedule engages at this size."""
    import torch
    cells = _cells("terrain")
    setup = irt.setup_frame(cells, W, H)
    monkeypatch.setenv("IRT_SCHED", "0")
    ref_ctx = irt.Context(cells, 0)
    monkeypatch.setenv("IRT_SCHED", "1")
    monkeypatch.setenv("IRT_SPLIT_FACTOR", "1e-6")
    ctx = irt.Context(cells, 0)
    lp = _lp("terrain", "shell_horizon")
    out = {}
    for c in (ref_ctx, ctx):
        c.set_transfunc(setup.lut, setup.value_range)
        fr = _Frame()
        res = []
        for aid in range(24):
            lp.accumID = aid
            c.render(lp, W, H, fr.fb.data_ptr(), fr.accum.data_ptr())
            a, f = fr.host()
            res.append((a, f, _counts(c.stats()), c.sched_split()[0]))
        out[c] = res
    for k, (g, r) in enumerate(zip(out[ctx], out[ref_ctx])):
        _assert_same(g[:3], r[:3], f"frame {k}")
    assert all(r[3] == 0 for r in out[ref_ctx])
    splits = [g[3] for g in out[ctx]]
    assert max(splits[8:]) >= 8 and max(splits) % 8 == 0, splits
    a_ref, f_ref, n_ref = _oracle("terrain", "shell_horizon")
    assert out[ctx][0][2] == n_ref[0]  # frame 0 starts from the same pattern as the oracle's
    ref_ctx.close()
    ctx.close()


# ---- 6. kernel forms
@pytest.mark.parametrize("view", ["shell_down", "underground"])
def test_view_under_every_kernel_form(monkeypatch, scene, view):
    """Every render variant the product library compiled, the hole form the scene does not
    select by itself included, and a context with the slot table forced (IRT_SLOTS=1): the
    default's frame and counts, which are the oracle's."""
    name, _ = scene
    L = irt.lib()
    L.irt_debug_set_variant.argtypes = [C.c_void_p, C.c_int]
    a_ref, f_ref, n_ref = _oracle(name, view)
    want = (a_ref, f_ref, n_ref[0])
    lp = _lp(name, view)
    ctx = _context(name)
    _assert_same(_render(ctx, lp), want, f"{name} {view} default")
    d = L.irt_debug_default_variant()
    forms = list(irt.compiled_variants())
    for v in (d | NOMISS, d | VOIDLOC) if name == "terrain" else (d | NOMISS,):
        if v not in forms:
            forms.append(v)
    for v in forms:
        assert L.irt_debug_set_variant(ctx._h, v) == 0, v
        _assert_same(_render(ctx, lp), want, f"{name} {view} variant {v}")
    ctx.close()
    monkeypatch.setenv("IRT_SLOTS", "1")
    ctx = _context(name)
    assert (ctx.array_bytes("slots") > 0) == (name == "flat")
    _assert_same(_render(ctx, lp), want, f"{name} {view} IRT_SLOTS=1")
    ctx.close()
