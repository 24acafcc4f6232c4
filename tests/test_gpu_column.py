"""The column products on the device (csrc/irt_column.hip), bit for bit: irt_column_latlon against
irt_column_reduce of the oracle's grid answers and of the device's own irt_sample_latlon output,
irt_render_column against the restatement of its definition (tests/column_scenes.py), on the
inputs tests/test_column_cpu.py takes its census of; then the calls' conduct.  Every output goes
to a buffer pre-filled with a sentinel, with guard words on both sides."""
import ctypes as C

import numpy as np
import pytest

import column_scenes as CS
import irt
import levels_scenes as LS
import sample_scenes as S
from test_gpu_levels import SENT, Frame
from test_gpu_sample import sample_latlon, sample_points

pytestmark = pytest.mark.gpu

GUARD = 96
F = np.float32
MODES = {"cubql": irt.MODE_CUBQL, "triangles": irt.MODE_TRIANGLES}


class Columns:
    """The six outputs of n columns as device buffers between guards, sentinel-filled; `which`:
    the outputs handed to the call (the others stay NULL)."""

    def __init__(self, shape, which=CS.OUTPUTS, device=0):
        import torch
        self.torch, self.shape, self.n, self.which = torch, tuple(shape), int(np.prod(shape)), tuple(which)
        self.buf = {k: torch.full((self.n + 2 * GUARD,), SENT, dtype=torch.int32, device=f"cuda:{device}")
                    for k in CS.OUTPUTS}

    def ptrs(self):
        return {k: self.buf[k].data_ptr() + 4 * GUARD for k in self.which}

    def host(self, written=True):
        """The outputs as a dict of (shape) arrays, after checking the guards, and that an output
        not handed over (or, written=False, any output) still holds the sentinel."""
        out = {}
        for k, t in self.buf.items():
            v = t.cpu().numpy().view(np.uint32)
            assert (v[:GUARD] == SENT).all() and (v[GUARD + self.n:] == SENT).all(), f"{k} guards"
            v = v[GUARD:GUARD + self.n]
            if not written or k not in self.which:
                assert (v == SENT).all(), f"{k} was written"
            else:
                out[k] = v.view(irt.COLUMN_OUTPUTS[k]).reshape(self.shape)
        return out


def column_latlon(ctx, grid, wname, mode=irt.MODE_USER_GEOM, miss=CS.MISS, which=CS.OUTPUTS, stream=0):
    lat, lon, rad = grid
    cols = Columns((lat.size, lon.size), which, ctx.device)
    assert ctx.column_latlon(lat, lon, rad, cols.ptrs(), CS.weights(wname, rad.size), mode, miss, stream) == \
        (lat.size, lon.size)
    cols.torch.cuda.synchronize(ctx.device)
    return cols.host()


def two_pass(ctx, grid, wname, mode=irt.MODE_USER_GEOM, miss=CS.MISS):
    """irt_column_reduce of the device's own irt_sample_latlon output: the header's promise."""
    lat, lon, rad = grid
    f, v = sample_latlon(ctx, grid, mode, miss)
    shape = (rad.size, lat.size, lon.size)
    return irt.column_reduce(v.reshape(shape), f.reshape(shape), CS.weights(wname, rad.size), miss)


def check_columns(got, want, what, which=CS.OUTPUTS):
    assert set(got) == set(which)
    k = CS.same_outputs(got, want, which)
    if k is not None:
        bad = np.argwhere(CS.bits(got[k]) != CS.bits(want[k]))
        raise AssertionError(f"{what}: {k} differs in {len(bad)} of {got[k].size} columns, first {tuple(bad[0])}: "
                             f"{got[k][tuple(bad[0])]!r} vs {want[k][tuple(bad[0])]!r}")


# ------------------------------------------------------------------ irt_column_latlon, cell sampler
@pytest.mark.parametrize("slots", [False, True], ids=["headers", "slots"])
@pytest.mark.parametrize("name", CS.SCENE_NAMES)
def test_column_latlon_equals_the_oracles_reduction(monkeypatch, name, slots):
    """Three grids x three weight sets per scene, from headers and (IRT_SLOTS=1) from the slot table
    where the scene has one: every output equals, as bits, irt_column_reduce of the oracle's grid
    answers -- and of irt_sample_latlon's output on the device."""
    if slots:
        monkeypatch.setenv("IRT_SLOTS", "1")
    with irt.Context(S.scene(name), 0) as ctx:
        assert (ctx.array_bytes("slots") > 0) == (slots and name != "terrain")
        for key in CS.GPU_GRIDS:
            for wname in CS.WEIGHTS:
                want = CS.reduced(name, key, wname)
                got = column_latlon(ctx, CS.grid(name, key), wname)
                print(f"{name} {key} {wname}: {int((want['count'] > 0).sum())} of {want['count'].size} columns found")
                check_columns(got, want, f"irt_column_latlon {name} {key} {wname} against the oracle")
                check_columns(got, two_pass(ctx, CS.grid(name, key), wname),
                              f"irt_column_latlon {name} {key} {wname} against irt_sample_latlon")
        # a NaN missValue, and the ascending order of the same levels
        nan = column_latlon(ctx, CS.grid(name, "all"), "mixed", miss=float("nan"))
        check_columns(nan, CS.reduced(name, "all", "mixed", float("nan")), f"{name}: NaN missValue")
        check_columns(column_latlon(ctx, CS.grid(name, "all_ascending"), "none"),
                      CS.reduced(name, "all_ascending", "none"), f"{name}: ascending levels")


# ------------------------------------------------------------------ wedge and triangle samplers
@pytest.mark.parametrize("mode", list(MODES))
def test_column_latlon_of_the_unstructured_samplers(mode):
    """On the flat scene, against irt_column_reduce of the device's own irt_sample_latlon output
    (the samplers' own parity with the oracle is pinned in tests/test_gpu_samplers.py)."""
    cells = S.scene("flat")
    with irt.Context(cells, 0) as ctx:
        ctx.build_wedge_accel(cells)
        for key in CS.GPU_GRIDS:
            for wname in ("none", "mixed"):
                want = two_pass(ctx, CS.grid("flat", key), wname, MODES[mode])
                if key == "all":
                    assert (want["count"] > 0).sum() >= 100 and (want["kmax"] != want["kmin"]).sum() >= 100
                check_columns(column_latlon(ctx, CS.grid("flat", key), wname, MODES[mode]), want,
                              f"irt_column_latlon {mode} flat {key} {wname}")


# ------------------------------------------------------------------ irt_render_column
def make_context(name, mode=irt.MODE_USER_GEOM):
    cells = S.scene(name)
    ctx = irt.Context(cells, 0)
    lut, vr, scale = CS.transfunc(name)
    ctx.set_transfunc(lut, vr, scale)
    if mode != irt.MODE_USER_GEOM:
        ctx.build_wedge_accel(cells)
    return ctx


def render(ctx, frame, case, mode=irt.MODE_USER_GEOM, value=True, stream=0):
    name, view_name, size, accum_id, product, wname = case
    ctx.render_column(LS.launch_params(name, view_name, size, accum_id, mode), frame.W, frame.H, CS.surface(name),
                      CS.levels(name, "render"), frame.ptr("fb"), frame.ptr("accum"),
                      frame.ptr("value") if value else 0, CS.render_weights(name, wname), CS.PRODUCTS[product],
                      CS.MISS, stream)
    frame.torch.cuda.synchronize(ctx.device)


def new_frame(case):
    W, H = LS.SIZES[case[2]]
    return Frame(W, H, prior=LS.prior_accum(W, H) if case[3] else np.zeros((H, W, 4), F))


def check_frame(frame, want, what, value=True):
    for which, exp in (("fb", want.fb), ("accum", want.accum), ("value", want.value)):
        written = value or which != "value"
        got = frame.host(which, written)
        if written:
            e = np.ascontiguousarray(exp).view(np.uint32).reshape(got.shape)
            bad = np.argwhere(got != e)
            assert len(bad) == 0, (f"{what}: {which} differs at {len(bad)} places, first {tuple(bad[0])}: "
                                   f"{hex(int(got[tuple(bad[0])]))} vs {hex(int(e[tuple(bad[0])]))}")
    frame.host("level", written=False)  # the call has no such output


@pytest.mark.parametrize("slots", [False, True], ids=["headers", "slots"])
@pytest.mark.parametrize("case", CS.FRAMES, ids=CS.frame_id)
def test_column_frames_equal_the_restatement(monkeypatch, case, slots):
    if slots:
        monkeypatch.setenv("IRT_SLOTS", "1")
    want = CS.expected_frame(*case)
    with make_context(case[0]) as ctx:
        assert (ctx.array_bytes("slots") > 0) == (slots and case[0] != "terrain")
        frame = new_frame(case)
        render(ctx, frame, case)
        print(f"{CS.frame_id(case)}: {int((want.columns['count'] > 0).sum())} of {frame.n} pixels found a column")
        check_frame(frame, want, CS.frame_id(case))


def test_column_frame_of_the_wedge_sampler():
    case = CS.SAMPLER_FRAME
    want = CS.expected_frame(*case, mode=irt.MODE_CUBQL)
    assert (want.columns["count"] > 0).sum() >= 30 and not np.isnan(want.value).any()
    with make_context(case[0], irt.MODE_CUBQL) as ctx:
        frame = new_frame(case)
        render(ctx, frame, case, irt.MODE_CUBQL)
        check_frame(frame, want, "cubql " + CS.frame_id(case))


@pytest.mark.parametrize("case", [CS.FRAMES[0], CS.FRAMES[4]], ids=CS.frame_id)
def test_frame_values_are_the_reduction_of_sampled_column_points(case):
    """d_value of every pixel is the chosen product of irt_column_reduce over irt_sample_points'
    answers at the restatement's column points of that pixel, bit for bit."""
    name, _, _, _, product, wname = case
    want = CS.expected_frame(*case)
    s = want.samples
    with make_context(name) as ctx:
        frame = new_frame(case)
        render(ctx, frame, case)
        f, v = sample_points(ctx, s.points, miss=CS.MISS)
        shape = s.found.shape
        f = f.reshape(shape) * s.live[None].astype(np.uint8)  # a pixel without a live hit has no column
        col = irt.column_reduce(v.reshape(shape), f, CS.render_weights(name, wname), CS.MISS)
        probe = col[{"wsum": "wsum", "max": "vmax", "min": "vmin"}[product]]
        assert (col["count"] > 0).sum() >= 100
        assert np.array_equal(frame.host("value"), CS.bits(probe))


# ------------------------------------------------------------------ NULL outputs
def test_null_outputs():
    name, key, wname = "terrain", "all", "mixed"
    want = CS.reduced(name, key, wname)
    case = CS.FRAMES[3]
    with make_context(name) as ctx:
        for which in (("wsum",), ("kmin", "count"), ("vmax", "vmin", "kmax")):
            check_columns(column_latlon(ctx, CS.grid(name, key), wname, which=which), want, f"only {which}", which)
        lat, lon, rad = CS.grid(name, key)
        cols = Columns((lat.size, lon.size), ())
        ctx.column_latlon(lat, lon, rad, {}, None)  # every pointer NULL: IRT_OK, nothing launched
        ctx.column_latlon(lat, lon, rad, {"wsum": 0, "count": 0}, None)
        cols.torch.cuda.synchronize(0)
        cols.host(written=False)
        frame = new_frame(case)
        render(ctx, frame, case, value=False)
        check_frame(frame, CS.expected_frame(*case), "d_value NULL", value=False)


def test_grids_without_points_launch_nothing():
    lat, lon, rad = CS.grid("flat", "five")
    none = np.zeros(0, F)
    with irt.Context(S.scene("flat"), 0) as ctx:
        cols = Columns((lat.size, lon.size))
        for g in ((none, lon, rad), (lat, none, rad), (lat, lon, none)):
            assert 0 in ctx.column_latlon(*g, cols.ptrs()) or g[2].size == 0
        cols.torch.cuda.synchronize(0)
        cols.host(written=False)
    with irt.Context(np.zeros(0, irt.CELL_DTYPE), 0) as ctx:  # an empty scene: every column is empty
        got = column_latlon(ctx, (lat, lon, rad), "mixed")
        assert (got["count"] == 0).all() and (got["kmax"] == -1).all() and (got["wsum"] == F(CS.MISS)).all()


# ------------------------------------------------------------------ refusals
def test_every_refusal_of_column_latlon_writes_nothing():
    import torch
    cells = S.scene("flat")
    lat, lon, rad = (np.array(a, F) for a in CS.grid("flat", "five"))
    L = irt.lib()
    cols = Columns((lat.size, lon.size))
    out = irt.ColumnOut(**cols.ptrs())

    def call(h, mode=0, lat=lat, nlat=None, lon=lon, nlon=None, rad=rad, n=None, w=None):
        p = lambda a: C.c_void_p(a.ctypes.data) if a is not None else None  # noqa: E731
        w = np.ascontiguousarray(w, F) if w is not None else None
        return L.irt_column_latlon(h, mode, p(lat), lat.size if nlat is None else nlat, p(lon),
                                   lon.size if nlon is None else nlon, p(rad), p(w), rad.size if n is None else n,
                                   out, CS.MISS, None)

    def refused(rc, word):
        assert rc == irt.E_INVALID and word in L.irt_last_error().decode(), L.irt_last_error()

    refused(call(None), "null context")
    with irt.Context(cells, 0) as ctx:
        for mode in MODES.values():
            refused(call(ctx._h, mode=mode), "irt_build_wedge_accel")
        refused(call(ctx._h, mode=7), "sampler mode 7")
        refused(call(ctx._h, nlat=-1), "negative count")
        refused(call(ctx._h, n=-1), "negative count")
        refused(call(ctx._h, nlat=1 << 20, nlon=1 << 20), "2^36")
        refused(call(ctx._h, lat=None, nlat=7), "null lat, lon or radius")
        refused(call(ctx._h, rad=None, n=5), "null lat, lon or radius")
        for bad in (np.nan, np.inf, -np.inf):
            refused(call(ctx._h, w=[1.0, 2.0, bad, 0.0, 1.0]), "weight[2]")
        with pytest.raises(irt.IrtError, match="weights"):
            ctx.column_latlon(lat, lon, rad, cols.ptrs(), [1.0, 2.0])
        with pytest.raises(irt.IrtError, match="unknown outputs"):
            ctx.column_latlon(lat, lon, rad, {"mean": 1})
        ctx.update_values(np.ascontiguousarray(cells["value"]))
        refused(call(ctx._h), "update is pending")
        ctx.end_update()
        torch.cuda.synchronize(0)
        cols.host(written=False)
        assert call(ctx._h, w=[1.0, 2.0, 0.0, -1.0, 1.0]) == 0  # the same call, now valid
        torch.cuda.synchronize(0)
        assert set(cols.host()) == set(CS.OUTPUTS)
    h = C.c_void_p()  # a context still being created; then completed and destroyed as usual
    assert L.irt_create_begin(cells.size, 0, C.byref(h)) == 0
    refused(call(h), "still being created")
    assert L.irt_create_append(h, C.c_void_p(cells.ctypes.data), cells.size) == 0 and L.irt_create_end(h) == 0
    L.irt_destroy(h)


def test_every_refusal_of_render_column_writes_nothing():
    import torch
    W, H = 8, 8
    cells = S.scene("flat")
    lp = LS.launch_params("flat", "outside", "packet")
    good = np.array(CS.levels("flat", "render"), F)
    L = irt.lib()
    frame = Frame(W, H)

    def call(h, lp=lp, w=W, hgt=H, surface=float(CS.surface("flat")), radii=good, n=None, weight=None, product=0,
             fb=True, accum=True):
        r = np.ascontiguousarray(radii, F) if radii is not None else None
        wt = np.ascontiguousarray(weight, F) if weight is not None else None
        return L.irt_render_column(h, C.byref(lp) if lp is not None else None, w, hgt, surface,
                                   C.c_void_p(r.ctypes.data) if r is not None else None,
                                   C.c_void_p(wt.ctypes.data) if wt is not None else None,
                                   len(r) if n is None else n, product,
                                   C.c_void_p(frame.ptr("fb")) if fb else None,
                                   C.c_void_p(frame.ptr("accum")) if accum else None,
                                   C.c_void_p(frame.ptr("value")), CS.MISS, None)

    def refused(rc, word):
        assert rc == irt.E_INVALID and word in L.irt_last_error().decode(), L.irt_last_error()

    refused(call(None), "null context")
    with irt.Context(cells, 0) as ctx:
        refused(call(ctx._h), "no transfer function")
        ctx.set_transfunc(*CS.transfunc("flat"))
        for mode in MODES.values():
            refused(call(ctx._h, lp=LS.launch_params("flat", "outside", "packet", mode=mode)), "irt_build_wedge_accel")
        refused(call(ctx._h, lp=LS.launch_params("flat", "outside", "packet", mode=7)), "sampler mode 7")
        refused(call(ctx._h, n=0), "levels")
        refused(call(ctx._h, n=-1), "levels")
        for r in (0.0, -6.4e6, np.nan, np.inf, -np.inf):
            refused(call(ctx._h, radii=[good[0], r, good[1]]), "radius[1]")
            refused(call(ctx._h, surface=r), "surfaceRadius")
        for bad in (np.nan, np.inf, -np.inf):
            refused(call(ctx._h, radii=good[:3], weight=[1.0, bad, 2.0]), "weight[1]")
        for product in (-1, 3):
            refused(call(ctx._h, product=product), "product")
        for w, h in ((0, 8), (8, 0), (-3, 8), (1 << 14, 1 << 13), (1 << 27, 1)):
            refused(call(ctx._h, w=w, hgt=h), "pixels")
        refused(call(ctx._h, lp=None), "null lp")
        refused(call(ctx._h, radii=None, n=4), "null radius")
        refused(call(ctx._h, fb=False), "null d_fb or d_accum")
        refused(call(ctx._h, accum=False), "null d_fb or d_accum")
        ctx.update_values(np.ascontiguousarray(cells["value"]))
        refused(call(ctx._h), "update is pending")
        ctx.end_update()
        torch.cuda.synchronize(0)
        for which in ("fb", "accum", "value"):
            frame.host(which, written=False)
        assert call(ctx._h, radii=np.tile(good, 10)) == 0  # valid: 120 levels, more than IRT_MAX_LEVELS
        torch.cuda.synchronize(0)
        assert (frame.host("fb") != SENT).all() and (frame.host("value") != SENT).all()


# ------------------------------------------------------------------ time series
def test_columns_follow_value_updates():
    """A pending irt_update_values is refused and leaves the outputs alone; after _end both calls
    answer from the new values."""
    name, key, wname = "flat", "five", "mixed"
    cells = np.array(S.scene(name), copy=True)
    new = np.array(cells, copy=True)
    new["value"] = (1.0 - cells["value"][::-1]) * F(0.75) + F(0.125)
    lat, lon, rad = CS.grid(name, key)
    import oracle as O
    f, v = O.sample_volume(new, irt.latlon_points(lat, lon, rad).reshape(-1, 3), fast=1)
    shape = (rad.size, lat.size, lon.size)
    want = irt.column_reduce(v.reshape(shape), (f != 0).astype(np.uint8).reshape(shape), CS.weights(wname, rad.size),
                             CS.MISS)
    assert CS.same_outputs(want, CS.reduced(name, key, wname)) is not None  # the update is visible
    case = CS.FRAMES[2]
    with make_context(name) as ctx:
        check_columns(column_latlon(ctx, (lat, lon, rad), wname), CS.reduced(name, key, wname), "before the update")
        ctx.update_values(np.ascontiguousarray(new["value"]))
        cols = Columns((lat.size, lon.size))
        with pytest.raises(irt.IrtError, match="update is pending") as e:
            ctx.column_latlon(lat, lon, rad, cols.ptrs())
        assert e.value.code == irt.E_INVALID
        frame = new_frame(case)
        with pytest.raises(irt.IrtError, match="update is pending"):
            render(ctx, frame, case)
        cols.torch.cuda.synchronize(0)
        cols.host(written=False)
        frame.host("fb", written=False)
        ctx.end_update()
        check_columns(column_latlon(ctx, (lat, lon, rad), wname), want, "after the update")
        render(ctx, frame, case)
        assert not np.array_equal(frame.host("value"), CS.bits(CS.expected_frame(*case).value))


# ------------------------------------------------------------------ streams
def test_column_calls_on_a_second_stream_after_a_sampling_call():
    """A long irt_sample_points on one stream, then both column calls on another: they run behind
    it (the shared device table is theirs in call order) and every result is right."""
    import torch
    name, key, wname = "filtered", "all", "mixed"
    pts = S.points(name)
    case = CS.FRAMES[0]
    with make_context(name) as ctx, make_context("flat") as flat:
        s1, s2 = torch.cuda.Stream(0), torch.cuda.Stream(0)
        xyz = torch.from_numpy(np.ascontiguousarray(np.tile(pts, (64, 1)))).to("cuda:0")
        val = torch.zeros(len(xyz), dtype=torch.float32, device="cuda:0")
        torch.cuda.synchronize(0)
        ctx.sample_points(xyz.data_ptr(), len(xyz), val.data_ptr(), 0, irt.MODE_USER_GEOM, CS.MISS, s1.cuda_stream)
        a = column_latlon(ctx, CS.grid(name, key), wname, stream=s2.cuda_stream)
        b = column_latlon(ctx, CS.grid(name, "five"), "none", stream=s1.cuda_stream)  # smaller tables, other stream
        check_columns(a, CS.reduced(name, key, wname), "on the second stream")
        check_columns(b, CS.reduced(name, "five", "none"), "back on the first stream")
        f, v = S.cell_answers(name)
        assert np.array_equal(CS.bits(val.cpu().numpy()[:len(pts)]), CS.bits(np.where(f != 0, v, F(CS.MISS))))
        frame = new_frame(case)
        render(flat, frame, case, stream=s2.cuda_stream)
        check_frame(frame, CS.expected_frame(*case), "a frame on the second stream")


# ------------------------------------------------------------------ rendering is untouched
def test_column_calls_leave_rendering_alone():
    from helpers import FRAMING, GpuFrame
    cells = S.scene("flat")
    setup = irt.setup_frame(cells, 64, 64, camera=FRAMING)
    keys = ("raysLaunched", "raysInBox", "locateCalls", "samplesFound", "candidatesTested")
    case = CS.FRAMES[0]
    with irt.Context(cells, 0) as ctx:
        ctx.set_transfunc(setup.lut, setup.value_range)

        def frame():
            fr = GpuFrame(ctx, 64, 64)
            st = fr.render(setup.lp)
            a, f = fr.host()
            return a.view(np.uint32).copy(), f.copy(), tuple(st.asdict()[k] for k in keys)

        before = frame()
        launches = ctx.stats_total()[1]
        column_latlon(ctx, CS.grid("flat", "all"), "mixed")
        render(ctx, new_frame(case), case)
        assert ctx.stats_total()[1] == launches
        assert tuple(ctx.stats().asdict()[k] for k in keys) == before[2]
        after = frame()
        assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
        assert before[2] == after[2] and before[2][2] > 0
        assert ctx.chain_errors() == 0


# ------------------------------------------------------------------ Context.column
def test_context_column_returns_tensors_on_the_device():
    import torch
    name, key, wname = "terrain", "all", "mixed"
    lat, lon, rad = CS.grid(name, key)
    with irt.Context(S.scene(name), 0) as ctx:
        out = ctx.column(lat, lon, rad, CS.weights(wname, rad.size), miss=CS.MISS)
        assert set(out) == set(CS.OUTPUTS)
        for k, t in out.items():
            assert t.is_cuda and t.shape == (lat.size, lon.size)
            assert t.dtype == (torch.float32 if irt.COLUMN_OUTPUTS[k] is np.float32 else torch.int32)
        check_columns({k: t.cpu().numpy() for k, t in out.items()}, CS.reduced(name, key, wname), "Context.column")
        assert np.isnan(ctx.column(lat, lon, [1.0])["vmax"].cpu().numpy()).all()  # the default miss
