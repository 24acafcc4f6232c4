"""Resampling on the device: irt_sample_points and irt_sample_latlon (csrc/irt_sample.hip) against
the oracle, point by point -- found flags and value bits -- on the inputs tests/test_sample_cpu.py
takes its census of (tests/sample_scenes.py), and for the wedge and triangle samplers on
tests/sampler_scenes.py.  Every output goes to a buffer pre-filled with a sentinel, with guard
words on both sides.  Two NaNs count as equal only in the sampler modes (sampler_scenes.
first_difference), as in tests/test_gpu_samplers.py."""
import ctypes as C

import numpy as np
import pytest

import irt
import oracle as O
import sample_scenes as S
import sampler_scenes as SS

pytestmark = pytest.mark.gpu

GUARD = 96                  # guard elements on each side of an output
SENT_BITS = 0xDEADBEEF      # the float sentinel's bits (a finite negative number)
SENT_BYTE = 0xAB
MISSES = {"finite": -12345.5, "nan": float("nan")}
MODES = {"cubql": irt.MODE_CUBQL, "triangles": irt.MODE_TRIANGLES}


def f32bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def miss_bits(miss):
    return np.uint32(f32bits(np.array([C.c_float(miss).value], np.float32))[0])


class Out:
    """value (float32) and found (uint8) device buffers of n elements between guards."""

    def __init__(self, n, device=0, with_found=True):
        import torch
        self.torch, self.n = torch, n
        dev = f"cuda:{device}"
        sent = int(np.array([SENT_BITS], np.uint32).view(np.int32)[0])
        self.value = torch.full((n + 2 * GUARD,), sent, dtype=torch.int32, device=dev)
        self.found = torch.full((n + 2 * GUARD,), SENT_BYTE, dtype=torch.uint8, device=dev) if with_found else None

    @property
    def value_ptr(self):
        return self.value.data_ptr() + 4 * GUARD

    @property
    def found_ptr(self):
        return self.found.data_ptr() + GUARD if self.found is not None else 0

    def host(self, written=True):
        """(found or None, value) of the n elements, after checking the guards (written=False: and
        that the n elements still hold the sentinel)."""
        v = self.value.cpu().numpy().view(np.uint32)
        assert (v[:GUARD] == SENT_BITS).all() and (v[GUARD + self.n:] == SENT_BITS).all(), "value guards"
        f = None
        if self.found is not None:
            f = self.found.cpu().numpy()
            assert (f[:GUARD] == SENT_BYTE).all() and (f[GUARD + self.n:] == SENT_BYTE).all(), "found guards"
            f = f[GUARD:GUARD + self.n]
            assert written or (f == SENT_BYTE).all()
            assert not written or np.isin(f, (0, 1)).all()
        v = v[GUARD:GUARD + self.n]
        assert written or (v == SENT_BITS).all()
        return f, v.view(np.float32)


def sample_points(ctx, pts, mode=irt.MODE_USER_GEOM, miss=float("nan"), with_found=True, stream=0):
    import torch
    pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 3)
    xyz = torch.from_numpy(pts.copy()).to(f"cuda:{ctx.device}")
    out = Out(len(pts), ctx.device, with_found)
    ctx.sample_points(xyz.data_ptr(), len(pts), out.value_ptr, out.found_ptr, mode, miss, stream)
    torch.cuda.synchronize(ctx.device)
    return out.host()


def sample_latlon(ctx, grid, mode=irt.MODE_USER_GEOM, miss=float("nan"), stream=0):
    import torch
    lat, lon, rad = grid
    out = Out(rad.size * lat.size * lon.size, ctx.device)
    assert ctx.sample_latlon(lat, lon, rad, out.value_ptr, out.found_ptr, mode, miss, stream) == \
        (rad.size, lat.size, lon.size)
    torch.cuda.synchronize(ctx.device)
    return out.host()


def check_cell(got, want, miss, what):
    """got (found, value) from the device; want (found, value) from the oracle: flags equal, the
    found values equal as bits, the misses holding `miss`'s bits."""
    gf, gv = got
    wf, wv = want
    hit = np.asarray(wf) != 0
    expect = np.where(hit, f32bits(wv), miss_bits(miss))
    if gf is not None:
        k = np.flatnonzero((gf != 0) != hit)
        assert k.size == 0, f"{what}: found differs at {k[:5]} of {len(hit)}"
    k = np.flatnonzero(f32bits(gv) != expect)
    assert k.size == 0, (f"{what}: {k.size} of {len(hit)} values differ; first {k[0]}: "
                         f"{hex(f32bits(gv)[k[0]])} vs {hex(expect[k[0]])}")


def check_sampler(name, got, want, miss, what):
    """The sampler modes' bar: found flags equal, found values equal as bits or both NaN; misses
    hold `miss`."""
    gf, gv = got
    assert SS.first_difference(gf, gv, want[0], want[1]) < 0, \
        f"{what} on {name}: first difference at {SS.first_difference(gf, gv, want[0], want[1])}"
    missed = np.asarray(want[0]) == 0
    assert (f32bits(gv)[missed] == miss_bits(miss)).all(), f"{what} on {name}: a miss without missValue"


# ------------------------------------------------------------------ the cell sampler
@pytest.mark.parametrize("miss", list(MISSES))
@pytest.mark.parametrize("slots", [False, True], ids=["headers", "slots"])
@pytest.mark.parametrize("name", S.SCENE_NAMES)
def test_cell_sampler_points(monkeypatch, name, slots, miss):
    """Every point of sample_scenes.points -- locator_points, then the guard points -- through
    irt_sample_points from headers and (IRT_SLOTS=1) from the slot table, where the scene has one
    (the terrain scene's cells have more than three edges: no table, the header form again)."""
    if slots:
        monkeypatch.setenv("IRT_SLOTS", "1")
    pts, want = S.points(name), S.cell_answers(name)
    with irt.Context(S.scene(name), 0) as ctx:
        assert (ctx.array_bytes("slots") > 0) == (slots and name != "terrain")
        got = sample_points(ctx, pts, miss=MISSES[miss])
        print(f"{name}: {len(pts)} points, device found {int(got[0].sum())}, oracle {int(want[0].sum())}")
        check_cell(got, want, MISSES[miss], f"irt_sample_points {name}")
        assert not got[0][-len(S.GUARD_POINTS):].any()  # the guard's defined result
        if miss == "finite":  # the edges of a wave and of four: prefixes of the points
            for n in (1, 63, 64, 65, 255, 257):
                check_cell(sample_points(ctx, pts[:n], miss=MISSES[miss]), (want[0][:n], want[1][:n]),
                           MISSES[miss], f"irt_sample_points {name} first {n}")
        else:  # d_found == NULL: the values alone
            got = sample_points(ctx, pts, miss=MISSES[miss], with_found=False)
            assert got[0] is None
            check_cell(got, want, MISSES[miss], f"irt_sample_points {name} without d_found")


# ------------------------------------------------------------------ wedge and triangle samplers
@pytest.fixture(scope="module")
def sampler_contexts():
    made = {}

    def get(name):
        if name not in made:
            cells = SS.scene(name)
            made[name] = irt.Context(cells, 0)
            made[name].build_wedge_accel(cells)
        return made[name]

    yield get
    for ctx in made.values():
        ctx.close()


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", SS.SCENE_NAMES)
def test_unstructured_samplers_points(name, mode, sampler_contexts):
    ps = SS.points(name)
    want = SS.oracle_answers(name)[0 if mode == "cubql" else 1]
    miss = MISSES["finite"] if mode == "cubql" else MISSES["nan"]
    got = sample_points(sampler_contexts(name), ps.points, MODES[mode], miss)
    print(f"{name} {mode}: {len(ps.points)} points, device found {int(got[0].sum())}, oracle {int(want[0].sum())}")
    check_sampler(name, got, want, miss, f"irt_sample_points {mode}")
    # and the guard points: misses, whatever the sampler
    got = sample_points(sampler_contexts(name), S.GUARD_POINTS, MODES[mode], miss)
    assert not got[0].any() and (f32bits(got[1]) == miss_bits(miss)).all()


@pytest.mark.parametrize("mode", list(MODES))
def test_unstructured_samplers_latlon(mode, sampler_contexts):
    """irt_sample_latlon through the samplers' kernel: equal to irt_sample_points on
    irt_latlon_points, and to the oracle's scan there."""
    name = "filtered"
    cells = SS.scene(name)
    h0, top, inner = S.shell(cells)
    lat = np.linspace(-0.6, 1.1, 17).astype(np.float32)
    lon = np.linspace(-1.7, 0.9, 33).astype(np.float32)
    rad = np.array([inner, h0, np.float32(top + 300.0)], np.float32)
    pts = irt.latlon_points(lat, lon, rad).reshape(-1, 3)
    entry = O.wedge_sample_points if mode == "cubql" else O.triangle_sample_points
    want = entry(cells, pts)
    assert 0 < want[0].sum() < len(pts)
    ctx = sampler_contexts(name)
    miss = MISSES["finite"]
    a = sample_latlon(ctx, (lat, lon, rad), MODES[mode], miss)
    b = sample_points(ctx, pts, MODES[mode], miss)
    check_sampler(name, a, want, miss, f"irt_sample_latlon {mode}")
    check_sampler(name, b, want, miss, f"irt_sample_points {mode} on the grid's points")
    assert np.array_equal(a[0], b[0]) and SS.first_difference(a[0], a[1], b[0], b[1]) < 0


def test_sampler_modes_need_the_wedge_accel():
    cells = SS.scene("single")
    pts = SS.points("single").points[:8]
    one = np.zeros(1, np.float32)
    with irt.Context(cells, 0) as ctx:
        out = Out(len(pts))
        import torch
        xyz = torch.from_numpy(np.array(pts, np.float32)).to("cuda:0")
        for mode in MODES.values():
            with pytest.raises(irt.IrtError, match="irt_build_wedge_accel") as e:
                ctx.sample_points(xyz.data_ptr(), len(pts), out.value_ptr, out.found_ptr, mode)
            assert e.value.code == -1
            with pytest.raises(irt.IrtError, match="irt_build_wedge_accel"):
                ctx.sample_latlon(one, one, one, out.value_ptr, out.found_ptr, mode)
        with pytest.raises(irt.IrtError, match="sampler mode 7"):
            ctx.sample_points(xyz.data_ptr(), len(pts), out.value_ptr, out.found_ptr, 7)
        with pytest.raises(irt.IrtError, match="null d_xyz or d_value"):
            ctx.sample_points(0, len(pts), out.value_ptr, out.found_ptr)
        with pytest.raises(irt.IrtError, match="null d_xyz or d_value"):
            ctx.sample_points(xyz.data_ptr(), len(pts), 0, out.found_ptr)
        with pytest.raises(irt.IrtError, match="2\\^36"):
            ctx.sample_points(xyz.data_ptr(), (1 << 36) + 1, out.value_ptr, out.found_ptr)
        with pytest.raises(irt.IrtError, match="2\\^36"):  # a negative count, as size_t
            lib = irt.lib()
            irt._check(lib.irt_sample_points(ctx._h, 0, C.c_void_p(xyz.data_ptr()), C.c_size_t(-1 & (2 ** 64 - 1)),
                                             C.c_void_p(out.value_ptr), None, 0.0, None), "irt_sample_points")
        torch.cuda.synchronize(0)
        out.host(written=False)


# ------------------------------------------------------------------ lat/lon grids
@pytest.mark.parametrize("slots", [False, True], ids=["headers", "slots"])
@pytest.mark.parametrize("name", ["flat", "filtered"])
def test_latlon_grids(monkeypatch, name, slots):
    """irt_sample_latlon on the five grids == irt_sample_points on irt_latlon_points == the oracle
    there (grids of 1 x 1, 7 x 9, 8 x 8, 17 x 33 and 64 x 128 points a level: patches cut by both
    edges, one whole patch, many patches)."""
    if slots:
        monkeypatch.setenv("IRT_SLOTS", "1")
    miss = MISSES["nan"] if slots else MISSES["finite"]
    with irt.Context(S.scene(name), 0) as ctx:
        assert (ctx.array_bytes("slots") > 0) == slots
        for shape in S.GRID_SHAPES:
            want = S.grid_answers(name, shape)
            a = sample_latlon(ctx, S.grid(name, shape), miss=miss)
            b = sample_points(ctx, S.grid_points(name, shape), miss=miss)
            print(f"{name} {shape}: device found {int(a[0].sum())} of {a[0].size}, oracle {int(want[0].sum())}")
            check_cell(a, want, miss, f"irt_sample_latlon {name} {shape}")
            check_cell(b, want, miss, f"irt_sample_points on irt_latlon_points {name} {shape}")
            assert np.array_equal(a[0], b[0]) and np.array_equal(f32bits(a[1]), f32bits(b[1]))


# ------------------------------------------------------------------ time series
def test_sampling_follows_value_updates():
    """After update_values + end_update both calls answer from the new values; while the update is
    pending they return IRT_E_INVALID and leave their outputs alone."""
    import torch
    cells = np.array(S.scene("flat"), copy=True)
    pts = S.points("flat")
    shape = (2, 7, 9)
    grid = S.grid("flat", shape)
    new = np.array(cells, copy=True)
    new["value"] = (1.0 - cells["value"][::-1]) * np.float32(0.75) + np.float32(0.125)
    n_oracle = len(pts) - 2
    want_pts = [np.concatenate([a, np.zeros(2, a.dtype)]) for a in O.sample_volume(new, pts[:n_oracle], fast=1)]
    want_grid = O.sample_volume(new, S.grid_points("flat", shape).reshape(-1, 3), fast=1)
    old = S.cell_answers("flat")
    assert S.same_bits(old[0], old[1], want_pts[0], want_pts[1]) >= 0  # the update is visible
    miss = MISSES["finite"]
    with irt.Context(cells, 0) as ctx:
        check_cell(sample_points(ctx, pts, miss=miss), old, miss, "before the update")
        ctx.update_values(np.ascontiguousarray(new["value"]))
        xyz = torch.from_numpy(np.array(pts, np.float32)).to("cuda:0")
        out = Out(len(pts))
        with pytest.raises(irt.IrtError, match="update is pending") as e:
            ctx.sample_points(xyz.data_ptr(), len(pts), out.value_ptr, out.found_ptr)
        assert e.value.code == -1
        with pytest.raises(irt.IrtError, match="update is pending"):
            ctx.sample_latlon(*grid, out.value_ptr, out.found_ptr)
        torch.cuda.synchronize(0)
        out.host(written=False)
        ctx.end_update()
        check_cell(sample_points(ctx, pts, miss=miss), want_pts, miss, "irt_sample_points after the update")
        check_cell(sample_latlon(ctx, grid, miss=miss), want_grid, miss, "irt_sample_latlon after the update")
        # the device-pointer form, sampled on the stream that carried the update
        d_old = torch.from_numpy(np.ascontiguousarray(cells["value"])).to("cuda:0")
        s = torch.cuda.current_stream(0).cuda_stream
        ctx.update_values_device(d_old.data_ptr(), cells.size, 0, s)
        ctx.end_update()
        check_cell(sample_points(ctx, pts, miss=miss, stream=s), old, miss, "after irt_update_values_device")


# ------------------------------------------------------------------ streams
@pytest.mark.parametrize("where", ["side", "null"])
def test_sampling_on_the_callers_stream(where):
    """Points produced by a torch op on a stream, sampled on that stream, read after its
    synchronize(): a side stream, and the null stream next to torch's default stream."""
    import torch
    pts, want = S.points("filtered"), S.cell_answers("filtered")
    host = torch.from_numpy(np.ascontiguousarray(pts) * np.float32(0.5)).pin_memory()
    miss = MISSES["finite"]
    with irt.Context(S.scene("filtered"), 0) as ctx:
        out = Out(len(pts))
        stream = torch.cuda.Stream(0) if where == "side" else torch.cuda.default_stream(0)
        with torch.cuda.stream(stream):
            big = torch.randn(1 << 24, device="cuda:0")  # work ahead of the points on that stream
            big = (big * big).sum()
            xyz = host.to("cuda:0", non_blocking=True) * 2.0  # exact: the points, made on the stream
            ctx.sample_points(xyz.data_ptr(), len(pts), out.value_ptr, out.found_ptr, irt.MODE_USER_GEOM, miss,
                              stream.cuda_stream if where == "side" else 0)
        stream.synchronize()
        check_cell(out.host(), want, miss, f"irt_sample_points on the {where} stream")
        assert float(big) > 0


# ------------------------------------------------------------------ rendering is untouched
def test_sampling_leaves_rendering_alone():
    """A 64 x 64 frame and its statistics (the counts; kernelMs is a measured time) before and after
    a batch of sampling calls are identical, and the calls are no launches of the statistics."""
    from helpers import FRAMING, GpuFrame
    cells = S.scene("flat")
    setup = irt.setup_frame(cells, 64, 64, camera=FRAMING)
    with irt.Context(cells, 0) as ctx:
        ctx.set_transfunc(setup.lut, setup.value_range)

        def frame():
            fr = GpuFrame(ctx, 64, 64)
            st = fr.render(setup.lp)
            a, f = fr.host()
            return a.view(np.uint32).copy(), f.copy(), tuple(st.asdict()[k] for k in
                                                             ("raysLaunched", "raysInBox", "locateCalls",
                                                              "samplesFound", "candidatesTested"))

        before = frame()
        launches = ctx.stats_total()[1]
        for shape in S.GRID_SHAPES[:4]:
            sample_latlon(ctx, S.grid("flat", shape))
        check_cell(sample_points(ctx, S.points("flat")), S.cell_answers("flat"), float("nan"), "between frames")
        assert ctx.stats_total()[1] == launches
        assert tuple(ctx.stats().asdict()[k] for k in ("raysLaunched", "locateCalls")) == (before[2][0], before[2][2])
        after = frame()
        assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
        assert before[2] == after[2] and before[2][2] > 0
        assert ctx.chain_errors() == 0


# ------------------------------------------------------------------ empty and zero
def test_empty_scene_and_zero_points():
    import torch
    pts = S.points("flat")[:300]
    with irt.Context(np.zeros(0, irt.CELL_DTYPE), 0) as ctx:
        f, v = sample_points(ctx, pts, miss=MISSES["finite"])
        assert not f.any() and (f32bits(v) == miss_bits(MISSES["finite"])).all()
        f, v = sample_latlon(ctx, S.grid("flat", (2, 7, 9)))
        assert not f.any() and np.isnan(v).all()
    with irt.Context(S.scene("filtered"), 0) as ctx:
        out = Out(16)
        xyz = torch.from_numpy(np.array(pts, np.float32)).to("cuda:0")
        ctx.sample_points(xyz.data_ptr(), 0, out.value_ptr, out.found_ptr)
        ctx.sample_points(0, 0, 0, 0)
        none = np.zeros(0, np.float32)
        lat, lon, rad = S.grid("filtered", (2, 7, 9))
        for g in ((none, lon, rad), (lat, none, rad), (lat, lon, none)):
            assert 0 in ctx.sample_latlon(*g, out.value_ptr, out.found_ptr)
        torch.cuda.synchronize(0)
        out.host(written=False)


# ------------------------------------------------------------------ Context.resample
def test_resample_tensor_and_array():
    import torch
    pts, want = S.points("terrain"), S.cell_answers("terrain")
    with irt.Context(S.scene("terrain"), 0) as ctx:
        v_np, f_np = ctx.resample(pts, miss=-1.0)
        assert isinstance(v_np, np.ndarray) and v_np.dtype == np.float32 and f_np.dtype == bool
        check_cell((f_np, v_np), want, -1.0, "Context.resample(numpy)")
        t = torch.from_numpy(np.ascontiguousarray(pts)).to("cuda:0").reshape(5, -1, 3)
        v_t, f_t = ctx.resample(t, miss=-1.0)
        assert v_t.is_cuda and v_t.shape == t.shape[:-1] and f_t.dtype == torch.bool
        assert np.array_equal(f_t.cpu().numpy().reshape(-1), f_np)
        assert np.array_equal(f32bits(v_t.cpu().numpy().reshape(-1)), f32bits(v_np))
        with pytest.raises(irt.IrtError, match="float32"):
            ctx.resample(t.double())
