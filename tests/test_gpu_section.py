"""irt_section on the device (csrc/irt_section.hip), bit for bit: value and found against the oracle
samplers and against the device's own irt_sample_points on irt_section_points' output, the column
outputs against irt_column_reduce of those values, the curtain against the restatement of its
definition (tests/section_scenes.py), on the inputs tests/test_section_cpu.py takes its census of;
then the call's conduct.  Every output goes to a buffer pre-filled with a sentinel, with guard
words on both sides."""
import ctypes as C

import numpy as np
import pytest

import column_scenes as CS
import irt
import levels_scenes as LS
import sample_scenes as S
import section_scenes as SS
from test_gpu_levels import SENT
from test_gpu_sample import sample_latlon, sample_points

pytestmark = pytest.mark.gpu

GUARD = 96
F = np.float32
MODES = {"cubql": irt.MODE_CUBQL, "triangles": irt.MODE_TRIANGLES}
POINT_OUTPUTS = tuple(irt.SECTION_OUTPUTS)          # value, found, rgba
ALL_OUTPUTS = POINT_OUTPUTS + tuple(CS.OUTPUTS)     # ... and the six column outputs
NO_RGBA = tuple(k for k in ALL_OUTPUTS if k != "rgba")
SENT_BYTE = 0xA5


class Section:
    """The nine outputs of a levels x columns section as device buffers between guards,
    sentinel-filled; `which`: the outputs handed to the call (the others stay NULL)."""

    def __init__(self, levels, columns, which=ALL_OUTPUTS, device=0):
        import torch
        self.torch, self.L, self.n, self.which = torch, int(levels), int(columns), tuple(which)
        dev = f"cuda:{device}"
        self.buf = {}
        for k in ALL_OUTPUTS:
            size = (self.L * self.n if k in POINT_OUTPUTS else self.n) + 2 * GUARD
            if k == "found":
                self.buf[k] = torch.full((size,), SENT_BYTE, dtype=torch.uint8, device=dev)
            else:
                self.buf[k] = torch.full((size,), SENT, dtype=torch.int32, device=dev)

    def ptrs(self):
        return {k: self.buf[k].data_ptr() + GUARD * (1 if k == "found" else 4) for k in self.which}

    def host(self, written=True):
        """The outputs as a dict of arrays -- (levels, columns) or (columns,) -- after checking the
        guards, and that an output not handed over (or, written=False, any output) still holds the
        sentinel."""
        out = {}
        for k, t in self.buf.items():
            sent = SENT_BYTE if k == "found" else SENT
            v = t.cpu().numpy()
            v = v if k == "found" else v.view(np.uint32)
            size = self.L * self.n if k in POINT_OUTPUTS else self.n
            assert (v[:GUARD] == sent).all() and (v[GUARD + size:] == sent).all(), f"{k} guards"
            v = v[GUARD:GUARD + size]
            if not written or k not in self.which:
                assert (v == sent).all(), f"{k} was written"
            elif k in POINT_OUTPUTS:
                out[k] = v.view(irt.SECTION_OUTPUTS[k]).reshape(self.L, self.n)
            else:
                out[k] = v.view(irt.COLUMN_OUTPUTS[k])
        return out


def section(ctx, cols, rad, wname="none", mode=irt.MODE_USER_GEOM, miss=SS.MISS, which=NO_RGBA, ambient=SS.AMBIENT,
            stream=0):
    lat, lon = cols
    sec = Section(rad.size, lat.size, which, ctx.device)
    assert ctx.section_raw(lat, lon, rad, sec.ptrs(), SS.weights(wname, rad.size), ambient[0], ambient[1], mode, miss,
                           stream) == (rad.size, lat.size)
    sec.torch.cuda.synchronize(ctx.device)
    return sec.host()


def check_points(got, want_f, want_v, miss, what):
    """found equal, every value equal as bits, the misses holding `miss`'s bits."""
    expect = np.where(np.asarray(want_f) != 0, np.asarray(want_v, F), F(miss)).astype(F)
    k = S.same_bits(got["found"], got["value"], want_f, expect)
    assert k < 0, (f"{what}: value or found differs, first at flat index {k} of {expect.size}: "
                   f"{got['value'].reshape(-1)[k]!r}/{got['found'].reshape(-1)[k]} vs "
                   f"{expect.reshape(-1)[k]!r}/{np.asarray(want_f).reshape(-1)[k]}")
    assert set(np.unique(got["found"])) <= {0, 1}


def check_columns(got, want, what, which=CS.OUTPUTS):
    k = CS.same_outputs(got, want, which)
    if k is not None:
        bad = np.flatnonzero(CS.bits(got[k]) != CS.bits(want[k]))
        raise AssertionError(f"{what}: {k} differs in {len(bad)} of {got[k].size} columns, first {bad[0]}: "
                             f"{got[k][bad[0]]!r} vs {want[k][bad[0]]!r}")


def two_pass(ctx, cols, rad, wname, mode=irt.MODE_USER_GEOM, miss=SS.MISS):
    """The device's own irt_sample_points on irt_section_points' output, and irt_column_reduce of it:
    the header's two promises."""
    pts = irt.section_points(cols[0], cols[1], rad)
    f, v = sample_points(ctx, pts, mode, miss)
    shape = pts.shape[:2]
    f, v = f.reshape(shape), v.reshape(shape)
    return f, v, irt.column_reduce(v, f, SS.weights(wname, rad.size), miss)


# ------------------------------------------------------------------ the cell sampler
@pytest.mark.parametrize("slots", [False, True], ids=["headers", "slots"])
@pytest.mark.parametrize("name", SS.SCENE_NAMES)
def test_section_equals_the_oracle_and_sample_points(monkeypatch, name, slots):
    """Every track and station list (1, 41, 63, 64, 65 and 130 columns) x three weight sets per
    scene, from headers and (IRT_SLOTS=1) from the slot table where the scene has one: value and
    found equal the oracle's point by point and the device's own irt_sample_points on
    irt_section_points' output; the column outputs equal irt_column_reduce of them."""
    if slots:
        monkeypatch.setenv("IRT_SLOTS", "1")
    rad = SS.levels(name)
    with irt.Context(S.scene(name), 0) as ctx:
        assert (ctx.array_bytes("slots") > 0) == (slots and name != "terrain")
        for key in SS.SETS:
            cols = SS.columns(key)
            wf, wv = SS.answers(name, key)
            df, dv, _ = two_pass(ctx, cols, rad, "none")
            print(f"{name} {key}: {int(wf.sum())} of {wf.size} points found, "
                  f"{int((wf.sum(1) == 0).sum())} levels without one")
            for wname in SS.WEIGHTS:
                got = section(ctx, cols, rad, wname)
                what = f"irt_section {name} {key} {wname}"
                check_points(got, wf, wv, SS.MISS, what + " against the oracle")
                check_points(got, df, dv, SS.MISS, what + " against irt_sample_points")
                check_columns(got, SS.reduced(name, key, wname), what + " against irt_column_reduce")
        # a NaN missValue, and the ascending order of the same levels
        got = section(ctx, SS.columns("stations"), rad, "mixed", miss=float("nan"))
        check_points(got, *SS.answers(name, "stations"), float("nan"), f"{name}: NaN missValue")
        check_columns(got, SS.reduced(name, "stations", "mixed", miss=float("nan")), f"{name}: NaN missValue")
        if name == "filtered":
            assert np.isnan(got["value"]).any() and np.isnan(got["wsum"]).any()
        asc = SS.levels(name, "ascending")
        got = section(ctx, SS.columns("pole"), asc, "none")
        check_points(got, *SS.answers(name, "pole", "ascending"), SS.MISS, f"{name}: ascending levels")
        check_columns(got, SS.reduced(name, "pole", "none", "ascending"), f"{name}: ascending levels")


# ------------------------------------------------------------------ wedge and triangle samplers
@pytest.mark.parametrize("mode", list(MODES))
def test_section_of_the_unstructured_samplers(mode):
    """On the flat scene: value and found against the mode's oracle sampler (found flags equal, found
    values equal as bits) and, bit for bit, against the device's own irt_sample_points; the columns
    against irt_column_reduce."""
    cells = S.scene("flat")
    rad = SS.levels("flat")
    with irt.Context(cells, 0) as ctx:
        ctx.build_wedge_accel(cells)
        for key in ("oblique", "stations"):
            for wname in ("none", "mixed"):
                got = section(ctx, SS.columns(key), rad, wname, MODES[mode])
                what = f"irt_section {mode} flat {key} {wname}"
                wf, wv = SS.answers("flat", key, "shuffled", MODES[mode])
                assert not np.isnan(wv[wf != 0]).any()
                check_points(got, wf, wv, SS.MISS, what + " against the oracle")
                df, dv, dcol = two_pass(ctx, SS.columns(key), rad, wname, MODES[mode])
                check_points(got, df, dv, SS.MISS, what + " against irt_sample_points")
                check_columns(got, dcol, what)
                check_columns(got, SS.reduced("flat", key, wname, "shuffled", MODES[mode]), what + " (oracle)")


# ------------------------------------------------------------------ the curtain
def make_context(name, tf_name, mode=irt.MODE_USER_GEOM):
    cells = S.scene(name)
    ctx = irt.Context(cells, 0)
    ctx.set_transfunc(*LS.transfunc(name, tf_name))
    if mode != irt.MODE_USER_GEOM:
        ctx.build_wedge_accel(cells)
    return ctx


@pytest.mark.parametrize("case", SS.CURTAINS, ids="-".join)
def test_curtain_equals_the_restatement(case):
    """rgba against pixels(classify(...)) of the oracle's values with a non-unit ambient, together
    with every other output; and with unit ambient terms."""
    name, key, tf_name = case
    rad = SS.levels(name)
    with make_context(name, tf_name) as ctx:
        got = section(ctx, SS.columns(key), rad, "mixed", which=ALL_OUTPUTS)
        want = SS.curtain(name, key, tf_name)
        bad = np.argwhere(got["rgba"] != want)
        print(f"{case}: {np.unique(want[want != 0]).size} distinct non-zero pixels of {want.size}")
        assert len(bad) == 0, (f"{case}: rgba differs at {len(bad)} of {want.size} points, first {tuple(bad[0])}: "
                               f"{hex(int(got['rgba'][tuple(bad[0])]))} vs {hex(int(want[tuple(bad[0])]))}")
        check_points(got, *SS.answers(name, key), SS.MISS, f"{case}: with rgba")
        check_columns(got, SS.reduced(name, key, "mixed"), f"{case}: with rgba")
        unit = ((1.0, 1.0, 1.0), 1.0)
        got = section(ctx, SS.columns(key), rad, which=("rgba",), ambient=unit)
        f, v = SS.answers(name, key)
        assert np.array_equal(got["rgba"], SS.curtain_of(LS.transfunc(name, tf_name), f, v, unit))


def test_curtain_of_the_wedge_sampler():
    name, key, tf_name = "flat", "oblique", "translucent"
    with make_context(name, tf_name, irt.MODE_CUBQL) as ctx:
        got = section(ctx, SS.columns(key), SS.levels(name), mode=irt.MODE_CUBQL, which=("rgba", "found"))
        f, v = SS.answers(name, key, "shuffled", irt.MODE_CUBQL)
        assert np.array_equal(got["found"], f)
        assert np.array_equal(got["rgba"], SS.curtain_of(LS.transfunc(name, tf_name), f, v))


# ------------------------------------------------------------------ NULL outputs
def test_each_output_alone_is_the_same_output():
    name, key, wname = "terrain", "equator", "mixed"
    rad = SS.levels(name)
    with make_context(name, "translucent") as ctx:
        full = section(ctx, SS.columns(key), rad, wname, which=ALL_OUTPUTS)
        for k in ALL_OUTPUTS:
            one = section(ctx, SS.columns(key), rad, wname, which=(k,))  # (host() checks the others' sentinels)
            assert set(one) == {k} and np.array_equal(one[k].view(np.uint8), full[k].view(np.uint8)), k
        for which in (("found", "kmin"), ("value", "rgba", "count"), ("wsum", "vmax", "vmin", "kmax")):
            some = section(ctx, SS.columns(key), rad, wname, which=which)
            assert all(np.array_equal(some[k].view(np.uint8), full[k].view(np.uint8)) for k in which), which


def test_sections_without_points_or_outputs_launch_nothing():
    lat, lon = SS.columns("stations")
    rad = SS.levels("flat")
    none = np.zeros(0, F)
    with irt.Context(S.scene("flat"), 0) as ctx:
        sec = Section(rad.size, lat.size, NO_RGBA)
        assert ctx.section_raw(none, none, rad, sec.ptrs()) == (rad.size, 0)
        assert ctx.section_raw(lat, lon, none, sec.ptrs()) == (0, lat.size)
        ctx.section_raw(lat, lon, rad, {})  # every pointer NULL: IRT_OK, nothing launched
        ctx.section_raw(lat, lon, rad, {"value": 0, "count": 0})
        sec.torch.cuda.synchronize(0)
        sec.host(written=False)
    with irt.Context(np.zeros(0, irt.CELL_DTYPE), 0) as ctx:  # an empty scene: every point is a miss
        got = section(ctx, (lat, lon), rad, "mixed")
        assert not got["found"].any() and (got["value"] == F(SS.MISS)).all()
        assert (got["count"] == 0).all() and (got["kmax"] == -1).all() and (got["wsum"] == F(SS.MISS)).all()


# ------------------------------------------------------------------ pairs that form a grid
@pytest.mark.parametrize("name", SS.SCENE_NAMES)
def test_a_grids_pairs_equal_the_grid_calls(name):
    lat, lon, rad, plat, plon = SS.grid_pairs(name)
    from test_gpu_column import column_latlon
    with irt.Context(S.scene(name), 0) as ctx:
        got = section(ctx, (plat, plon), rad, "mixed")
        f, v = sample_latlon(ctx, (lat, lon, rad), miss=SS.MISS)
        check_points(got, f.reshape(got["found"].shape), v.reshape(got["value"].shape), SS.MISS,
                     f"{name}: against irt_sample_latlon")
        grid = column_latlon(ctx, (lat, lon, rad), "mixed", miss=SS.MISS)
        check_columns(got, {k: a.reshape(-1) for k, a in grid.items()}, f"{name}: against irt_column_latlon")
        check_columns(got, {k: a.reshape(-1) for k, a in CS.reduced(name, "five", "mixed").items()},
                      f"{name}: against the oracle's grid")


# ------------------------------------------------------------------ refusals
def test_every_refusal_writes_nothing():
    import torch
    cells = S.scene("flat")
    lat, lon = (np.array(a, F) for a in SS.columns("stations"))
    rad = np.array(SS.levels("flat")[:5], F)
    L = irt.lib()
    sec = Section(rad.size, lat.size)
    ptrs = sec.ptrs()
    full = irt.SectionOut(column=irt.ColumnOut(**{k: ptrs[k] for k in CS.OUTPUTS}),
                          **{k: ptrs[k] for k in POINT_OUTPUTS})
    no_rgba = irt.SectionOut(column=irt.ColumnOut(**{k: ptrs[k] for k in CS.OUTPUTS}), value=ptrs["value"],
                             found=ptrs["found"])

    def call(h, mode=0, lat=lat, lon=lon, n=None, rad=rad, levels=None, w=None, amb=(1.0, 1.0, 1.0), radiance=1.0,
             out=no_rgba):
        p = lambda a: C.c_void_p(a.ctypes.data) if a is not None else None  # noqa: E731
        w = np.ascontiguousarray(w, F) if w is not None else None
        return L.irt_section(h, mode, p(lat), p(lon), lat.size if n is None else n, p(rad), p(w),
                             rad.size if levels is None else levels, irt.vec3(amb), radiance, out, SS.MISS, None)

    def refused(rc, word):
        assert rc == irt.E_INVALID and word in L.irt_last_error().decode(), L.irt_last_error()

    refused(call(None), "null context")
    with irt.Context(cells, 0) as ctx:
        for mode in MODES.values():
            refused(call(ctx._h, mode=mode), "irt_build_wedge_accel")
        refused(call(ctx._h, mode=7), "sampler mode 7")
        refused(call(ctx._h, n=-1), "negative count")
        refused(call(ctx._h, levels=-1), "negative count")
        refused(call(ctx._h, n=1 << 30, levels=1 << 30), "2^36")
        refused(call(ctx._h, lat=None, n=41), "null lat, lon or radius")
        refused(call(ctx._h, lon=None, n=41), "null lat, lon or radius")
        refused(call(ctx._h, rad=None, levels=5), "null lat, lon or radius")
        for bad in (np.nan, np.inf, -np.inf):
            refused(call(ctx._h, w=[1.0, 2.0, bad, 0.0, 1.0]), "weight[2]")
        refused(call(ctx._h, out=full), "no transfer function")
        ctx.set_transfunc(*LS.transfunc("flat", "default"))
        for bad in (np.nan, np.inf, -np.inf):
            refused(call(ctx._h, out=full, amb=(1.0, bad, 1.0)), "non-finite ambientColor or ambientRadiance")
            refused(call(ctx._h, out=full, radiance=bad), "non-finite ambientColor or ambientRadiance")
        with pytest.raises(irt.IrtError, match="weights"):
            ctx.section_raw(lat, lon, rad, ptrs, [1.0, 2.0])
        with pytest.raises(irt.IrtError, match="unknown outputs"):
            ctx.section_raw(lat, lon, rad, {"mean": 1})
        with pytest.raises(irt.IrtError, match="pairs"):
            ctx.section_raw(lat, lon[:3], rad, ptrs)
        ctx.update_values(np.ascontiguousarray(cells["value"]))
        refused(call(ctx._h), "update is pending")
        ctx.end_update()
        torch.cuda.synchronize(0)
        sec.host(written=False)
        # the same calls, now valid: a non-finite ambient is not looked at without rgba
        assert call(ctx._h, amb=(np.nan, 1.0, 1.0), radiance=np.inf, w=[1.0, 2.0, 0.0, -1.0, 1.0]) == 0
        assert call(ctx._h, out=full) == 0
        torch.cuda.synchronize(0)
        assert set(sec.host()) == set(ALL_OUTPUTS)
    h = C.c_void_p()  # a context still being created; then completed and destroyed as usual
    assert L.irt_create_begin(cells.size, 0, C.byref(h)) == 0
    refused(call(h), "still being created")
    assert L.irt_create_append(h, C.c_void_p(cells.ctypes.data), cells.size) == 0 and L.irt_create_end(h) == 0
    L.irt_destroy(h)


# ------------------------------------------------------------------ time series
def test_sections_follow_value_updates():
    """A pending irt_update_values refuses the call and leaves the outputs alone; after _end the
    new values show."""
    name, key, wname = "flat", "stations", "mixed"
    cells = np.array(S.scene(name), copy=True)
    new = np.array(cells, copy=True)
    new["value"] = (1.0 - cells["value"][::-1]) * F(0.75) + F(0.125)
    cols, rad = SS.columns(key), SS.levels(name)
    pts = irt.section_points(cols[0], cols[1], rad)
    f, v = LS.sample(new, irt.MODE_USER_GEOM, pts.reshape(-1, 3))
    f, v = f.astype(np.uint8).reshape(pts.shape[:2]), v.reshape(pts.shape[:2])
    want = irt.column_reduce(v, f, SS.weights(wname, rad.size), SS.MISS)
    assert CS.same_outputs(want, SS.reduced(name, key, wname)) is not None  # the update is visible
    with irt.Context(cells, 0) as ctx:
        got = section(ctx, cols, rad, wname)
        check_points(got, *SS.answers(name, key), SS.MISS, "before the update")
        ctx.update_values(np.ascontiguousarray(new["value"]))
        sec = Section(rad.size, cols[0].size, NO_RGBA)
        with pytest.raises(irt.IrtError, match="update is pending") as e:
            ctx.section_raw(cols[0], cols[1], rad, sec.ptrs())
        assert e.value.code == irt.E_INVALID
        sec.torch.cuda.synchronize(0)
        sec.host(written=False)
        ctx.end_update()
        got = section(ctx, cols, rad, wname)
        check_points(got, f, v, SS.MISS, "after the update")
        check_columns(got, want, "after the update")


# ------------------------------------------------------------------ streams
def test_a_section_on_a_second_stream_after_a_sampling_call():
    """A long irt_sample_points on one stream, then sections on another and back: they run behind
    it (the shared device table is theirs in call order) and every result is right."""
    import torch
    name = "filtered"
    pts = S.points(name)
    rad = SS.levels(name)
    with make_context(name, "default") as ctx:
        s1, s2 = torch.cuda.Stream(0), torch.cuda.Stream(0)
        xyz = torch.from_numpy(np.ascontiguousarray(np.tile(pts, (64, 1)))).to("cuda:0")
        val = torch.zeros(len(xyz), dtype=torch.float32, device="cuda:0")
        torch.cuda.synchronize(0)
        ctx.sample_points(xyz.data_ptr(), len(xyz), val.data_ptr(), 0, irt.MODE_USER_GEOM, SS.MISS, s1.cuda_stream)
        a = section(ctx, SS.columns("stations"), rad, "mixed", which=ALL_OUTPUTS, stream=s2.cuda_stream)
        b = section(ctx, SS.columns("oblique"), rad[:7], "none", stream=s1.cuda_stream)  # smaller tables, other stream
        check_points(a, *SS.answers(name, "stations"), SS.MISS, "on the second stream")
        check_columns(a, SS.reduced(name, "stations", "mixed"), "on the second stream")
        assert np.array_equal(a["rgba"], SS.curtain(name, "stations", "default"))
        f, v = SS.answers(name, "oblique")
        check_points(b, f[:7], v[:7], SS.MISS, "back on the first stream")
        f, v = S.cell_answers(name)
        assert np.array_equal(CS.bits(val.cpu().numpy()[:len(pts)]), CS.bits(np.where(f != 0, v, F(SS.MISS))))


# ------------------------------------------------------------------ rendering is untouched
def test_section_calls_leave_rendering_alone():
    from helpers import FRAMING, GpuFrame
    cells = S.scene("flat")
    setup = irt.setup_frame(cells, 64, 64, camera=FRAMING)
    keys = ("raysLaunched", "raysInBox", "locateCalls", "samplesFound", "candidatesTested")
    with irt.Context(cells, 0) as ctx:
        ctx.set_transfunc(setup.lut, setup.value_range)

        def frame():
            fr = GpuFrame(ctx, 64, 64)
            st = fr.render(setup.lp)
            a, f = fr.host()
            return a.view(np.uint32).copy(), f.copy(), tuple(st.asdict()[k] for k in keys)

        before = frame()
        launches = ctx.stats_total()[1]
        section(ctx, SS.columns("equator"), SS.levels("flat"), "mixed", which=ALL_OUTPUTS)
        assert ctx.stats_total()[1] == launches
        assert tuple(ctx.stats().asdict()[k] for k in keys) == before[2]
        after = frame()
        assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
        assert before[2] == after[2] and before[2][2] > 0
        assert ctx.chain_errors() == 0


# ------------------------------------------------------------------ Context.section, the app
def test_context_section_returns_tensors_on_the_device():
    import torch
    name, key, wname = "terrain", "stations", "mixed"
    lat, lon = SS.columns(key)
    rad = SS.levels(name)
    with make_context(name, "default") as ctx:
        out = ctx.section(lat, lon, rad, miss=SS.MISS)
        assert set(out) == {"value", "found"}
        out = ctx.section(lat, lon, rad, SS.weights(wname, rad.size), image=True, columns=True, ambient=SS.AMBIENT[0],
                          radiance=SS.AMBIENT[1], miss=SS.MISS)
        assert set(out) == set(ALL_OUTPUTS)
        for k, t in out.items():
            assert t.is_cuda
            if k in CS.OUTPUTS:
                assert t.shape == (lat.size,)
                assert t.dtype == (torch.float32 if irt.COLUMN_OUTPUTS[k] is np.float32 else torch.int32)
        assert out["value"].shape == out["found"].shape == (rad.size, lat.size)
        assert out["rgba"].shape == (rad.size, lat.size, 4) and out["rgba"].dtype == torch.uint8
        host = {k: t.cpu().numpy() for k, t in out.items()}
        check_points(host, *SS.answers(name, key), SS.MISS, "Context.section")
        check_columns(host, SS.reduced(name, key, wname), "Context.section")
        want = SS.curtain(name, key, "default")
        assert np.array_equal(host["rgba"].reshape(-1).view(np.uint32).reshape(want.shape), want)
        assert np.isnan(ctx.section(lat, lon, [1.0])["value"].cpu().numpy()).all()  # the default miss


def test_icon_rt_section_flag(tmp_path):
    """icon_rt --section lat0,lon0,lat1,lon1,n --section-levels r0,...: the curtain along the great
    circle (degrees in, the library's radians inside) with the app's default transfer function and
    unit ambient terms, as a PNG and, raw, where --dump-fb says; and the flag's refusals."""
    import os
    import subprocess
    name = "flat"
    cells = S.scene(name)
    ic, raw = str(tmp_path / "flat.ic"), str(tmp_path / "curtain.raw")
    irt.save_ic(ic, np.array(cells, copy=True))
    rad = np.sort(SS.levels(name, "ascending"))[::3]
    deg = (10.0, 170.0, -25.0, -160.0, 70)
    app = os.path.join(os.path.dirname(irt.LIB_PATH), "icon_rt")
    cmd = [app, ic, "--section", ",".join(repr(float(v)) for v in deg[:4]) + ",70",
           "--section-levels", ",".join(repr(float(r)) for r in rad), "--dump-fb", raw]
    out = subprocess.run(cmd, cwd=tmp_path, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert os.path.getsize(tmp_path / "icon_rt_section.png") > 0 and "icon_rt_section.png" in out.stdout
    to_rad = lambda d: float(F(d * (np.pi / 180.0)))  # noqa: E731
    lat, lon, _ = irt.great_circle(to_rad(deg[0]), to_rad(deg[1]), to_rad(deg[2]), to_rad(deg[3]), deg[4])
    pts = irt.section_points(lat, lon, rad)
    f, v = LS.sample(cells, irt.MODE_USER_GEOM, pts.reshape(-1, 3))
    want = SS.curtain_of(LS.transfunc(name, "default"), f.reshape(pts.shape[:2]), v.reshape(pts.shape[:2]),
                         ((1.0, 1.0, 1.0), 1.0))
    got = np.fromfile(raw, np.uint32).reshape(rad.size, deg[4])
    assert np.array_equal(got, want) and np.unique(got).size > 8 and (got == 0).any()
    for bad in (["--section", "1,2,3,4,5"], ["--section", "1,2,3,4", "--section-levels", "6.4e6"],
                ["--section", "1,2,3,4,0", "--section-levels", "6.4e6"],
                ["--section", "1,2,3,4,5", "--section-levels", "6.4e6", "--bench", "3"],
                ["--section", "1,2,3,4,5", "--section-levels", "6.4e6", "--gpus", "2"]):
        out = subprocess.run([app, ic] + bad, cwd=tmp_path, capture_output=True, text=True, timeout=120)
        assert out.returncode != 0 and "--section" in out.stderr, bad
