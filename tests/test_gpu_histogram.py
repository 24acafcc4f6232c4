"""irt_histogram on the device (csrc/irt_histogram.hip) against irt_histogram_cells, integer for
integer on bins, tails and outside, on the inputs tests/test_histogram_cpu.py takes its census of;
then the call's conduct.  Every output goes to a buffer pre-filled with a sentinel, with guard words
on both sides.

The kernel's grid: workgroups of 256 lanes, 16 lanes per record, 4 records per 16-lane group and
pass -- 64 records per workgroup and pass -- and as many workgroups as the device holds at once (at
most 8 per CU: 2,048 on 256 CUs, 131,072 records per pass), fewer for a small scene.  IRT_HIST_WGS
caps the grid, so that a small scene takes many passes."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import histogram_scenes as HS
import irt

pytestmark = pytest.mark.gpu

GUARD = 32
SENT = 0x5A5A5A5A5A5A5A5A  # (positive as int64)
F = np.float32
SIZES = {"bins": 4096, "tails": 192, "outside": 1}  # the most a call may write


class Hist:
    """The three outputs as device buffers between guards, sentinel-filled; `which`: the outputs
    handed to the call (the others stay NULL)."""

    def __init__(self, bands, bins, which=irt.HISTOGRAM_OUTPUTS, device=0):
        import torch
        self.torch, self.which = torch, tuple(which)
        self.size = {"bins": bands * bins, "tails": bands * 3, "outside": 1}
        self.shape = {"bins": (bands, bins), "tails": (bands, 3), "outside": (1,)}
        self.buf = {k: torch.full((n + 2 * GUARD,), SENT, dtype=torch.int64, device=f"cuda:{device}")
                    for k, n in self.size.items()}

    def ptrs(self):
        return {k: self.buf[k].data_ptr() + 8 * GUARD for k in self.which}

    def host(self, written=True):
        out = {}
        for k, t in self.buf.items():
            v = t.cpu().numpy().view(np.uint64)
            n = self.size[k]
            assert (v[:GUARD] == SENT).all() and (v[GUARD + n:] == SENT).all(), f"{k} guards"
            v = v[GUARD:GUARD + n]
            if not written or k not in self.which:
                assert (v == SENT).all(), f"{k} was written"
            else:
                out[k] = v.reshape(self.shape[k]).copy()
        return out


def histogram(ctx, vrange, bins, weighting="count", edges=None, which=irt.HISTOGRAM_OUTPUTS, stream=0, into=None):
    bands = 1 if edges is None else len(edges) - 1
    h = into or Hist(bands, bins, which, ctx.device)
    assert ctx.histogram_raw(vrange, bins, h.ptrs(), weighting, edges, stream) == (bands, bins)
    h.torch.cuda.synchronize(ctx.device)
    return h.host()


def check_scene(ctx, name, cases=None):
    for rk, bins, bk, w in cases or HS.cases(name):
        got = histogram(ctx, HS.value_range(name, rk), bins, w, HS.band_edges(name, bk))
        d = HS.differs(got, HS.expected(name, rk, bins, bk, w))
        assert d is None, f"irt_histogram {name} {rk} {bins} bins {bk} {w}: {d}"


# ------------------------------------------------------------------ against the helper
@pytest.mark.parametrize("name", HS.SCENE_NAMES)
def test_histogram_equals_the_helper_on_the_scenes(name):
    """Every range, bin count, band set and weighting of the scene."""
    with irt.Context(HS.scene(name), 0) as ctx:
        check_scene(ctx, name)


@pytest.mark.parametrize("n", HS.COUNTS)
def test_histogram_equals_the_helper_on_the_hand_made_records(n):
    """1, 63, 64, 65, 255, 256 and 257 records holding the values and layer counts the census needs."""
    with irt.Context(HS.scene(f"hand{n}"), 0) as ctx:
        check_scene(ctx, f"hand{n}")


LARGE_CASES = [("data", 300, "none", "count"), ("inner", 7, "three", "thickness")]


@pytest.mark.parametrize("wgs", [None, 7, 1], ids=["full", "wgs7", "wgs1"])
def test_more_records_than_one_pass_of_the_grid(monkeypatch, wgs):
    """61,440 records: one pass of the full grid (960 workgroups), and with the grid capped at 7
    workgroups (138 passes of 448 records, the last one partial) and at 1 (960 passes)."""
    if wgs:
        monkeypatch.setenv("IRT_HIST_WGS", str(wgs))
    with irt.Context(HS.scene("large"), 0) as ctx:
        check_scene(ctx, "large", LARGE_CASES)


def test_however_the_context_was_made(tmp_path):
    """irt_create_begin / _append / _end in uneven chunks, a file, and the synthetic generator."""
    cells = HS.scene("terrain")
    cuts = [0, 1, 2, 1002, 1039, 4096, cells.size]
    chunks = [cells[a:b] for a, b in zip(cuts, cuts[1:])]
    cases = [("inner", 300, "none", "count"), ("data", 7, "three", "thickness"), ("data", 64, "sixtyfour", "count")]
    with irt.Context.streamed(chunks, cells.size, 0) as ctx:
        check_scene(ctx, "terrain", cases)
    path = str(tmp_path / "terrain.ic")
    irt.save_ic(path, np.array(cells, copy=True))
    with irt.Context.from_file(path, -1, 0) as ctx:
        check_scene(ctx, "terrain", cases)
    with irt.Context.synth(2, 3, 90, 0) as ctx:  # the flat scene's generator, straight into HBM
        check_scene(ctx, "flat", cases)


# ------------------------------------------------------------------ time series
def test_histogram_follows_value_updates():
    """After update_values_device and end_update the result is the helper's on the updated records;
    between the two the call is refused and leaves the sentinel-filled outputs alone."""
    import torch
    name = "flat"
    cells = np.array(HS.scene(name), copy=True)
    new = np.array(cells, copy=True)
    new["value"] = (F(1.0) - cells["value"][::-1]) * F(0.75) + F(0.125)
    vr = HS.value_range(name, "inner")
    edges = HS.band_edges(name, "three")
    want = irt.histogram_cells(new, vr, 300, "thickness", edges)
    assert HS.differs(want, HS.expected(name, "inner", 300, "three", "thickness")) is not None  # the update shows
    with irt.Context(cells, 0) as ctx:
        assert HS.differs(histogram(ctx, vr, 300, "thickness", edges), HS.expected(name, "inner", 300, "three", "thickness")) is None
        d_new = torch.from_numpy(np.ascontiguousarray(new["value"])).to("cuda:0")
        torch.cuda.synchronize(0)
        ctx.update_values_device(d_new.data_ptr(), cells.size)
        h = Hist(3, 300)
        with pytest.raises(irt.IrtError, match="update is pending") as e:
            ctx.histogram_raw(vr, 300, h.ptrs(), "thickness", edges)
        assert e.value.code == irt.E_INVALID
        torch.cuda.synchronize(0)
        h.host(written=False)
        ctx.end_update()
        d = HS.differs(histogram(ctx, vr, 300, "thickness", edges), want)
        assert d is None, d
        # the new dataRange is the default range
        got = {k: t.cpu().numpy() for k, t in ctx.histogram(bins=7).items()}
        r = irt.volume_info(new).dataRange
        assert HS.differs(got, irt.histogram_cells(new, (r.lower, r.upper), 7)) is None


# ------------------------------------------------------------------ outputs
def test_each_output_alone_none_at_all_and_twice_into_the_same_buffers():
    name, case = "terrain", ("inner", 7, "three", "thickness")
    rk, bins, bk, w = case
    vr, edges = HS.value_range(name, rk), HS.band_edges(name, bk)
    want = HS.expected(name, *case)
    with irt.Context(HS.scene(name), 0) as ctx:
        for k in irt.HISTOGRAM_OUTPUTS:
            one = histogram(ctx, vr, bins, w, edges, which=(k,))  # (host() checks the others' sentinels)
            assert set(one) == {k} and np.array_equal(one[k], want[k]), k
        for which in (("bins", "outside"), ("tails", "outside")):
            some = histogram(ctx, vr, bins, w, edges, which=which)
            assert all(np.array_equal(some[k], want[k]) for k in which), which
        h = Hist(3, bins)
        ctx.histogram_raw(vr, bins, {}, w, edges)  # every pointer NULL: IRT_OK, nothing launched
        ctx.histogram_raw(vr, bins, {"bins": 0, "outside": 0}, w, edges)
        h.torch.cuda.synchronize(0)
        h.host(written=False)
        first = histogram(ctx, vr, bins, w, edges, into=h)
        second = histogram(ctx, vr, bins, w, edges, into=h)  # overwrites: not twice the counts
        assert HS.differs(first, want) is None and HS.differs(second, want) is None
        other = histogram(ctx, HS.value_range(name, "data"), bins, "count", edges, into=h)  # ... whatever they held
        assert HS.differs(other, HS.expected(name, "data", bins, bk, "count")) is None
    with irt.Context(np.zeros(0, irt.CELL_DTYPE), 0) as ctx:  # a scene without records: zeroes
        got = histogram(ctx, (0.0, 1.0), 7, "count", edges)
        assert all((a == 0).all() for a in got.values()) and got["bins"].shape == (3, 7)


def test_a_histogram_on_a_second_stream_after_a_sampling_call():
    """A long irt_sample_points on one stream, then histograms on another and back: every result is right."""
    import torch
    import sample_scenes as S
    name = "filtered"
    pts = S.points(name)
    with irt.Context(HS.scene(name), 0) as ctx:
        s1, s2 = torch.cuda.Stream(0), torch.cuda.Stream(0)
        xyz = torch.from_numpy(np.ascontiguousarray(np.tile(pts, (64, 1)))).to("cuda:0")
        val = torch.zeros(len(xyz), dtype=torch.float32, device="cuda:0")
        torch.cuda.synchronize(0)
        ctx.sample_points(xyz.data_ptr(), len(xyz), val.data_ptr(), 0, irt.MODE_USER_GEOM, -1.0, s1.cuda_stream)
        a = histogram(ctx, HS.value_range(name, "inner"), 300, "count", None, stream=s2.cuda_stream)
        b = histogram(ctx, HS.value_range(name, "data"), 64, "thickness", HS.band_edges(name, "sixtyfour"),
                      stream=s1.cuda_stream)
        assert HS.differs(a, HS.expected(name, "inner", 300, "none", "count")) is None
        assert HS.differs(b, HS.expected(name, "data", 64, "sixtyfour", "thickness")) is None
        f, v = S.cell_answers(name)
        got = val.cpu().numpy()[:len(pts)]
        assert np.array_equal(got.view(np.uint32), np.where(f != 0, v, F(-1.0)).astype(F).view(np.uint32))


# ------------------------------------------------------------------ refusals
def test_every_refusal_writes_nothing():
    import torch
    cells = HS.scene("hand65")
    L = irt.lib()
    h = Hist(64, 64)
    ptrs = h.ptrs()
    full = irt.HistogramOut(**ptrs)
    edges = np.array([6.3e6, 6.4e6, 6.5e6, 6.6e6], F)

    def call(handle, rng=(0.0, 1.0), bins=7, w=0, e=None, bands=1, out=full):
        return L.irt_histogram(handle, irt.box1(*rng), bins, w, e.ctypes.data if e is not None else None, bands, out, None)

    def refused(rc, word):
        assert rc == irt.E_INVALID and word in L.irt_last_error().decode(), L.irt_last_error()

    refused(call(None), "null context")
    with irt.Context(cells, 0) as ctx:
        for bins in (0, -1, 4097):
            refused(call(ctx._h, bins=bins), "bins are outside")
        for bands in (0, -3, 65):
            refused(call(ctx._h, e=edges, bands=bands), "bands are outside")
        refused(call(ctx._h, bins=2048, e=edges, bands=3), "more than 4096 counters")
        refused(call(ctx._h, bins=65, e=np.linspace(6.3e6, 6.5e6, 65).astype(F), bands=64), "more than 4096 counters")
        for rng in ((1.0, 1.0), (2.0, 1.0), (np.nan, 1.0), (0.0, np.nan), (-np.inf, 1.0), (0.0, np.inf)):
            refused(call(ctx._h, rng=rng), "valueRange")
        for w in (-1, 2):
            refused(call(ctx._h, w=w), "weighting")
        refused(call(ctx._h, bands=3), "null bandEdges")
        for k, bad in ((0, np.nan), (1, np.inf), (3, -np.inf), (2, 6.4e6), (2, 6.3e6)):
            e = edges.copy()
            e[k] = bad
            refused(call(ctx._h, e=e, bands=3), "bandEdges[")
        with pytest.raises(irt.IrtError, match="unknown outputs"):
            ctx.histogram_raw((0, 1), 7, {"mean": 1})
        with pytest.raises(irt.IrtError, match="weighting"):
            ctx.histogram_raw((0, 1), 7, ptrs, "volume")
        ctx.update_values(np.ascontiguousarray(cells["value"]))
        refused(call(ctx._h), "update is pending")
        ctx.end_update()
        torch.cuda.synchronize(0)
        h.host(written=False)
        assert call(ctx._h, bins=64, e=np.linspace(6.3e6, 6.5e6, 65).astype(F), bands=64) == 0  # the same call, now valid
        torch.cuda.synchronize(0)
        assert set(h.host()) == set(irt.HISTOGRAM_OUTPUTS)
    hnd = C.c_void_p()  # a context still being created; then completed and destroyed as usual
    assert L.irt_create_begin(cells.size, 0, C.byref(hnd)) == 0
    refused(call(hnd), "still being created")
    assert L.irt_create_append(hnd, C.c_void_p(cells.ctypes.data), cells.size) == 0 and L.irt_create_end(hnd) == 0
    L.irt_destroy(hnd)


# ------------------------------------------------------------------ rendering is untouched
def test_histogram_calls_leave_rendering_alone():
    from helpers import FRAMING, GpuFrame
    cells = HS.scene("flat")
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
        got = histogram(ctx, HS.value_range("flat", "inner"), 300, "thickness", HS.band_edges("flat", "three"))
        assert HS.differs(got, HS.expected("flat", "inner", 300, "three", "thickness")) is None
        assert ctx.stats_total()[1] == launches
        assert tuple(ctx.stats().asdict()[k] for k in keys) == before[2]
        after = frame()
        assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
        assert before[2] == after[2] and before[2][2] > 0
        assert ctx.chain_errors() == 0


# ------------------------------------------------------------------ Context.histogram, the app
def test_context_histogram_defaults():
    """No argument at all: 300 bins over the context's dataRange, counted, one band, int64 tensors on
    the device; without a transfer function and without the wedge accelerator."""
    import torch
    name = "terrain"
    with irt.Context(HS.scene(name), 0) as ctx:
        out = ctx.histogram()
        assert set(out) == set(irt.HISTOGRAM_OUTPUTS)
        assert all(t.is_cuda and t.dtype == torch.int64 for t in out.values())
        assert out["bins"].shape == (1, 300) and out["tails"].shape == (1, 3) and out["outside"].shape == (1,)
        got = {k: t.cpu().numpy() for k, t in out.items()}
        assert HS.differs(got, HS.expected(name, "data", 300, "none", "count")) is None
        assert got["tails"].sum() == 0 and got["bins"].sum() == HS.scene(name)["numLayers"].sum()
        out = ctx.histogram(HS.value_range(name, "inner"), 7, "thickness", HS.band_edges(name, "three"))
        got = {k: t.cpu().numpy() for k, t in out.items()}
        assert out["bins"].shape == (3, 7) and HS.differs(got, HS.expected(name, "inner", 7, "three", "thickness")) is None


def parse_app(stdout, bands, bins):
    """The flag's output: one line per band -- `band b: c0 ... cN-1 | under u over o nonfinite n` -- and `outside: n`."""
    rows = [ln for ln in stdout.splitlines() if ln.startswith("band ")]
    assert len(rows) == bands
    out = {"bins": np.zeros((bands, bins), np.uint64), "tails": np.zeros((bands, 3), np.uint64)}
    for b, ln in enumerate(rows):
        head, tail = ln.split("|")
        assert head.split(":")[0] == f"band {b}"
        out["bins"][b] = [int(x) for x in head.split(":")[1].split()]
        words = tail.split()
        assert words[0::2] == ["under", "over", "nonfinite"]
        out["tails"][b] = [int(x) for x in words[1::2]]
    out["outside"] = np.array([int(ln.split(":")[1]) for ln in stdout.splitlines() if ln.startswith("outside:")], np.uint64)
    return out


def test_icon_rt_histogram_flag(tmp_path):
    """icon_rt --histogram N [--histogram-thickness] [--histogram-bands ...] over the app's default
    transfer function's value range, against the helper; and the flag's refusals."""
    name = "terrain"
    cells = HS.scene(name)
    ic = str(tmp_path / "terrain.ic")
    irt.save_ic(ic, np.array(cells, copy=True))
    app = os.path.join(os.path.dirname(irt.LIB_PATH), "icon_rt")
    r = irt.volume_info(cells).dataRange
    vr = irt.default_transfunc((r.lower, r.upper))[1]
    edges = HS.band_edges(name, "three")
    out = subprocess.run([app, ic, "--histogram", "300"], cwd=tmp_path, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert HS.differs(parse_app(out.stdout, 1, 300), irt.histogram_cells(cells, vr, 300)) is None
    out = subprocess.run([app, ic, "--histogram", "7", "--histogram-thickness", "--histogram-bands",
                          ",".join(repr(float(e)) for e in edges)], cwd=tmp_path, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    want = irt.histogram_cells(cells, vr, 7, "thickness", edges)
    assert HS.differs(parse_app(out.stdout, 3, 7), want) is None and want["outside"][0] > 0
    for bad in (["--histogram", "0"], ["--histogram-thickness"], ["--histogram", "7", "--histogram-bands", "6.4e6"],
                ["--histogram", "7", "--bench", "3"], ["--histogram", "7", "--gpus", "2"],
                ["--histogram", "7", "--levels", "6.4e6"], ["--histogram", "5000"],
                ["--histogram", "7", "--histogram-bands", "6.5e6,6.4e6"]):
        out = subprocess.run([app, ic] + bad, cwd=tmp_path, capture_output=True, text=True, timeout=120)
        assert out.returncode != 0 and "histogram" in out.stderr, bad
