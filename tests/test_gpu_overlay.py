"""irt_render_overlay on the device (csrc/irt_overlay.hip): d_segment against irt_overlay_cover of the
restated points, integer for integer, and d_cover and d_fb against the restatement of the definition
(tests/overlay_scenes.py), bit for bit, on the inputs tests/test_overlay_cpu.py takes its census of;
then the call's conduct.  Every output goes to a buffer pre-filled with a sentinel, with guard words
on both sides (the Frame of tests/test_gpu_levels.py: its accum is the cover here, its level the
segment)."""
import ctypes as C
import functools

import numpy as np
import pytest

import irt
import overlay_scenes as OS
import sample_scenes as S
from test_gpu_levels import SENT, Frame, bits

pytestmark = pytest.mark.gpu

F = np.float32


def accum_tensor(a, device=0):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, F).copy()).to(f"cuda:{device}")


def draw(ctx, ov, frame, view, size, accum_id=0, over=False, accum_in=0, segment=True, stream=0):
    ctx.render_overlay(ov, OS.launch_params(view, size, accum_id), frame.W, frame.H, OS.surface_radius(),
                       frame.ptr("accum"), frame.ptr("fb"), accum_in, frame.ptr("level") if segment else 0, over, stream)
    frame.torch.cuda.synchronize(ctx.device)


@functools.lru_cache(maxsize=None)
def plain_expected(name, view, size):
    """The frame at accumID 0 over a zero cover with no accum."""
    W, H = OS.SIZES[size]
    return OS.expected_frame(name, view, size, 0, False, None, np.zeros((H, W, 4), F))


def check(frame, want, what, segment=True):
    s, K, fb = want
    for which, exp in (("level", s), ("accum", K), ("fb", fb)):
        written = segment or which != "level"
        got = frame.host(which, written)
        if not written:
            continue
        e = bits(exp).reshape(got.shape)
        bad = np.argwhere(got != e)
        assert len(bad) == 0, (f"{what}: {which} differs at {len(bad)} of {got.size} places, first {tuple(bad[0])}: "
                               f"{hex(int(got[tuple(bad[0])]))} vs {hex(int(e[tuple(bad[0])]))}")
    frame.host("value", written=False)  # the call has no such output


def zero_frame(size):
    W, H = OS.SIZES[size]
    return Frame(W, H, prior=np.zeros((H, W, 4), F))


@pytest.fixture(scope="module")
def ctx():
    with irt.Context(S.scene(OS.SCENE), 0) as c:
        yield c


# ------------------------------------------------------------------ every set x frame size x view
@pytest.mark.parametrize("name,bins", OS.DEVICE_SETS, ids=[f"{n}-N{b}" for n, b in OS.DEVICE_SETS])
def test_segments_cover_and_fb_equal_the_restatement(ctx, name, bins):
    with ctx.overlay(OS.segments(name), OS.STYLES, bins) as ov:
        n, entries = ov.bins()  # the table the object was made with
        assert (n == bins or bins == 0) and 1 <= n <= irt.OVERLAY_MAX_BINS
        assert entries == (irt.overlay_bins(OS.segments(name), OS.MAX_W, n)[0][-1] if OS.segments(name).size else 0)
        for view in OS.VIEWS:
            for size in OS.SIZES:
                want = plain_expected(name, view, size)
                frame = zero_frame(size)
                draw(ctx, ov, frame, view, size)
                print(f"{name} N{bins} {view} {size}: {int((want[0] >= 0).sum())} of {want[0].size} pixels on a line")
                check(frame, want, f"{name} N{bins} {view} {size}")


def test_the_wave_uniform_form_gives_the_same_frames(ctx, monkeypatch):
    """The form that lost the measurement (IRT_OVERLAY_UNIFORM=1, profiles/overlay_rate.py) stays correct."""
    monkeypatch.setenv("IRT_OVERLAY_UNIFORM", "1")
    for name, bins in (("coast", 4), ("graticule", 0), ("views", 0)):
        with ctx.overlay(OS.segments(name), OS.STYLES, bins) as ov:
            for view in OS.VIEWS:
                frame = zero_frame("odd")
                draw(ctx, ov, frame, view, "odd")
                check(frame, plain_expected(name, view, "odd"), f"wave-uniform {name} {view}")


# ------------------------------------------------------------------ the lerp and the composite
@pytest.mark.parametrize("over", [False, True], ids=["under", "over"])
@pytest.mark.parametrize("accum_id", [0, 3])
@pytest.mark.parametrize("source", ["null", "random", "render"])
def test_cover_lerp_and_composite(ctx, source, accum_id, over):
    import torch
    name, view, size = "views", "outside", "odd"
    W, H = OS.SIZES[size]
    prior = OS.prior_cover(W, H) if accum_id else np.zeros((H, W, 4), F)
    accum, dev = None, None
    if source == "random":
        accum = OS.random_accum(W, H)
        dev = accum_tensor(accum)
    elif source == "render":  # the accum of an actual irt_render frame of this view
        from helpers import GpuFrame
        setup = irt.setup_frame(S.scene(OS.SCENE), W, H)
        ctx.set_transfunc(setup.lut, setup.value_range)
        fr = GpuFrame(ctx, W, H)
        fr.render(OS.launch_params(view, size, 0))
        accum = fr.host()[0].copy()
        dev = fr.accum
        assert (accum[..., 3] > 0).any() and (accum[..., 3] < 1).any()
    before = dev.clone() if dev is not None else None
    want = OS.expected_frame(name, view, size, accum_id, over, accum, prior)
    assert (want[0] >= 0).sum() >= 20
    with ctx.overlay(OS.segments(name), OS.STYLES) as ov:
        frame = Frame(W, H, prior=prior)
        draw(ctx, ov, frame, view, size, accum_id, over, dev.data_ptr() if dev is not None else 0)
        check(frame, want, f"{source} accumID {accum_id} over={over}")
    if dev is not None:
        assert torch.equal(dev, before), "d_accum_in was written"


# ------------------------------------------------------------------ outputs and side effects
def test_null_segment_zero_segments_and_the_same_call_twice(ctx):
    name, view, size = "pole", "outside", "odd"
    W, H = OS.SIZES[size]
    want = plain_expected(name, view, size)
    with ctx.overlay(OS.segments(name), OS.STYLES) as ov, ctx.overlay(OS.segments("none"), OS.STYLES) as empty:
        frame = zero_frame(size)
        draw(ctx, ov, frame, view, size, segment=False)
        check(frame, want, "d_segment NULL", segment=False)
        draw(ctx, ov, frame, view, size)  # accumID 0 again into the same buffers: the same frame
        check(frame, want, "the same call twice")
        # ... and the next progressive frame lerps onto what the first left
        draw(ctx, ov, frame, view, size, accum_id=1)
        check(frame, OS.expected_frame(name, view, size, 1, False, None, want[1]), "accumID 1 onto accumID 0")
        # zero segments: the call only composites
        acc = OS.random_accum(W, H)
        dev = accum_tensor(acc)
        frame = zero_frame(size)
        draw(ctx, empty, frame, view, size, accum_in=dev.data_ptr())
        s, K, fb = OS.expected_frame("none", view, size, 0, False, acc, np.zeros((H, W, 4), F))
        assert (s == -1).all() and not K.any()
        check(frame, (s, K, fb), "zero segments")
        assert empty.num_segments == 0


# ------------------------------------------------------------------ context interactions
def test_two_overlays_destroy_foreign_context_update_and_a_second_stream(ctx):
    import torch
    view, size = "outside", "odd"
    cells = S.scene(OS.SCENE)
    a = ctx.overlay(OS.segments("graticule"), OS.STYLES, 8)
    b = ctx.overlay(OS.segments("views"), OS.STYLES)
    frame = zero_frame(size)
    draw(ctx, a, frame, view, size)
    check(frame, plain_expected("graticule", view, size), "the first of two overlays")
    frame = zero_frame(size)
    draw(ctx, b, frame, view, size)
    check(frame, plain_expected("views", view, size), "the second of two overlays")
    a.close()
    a.close()  # twice: nothing
    frame = zero_frame(size)
    draw(ctx, b, frame, view, size)
    check(frame, plain_expected("views", view, size), "after the other overlay's destruction")
    L = irt.lib()
    with irt.Context(cells[:64], 0) as other:
        frame = Frame(*OS.SIZES[size])
        with pytest.raises(irt.IrtError, match="not an overlay of this context") as e:
            draw(other, b, frame, view, size)
        assert e.value.code == irt.E_INVALID
        assert L.irt_overlay_destroy(other._h, b._h) == irt.E_INVALID
        for which in ("fb", "accum", "level"):
            frame.host(which, written=False)
    # a pending update: refused, then fine after the commit
    ctx.update_values(np.ascontiguousarray(cells["value"]))
    with pytest.raises(irt.IrtError, match="update is pending"):
        draw(ctx, b, frame, view, size)
    torch.cuda.synchronize(0)
    frame.host("fb", written=False)
    ctx.end_update()
    # a second stream, behind a sampling call on the first
    s1, s2 = torch.cuda.Stream(0), torch.cuda.Stream(0)
    frame2 = zero_frame(size)
    draw(ctx, b, frame, view, size, stream=s1.cuda_stream)
    draw(ctx, b, frame2, "beside", size, stream=s2.cuda_stream)
    check(frame, plain_expected("views", view, size), "on the first stream")
    check(frame2, plain_expected("views", "beside", size), "on the second stream")
    b.close()
    # overlays left open are the context's to free
    with irt.Context(cells[:64], 0) as other:
        other.overlay(OS.segments("pole"), OS.STYLES)
        other.overlay(OS.segments("none"), OS.STYLES)


def test_every_refusal_writes_nothing(ctx):
    import torch
    W, H = 8, 8
    L = irt.lib()
    frame = Frame(W, H)
    lp = OS.launch_params("outside", "packet")
    st, ns = irt.overlay_styles(OS.STYLES)
    seg = np.array(OS.segments("overlap"), copy=True)
    h = C.c_void_p()

    def create(c=ctx._h, seg=seg, n=None, st=st, ns=ns, N=0, out=C.byref(h)):
        return L.irt_overlay_create(c, C.c_void_p(seg.ctypes.data) if seg is not None else None,
                                    seg.size if n is None else n, st, ns, N, out)

    def refused(rc, word):
        assert rc == irt.E_INVALID and word in L.irt_last_error().decode(), L.irt_last_error()

    refused(create(c=None), "null context")
    refused(create(out=None), "null overlay")
    refused(create(seg=None, n=3), "null segments")
    refused(create(n=1 << 24), "2^24")
    refused(create(ns=0), "styles are outside")
    refused(create(ns=1), "style 1 is outside the table of 1")
    refused(create(st=irt.overlay_styles([((1, 1, 1, 1), 0.2), ((1, 1, 1, 1), 0.01)])[0]), "halfWidth")
    for N in (-1, 257):
        refused(create(N=N), "binsPerEdge")
    assert h.value is None
    with ctx.overlay(seg, OS.STYLES) as ov:
        def call(c=ctx._h, o=ov._h, lp=lp, w=W, hgt=H, r=OS.surface_radius(), flags=0, cover=True, fb=True):
            return L.irt_render_overlay(c, o, C.byref(lp) if lp is not None else None, w, hgt, r, flags, None,
                                        C.c_void_p(frame.ptr("accum")) if cover else None,
                                        C.c_void_p(frame.ptr("fb")) if fb else None, C.c_void_p(frame.ptr("level")), None)

        refused(call(c=None), "null context")
        refused(call(o=None), "null overlay")
        refused(call(lp=None), "null lp")
        refused(call(cover=False), "null d_cover or d_fb")
        refused(call(fb=False), "null d_cover or d_fb")
        for r in (0.0, -6.4e6, np.nan, np.inf, -np.inf):
            refused(call(r=r), "surfaceRadius")
        for flags in (2, 3, -1, 1 << 16):
            refused(call(flags=flags), "unknown flag bits")
        for w, hgt in ((0, 8), (8, 0), (-3, 8), (1 << 14, 1 << 13), (1 << 27, 1)):
            refused(call(w=w, hgt=hgt), "pixels")
        hb = C.c_void_p()  # a context still being created
        cells = S.scene(OS.SCENE)[:64]
        assert L.irt_create_begin(cells.size, 0, C.byref(hb)) == 0
        refused(call(c=hb), "still being created")
        refused(create(c=hb), "still being created")
        assert L.irt_create_append(hb, C.c_void_p(cells.ctypes.data), cells.size) == 0 and L.irt_create_end(hb) == 0
        L.irt_destroy(hb)
        torch.cuda.synchronize(0)
        for which in ("fb", "accum", "level"):
            frame.host(which, written=False)
        assert call(flags=irt.OVERLAY_OVER) == 0  # the same call, now valid
        torch.cuda.synchronize(0)
        assert (frame.host("fb") != SENT).all() and (frame.host("level") != SENT).all()


# ------------------------------------------------------------------ Python
def test_overlay_width_draws_a_line_of_that_many_pixels(ctx):
    view, size = "outside", "square"
    W, H = OS.SIZES[size]
    w = irt.overlay_width(OS.launch_params(view, size), H, OS.surface_radius(), 3.0)
    seg = irt.overlay_segments(np.array([60, 90, 60], F) * F(OS.RAD), np.array([90, 90, 270], F) * F(OS.RAD), None, 0.1)
    with ctx.overlay(seg, [((1.0, 1.0, 1.0, 1.0), w)]) as ov:
        frame = zero_frame(size)
        draw(ctx, ov, frame, view, size)
        on = frame.host("level").view(np.int32)[H // 2] >= 0
        assert 2 <= on.sum() <= 4
        fb = frame.host("fb")[H // 2]
        assert (fb[on] == 0xFFFFFFFF).all() and (fb[~on] == 0).all()


def test_icon_rt_line_flags_write_the_frame_of_the_api(tmp_path):
    """icon_rt --graticule a,b --lines FILE --line-width PX [--lines-over]: the dumped frame is irt_render's
    with irt_render_overlay drawn into it (file lines in style 0, the graticule in style 1, 1 degree pieces,
    PX pixels wide by overlay_width); and the flags' refusals."""
    import os
    import subprocess
    from helpers import FRAMING, GpuFrame
    cells = S.scene(OS.SCENE)
    size = 64
    ic, raw, txt = str(tmp_path / "flat.ic"), str(tmp_path / "frame.raw"), str(tmp_path / "lines.txt")
    irt.save_ic(ic, np.array(cells, copy=True))
    with open(txt, "w") as f:
        f.write("# two polylines\n80 0\n70.5 40  # a comment\n62 95\n\n\n85 -120" + " " * 300 + "# a long line\n75 -100\n")
    vp, vi, vu, fovy = FRAMING
    app = os.path.join(os.path.dirname(irt.LIB_PATH), "icon_rt")
    base = [app, ic, "--size", str(size), str(size), "--camera", *[str(v) for v in (*vp, *vi, *vu)], "-fovy", str(fovy),
            "--true-size", "--sample-limit", "1", "--dump-fb", raw]
    setup = irt.setup_frame(cells, size, size, camera=FRAMING)
    R = float(setup.info.sphericalBounds.lower.x)
    w = irt.overlay_width(setup.lp, size, R, 2.0)
    styles = [((1.0, 1.0, 1.0, 1.0), w), ((0.75, 0.75, 0.75, 0.7), w)]
    deg = F(np.pi / 180.0)
    to_rad = lambda v: np.array([x * (np.pi / 180.0) for x in v]).astype(F)  # noqa: E731
    seg = np.concatenate([irt.overlay_segments(to_rad([80, 70.5, 62, 85, 75]), to_rad([0, 40, 95, -120, -100]), [0, 3, 5],
                                               float(deg), 0),
                          irt.graticule(float(F(30 * (np.pi / 180.0))), float(F(45 * (np.pi / 180.0))), float(deg), 1)])
    for over in (False, True):
        cmd = base + ["--graticule", "30,45", "--lines", txt, "--line-width", "2"] + (["--lines-over"] if over else [])
        out = subprocess.run(cmd, cwd=tmp_path, capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stderr
        assert f"{seg.size} line segments" in out.stderr
        got = np.fromfile(raw, np.uint32).reshape(size, size)
        with irt.Context(cells, 0) as ctx:
            ctx.set_transfunc(setup.lut, setup.value_range)
            fr = GpuFrame(ctx, size, size)
            fr.render(setup.lp)
            plain = fr.host()[1].copy()
            cover = accum_tensor(np.zeros((size, size, 4), F))
            with ctx.overlay(seg, styles) as ov:
                ctx.render_overlay(ov, setup.lp, size, size, R, cover.data_ptr(), fr.fb.data_ptr(), fr.accum.data_ptr(), 0, over)
                want = fr.host()[1]
        assert np.array_equal(got, want), int((got != want).sum())
        # (on top the lines show everywhere; underneath only where the volume lets them through)
        assert (want != plain).sum() >= (100 if over else 1)
    for bad in (["--graticule", "30"], ["--lines-over"], ["--line-width", "2"], ["--graticule", "30,30", "--line-width", "0"],
                ["--graticule", "30,30", "--bench", "3"], ["--graticule", "30,30", "--gpus", "2"],
                ["--graticule", "30,30", "--histogram", "7"]):
        out = subprocess.run(base + bad, cwd=tmp_path, capture_output=True, text=True, timeout=120)
        assert out.returncode != 0 and "--graticule" in out.stderr, bad
    out = subprocess.run(base + ["--lines", str(tmp_path / "missing.txt")], cwd=tmp_path, capture_output=True, text=True,
                         timeout=120)
    assert out.returncode != 0 and "cannot read" in out.stderr


# ------------------------------------------------------------------ rendering is untouched
def test_overlay_calls_leave_rendering_alone():
    from helpers import FRAMING, GpuFrame
    cells = S.scene(OS.SCENE)
    setup = irt.setup_frame(cells, 64, 64, camera=FRAMING)
    keys = ("raysLaunched", "raysInBox", "locateCalls", "samplesFound", "candidatesTested")
    radii = [float(S.shell(cells)[2])]
    with irt.Context(cells, 0) as ctx:
        ctx.set_transfunc(setup.lut, setup.value_range)

        def frames():
            fr = GpuFrame(ctx, 64, 64)
            st = fr.render(setup.lp)
            a, f = fr.host()
            lv = Frame(64, 64, prior=np.zeros((64, 64, 4), F))
            ctx.render_levels(setup.lp, 64, 64, radii, lv.ptr("fb"), lv.ptr("accum"))
            lv.torch.cuda.synchronize(0)
            return (a.view(np.uint32).copy(), f.copy(), lv.host("fb").copy(), lv.host("accum").copy(),
                    tuple(st.asdict()[k] for k in keys))

        before = frames()
        launches = ctx.stats_total()[1]
        with ctx.overlay(OS.segments("graticule"), OS.STYLES) as ov:
            frame = zero_frame("square")
            draw(ctx, ov, frame, "outside", "square")
            assert ctx.stats_total()[1] == launches
            assert tuple(ctx.stats().asdict()[k] for k in keys) == before[4]
            after = frames()
        for x, y in zip(before[:4], after[:4]):
            assert np.array_equal(x, y)
        assert before[4] == after[4] and before[4][2] > 0
        assert ctx.chain_errors() == 0
