"""irt_contour_grid and irt_contour_latlon on the device (csrc/irt_contour.hip) against
irt_contour_cells, the host definition that tests/test_contour_cpu.py holds to the NumPy restatement:
every segment byte for byte, the count and the counts per threshold, on the fields of
tests/contour_scenes.py; then the overlay end to end and the calls' conduct.  d_out always lies
between two 64-byte guard lines in a buffer pre-filled with a sentinel."""
import numpy as np
import pytest

import contour_scenes as CS
import helpers
import irt
import levels_scenes as LS
import overlay_scenes as OS
import sample_scenes as S

pytestmark = pytest.mark.gpu

F = np.float32
SENT = 0xA5


class Out:
    """`capacity` segments of device memory with a guard line on either side."""

    def __init__(self, capacity, device=0):
        import torch
        self.torch, self.capacity = torch, int(capacity)
        self.buf = torch.full(((self.capacity + 2) * 64,), SENT, dtype=torch.uint8, device=f"cuda:{device}")
        assert self.buf.data_ptr() % 64 == 0
        self.ptr = self.buf.data_ptr() + 64

    def host(self, n):
        """The first n segments, after checking that every other byte still holds the sentinel."""
        self.torch.cuda.synchronize()
        raw = self.buf.cpu().numpy()
        rest = np.concatenate([raw[:64], raw[64 * (1 + n):]])
        assert (rest == SENT).all(), f"{int((rest != SENT).sum())} bytes outside the {n} segments were written"
        return raw[64:64 * (1 + n)].view(irt.SEGMENT_DTYPE).copy()


def device_field(name, device=0):
    import torch
    f = CS.field(name)
    v = torch.from_numpy(np.array(f.value)).to(f"cuda:{device}")
    fd = torch.from_numpy(np.array(f.found)).to(f"cuda:{device}") if f.found is not None else None
    return f, v, fd


def run_grid(ctx, name, wrap, thresholds=None, styles=None, stream=0, slack=3):
    f, v, fd = device_field(name, ctx.device)
    thr = f.thresholds if thresholds is None else thresholds
    sty = f.styles if styles is None else styles
    n0, per0 = ctx.contour_grid(v.data_ptr(), fd.data_ptr() if fd is not None else 0, f.lat, f.lon, thr, sty, 0, 0,
                                wrap, stream)
    out = Out(n0 + slack, ctx.device)
    n, per = ctx.contour_grid(v.data_ptr(), fd.data_ptr() if fd is not None else 0, f.lat, f.lon, thr, sty, out.ptr,
                              out.capacity, wrap, stream)
    assert n == n0 and per.tolist() == per0.tolist(), "the count-only call and the full call disagree"
    return out.host(n), per


@pytest.fixture(scope="module")
def ctx():
    with irt.Context(S.scene(OS.SCENE), 0) as c:
        yield c


# ------------------------------------------------------------------ every field, both wrap settings
@pytest.mark.parametrize("name,wrap", CS.CASES, ids=CS.CASE_IDS)
def test_grid_equals_the_host_definition(ctx, name, wrap):
    want, want_per = CS.host(name, wrap)
    got, per = run_grid(ctx, name, wrap)
    print(f"{name} wrap={wrap}: {got.size} segments, per threshold {per.tolist()}")
    assert per.tolist() == want_per.tolist()
    CS.same_bytes(got, want, f"{name} wrap={wrap}")
    if name == "wide":  # the order is the same in two runs
        again, _ = run_grid(ctx, name, wrap)
        CS.same_bytes(again, got, f"{name} wrap={wrap}, the second run")


def test_one_and_sixteen_thresholds_and_a_threshold_given_twice(ctx):
    f = CS.field("smooth")
    one, per1 = run_grid(ctx, "smooth", True, [0.35], [3])
    assert per1.tolist() == [one.size] and one.size > 0
    CS.same_bytes(one, irt.contour_cells(f.value, None, f.lat, f.lon, [0.35], [3], True), "T = 1")
    thr16, sty16 = np.linspace(-0.9, 0.9, 16).astype(F), np.arange(16) % 8
    many, per16 = run_grid(ctx, "smooth", True, thr16, sty16)
    want, want_per = irt.contour_cells(f.value, None, f.lat, f.lon, thr16, sty16, True, return_counts=True)
    assert per16.tolist() == want_per.tolist() and (per16 > 0).all()
    CS.same_bytes(many, want, "T = 16")
    other = irt.contour_cells(f.value, None, f.lat, f.lon, [-0.6], [1], True)
    twice, per = run_grid(ctx, "smooth", True, [0.35, -0.6, 0.35], [3, 1, 3])
    assert per.tolist() == [one.size, other.size, one.size]
    CS.same_bytes(twice, np.concatenate([one, other, one]), "a threshold given twice")


def test_count_only_and_a_short_capacity_write_nothing(ctx):
    f, v, fd = device_field("holes")
    want, want_per = CS.host("holes", True)
    args = (v.data_ptr(), fd.data_ptr(), f.lat, f.lon, f.thresholds, f.styles)
    out = Out(want.size)
    n, per = ctx.contour_grid(*args, 0, out.capacity, True)  # d_out NULL: the capacity means nothing
    assert n == want.size and per.tolist() == want_per.tolist()
    out.host(0)
    with pytest.raises(irt.ContourError, match="capacity") as e:
        ctx.contour_grid(*args, out.ptr, want.size - 1, True)
    assert e.value.code == irt.E_INVALID and e.value.count == want.size
    assert e.value.counts[:4].tolist() == want_per.tolist()
    out.host(0)
    n, _ = ctx.contour_grid(*args, out.ptr, want.size, True)  # exactly enough
    CS.same_bytes(out.host(n), want, "capacity = count")


# ------------------------------------------------------------------ irt_contour_latlon
LATLON_GRID = ("poles", True)  # 33 x 64 wrapped, pole to pole


@pytest.mark.parametrize("mode", [irt.MODE_USER_GEOM, irt.MODE_CUBQL, irt.MODE_TRIANGLES], ids=["cells", "wedges", "triangles"])
def test_latlon_equals_the_two_calls_by_hand_and_the_host_definition(mode):
    import torch
    cells = S.scene(OS.SCENE)
    g = CS.field(LATLON_GRID[0])
    h0, top, _ = S.shell(cells)
    radius = F(0.5 * (float(h0) + float(top)))
    with irt.Context(cells, 0) as c:
        if mode != irt.MODE_USER_GEOM:
            c.build_wedge_accel(cells)
        value = torch.full((g.lat.size, g.lon.size), -7.0, dtype=torch.float32, device="cuda:0")
        found = torch.full((g.lat.size, g.lon.size), 9, dtype=torch.uint8, device="cuda:0")
        c.sample_latlon(g.lat, g.lon, [radius], value.data_ptr(), found.data_ptr(), mode, float("nan"))
        torch.cuda.synchronize()
        v, fd = value.cpu().numpy(), found.cpu().numpy()
        assert set(np.unique(fd)) <= {0, 1} and fd.sum() > fd.size // 2
        # the thresholds: five quantiles of the values found at this level
        thr = np.quantile(v[fd == 1].astype(np.float64), [0.2, 0.35, 0.5, 0.65, 0.8]).astype(F)
        sty = np.arange(5) % 2
        want, want_per = irt.contour_cells(v, fd, g.lat, g.lon, thr, sty, True, return_counts=True)
        print(f"mode {mode}: radius {radius}, thresholds {thr.tolist()}, {want.size} segments {want_per.tolist()}")
        assert want.size >= 100
        hand = Out(want.size + 2)
        n, per = c.contour_grid(value.data_ptr(), found.data_ptr(), g.lat, g.lon, thr, sty, hand.ptr, hand.capacity, True)
        by_hand = hand.host(n)
        out = Out(want.size + 2)
        n2, per2 = c.contour_latlon(g.lat, g.lon, radius, thr, sty, out.ptr, out.capacity, True, mode)
        got = out.host(n2)
        assert n == n2 == want.size and per.tolist() == per2.tolist() == want_per.tolist()
        CS.same_bytes(got, by_hand, f"mode {mode}: irt_contour_latlon against the two calls by hand")
        CS.same_bytes(got, want, f"mode {mode}: irt_contour_latlon against irt_contour_cells")
        n3, per3 = c.contour_latlon(g.lat, g.lon, radius, thr, sty, 0, 0, True, mode)  # count only
        assert n3 == n and per3.tolist() == per.tolist()


# ------------------------------------------------------------------ end to end: isolines in a frame
def test_contour_overlay_draws_the_isolines(ctx):
    import torch
    W, H = 64, 48
    f, v, _ = device_field("smooth")
    sty = np.arange(f.thresholds.size) % len(OS.STYLES)
    want = irt.contour_cells(f.value, None, f.lat, f.lon, f.thresholds, sty, True)
    cam = helpers.view_battery(S.scene(OS.SCENE))[OS.VIEWS["outside"]]
    lp = irt.setup_frame(S.scene(OS.SCENE), W, H, camera=cam).lp
    lp.accumID = 0
    R = OS.surface_radius()
    # the frame's points on the sphere, restated as overlay_scenes.frame_points restates them
    org = lp.camera12()[0:3]
    d = LS.rays(lp, W, H)
    hit, tn, tf = LS.sphere_hits(org, d, R)
    near = tn > 0
    live = hit & (near | (tf > 0))
    t = np.where(near, tn, tf).astype(F)
    P = (org[None, None, :] + d * t[..., None]).astype(F)
    ln = np.sqrt((P[..., 0] * P[..., 0] + P[..., 1] * P[..., 1]) + P[..., 2] * P[..., 2])
    with np.errstate(invalid="ignore", divide="ignore"):
        u = (P / ln[..., None]).astype(F)
    expect = np.full((H, W), -1, np.int32)
    expect[live] = irt.overlay_cover(want, OS.STYLES, u[live])
    assert (expect >= 0).sum() >= 1, "no pixel of the frame lies on an isoline"
    with ctx.contour_overlay(f.lat, f.lon, f.thresholds, OS.STYLES, 0, value=v, wrap=True) as ov:
        assert ov.num_segments == want.size
        CS.same_bytes(ov.segments, want, "contour_overlay's segments")
        cover = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0")
        fb = torch.zeros((H, W), dtype=torch.int32, device="cuda:0")
        seg = torch.full((H, W), -9, dtype=torch.int32, device="cuda:0")
        ctx.render_overlay(ov, lp, W, H, R, cover.data_ptr(), fb.data_ptr(), 0, seg.data_ptr())
        torch.cuda.synchronize()
        got = seg.cpu().numpy()
    print(f"{int((expect >= 0).sum())} of {W * H} pixels on an isoline, {want.size} segments")
    assert np.array_equal(got, expect), f"{int((got != expect).sum())} pixels differ"
    assert (cover.cpu().numpy()[expect >= 0][:, 3] > 0).all()


# ------------------------------------------------------------------ conduct
def test_conduct(ctx):
    import torch
    cells = S.scene(OS.SCENE)
    f, v, _ = device_field("smooth")
    want, want_per = CS.host("smooth", True)
    args = (v.data_ptr(), 0, f.lat, f.lon, f.thresholds, f.styles)
    out = Out(want.size)
    # refusals on the device call, nothing written
    with pytest.raises(irt.ContourError, match="64-byte aligned"):
        ctx.contour_grid(*args, out.ptr + 16, want.size, True)
    with pytest.raises(irt.ContourError, match="null d_value"):
        ctx.contour_grid(0, 0, f.lat, f.lon, f.thresholds, f.styles, out.ptr, want.size, True)
    with pytest.raises(irt.ContourError, match="at least 2 x 2"):  # no request has zero cells
        ctx.contour_grid(v.data_ptr(), 0, f.lat[:1], f.lon, f.thresholds, f.styles, out.ptr, want.size, True)
    with pytest.raises(irt.ContourError, match="closing step"):
        g = CS.field("smooth53")
        ctx.contour_grid(v.data_ptr(), 0, g.lat, g.lon, g.thresholds, g.styles, out.ptr, want.size, True)
    with pytest.raises(irt.ContourError, match="radius"):
        ctx.contour_latlon(f.lat, f.lon, float("nan"), f.thresholds, f.styles, out.ptr, want.size, True)
    # a pending update: refused, then fine after the commit
    ctx.update_values(np.ascontiguousarray(cells["value"]))
    with pytest.raises(irt.IrtError, match="update is pending"):
        ctx.contour_grid(*args, out.ptr, want.size, True)
    with pytest.raises(irt.IrtError, match="update is pending"):
        ctx.contour_latlon(f.lat, f.lon, 6.4e6, f.thresholds, f.styles, out.ptr, want.size, True)
    out.host(0)
    ctx.end_update()
    # a non-default stream
    s1 = torch.cuda.Stream(0)
    torch.cuda.synchronize()
    n, per = ctx.contour_grid(*args, out.ptr, want.size, True, s1.cuda_stream)
    s1.synchronize()
    assert per.tolist() == want_per.tolist()
    CS.same_bytes(out.host(n), want, "on a non-default stream")
    # a second context: its call leaves this context's output alone, and this context's next call its
    with irt.Context(cells, 0) as other:
        g, gv, gfd = device_field("holes")
        gwant, _ = CS.host("holes", False)
        theirs = Out(gwant.size)
        m, _ = other.contour_grid(gv.data_ptr(), gfd.data_ptr(), g.lat, g.lon, g.thresholds, g.styles, theirs.ptr,
                                  theirs.capacity, False)
        CS.same_bytes(theirs.host(m), gwant, "the second context")
        CS.same_bytes(out.host(n), want, "the first context's output after the second's call")
        again = Out(want.size)
        n2, _ = ctx.contour_grid(*args, again.ptr, want.size, True)
        CS.same_bytes(again.host(n2), want, "the first context again")
        CS.same_bytes(theirs.host(m), gwant, "the second context's output after the first's call")
