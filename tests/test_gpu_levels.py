"""irt_render_levels on the device (csrc/irt_levels.hip) against the restatement of its definition
(tests/levels_scenes.py), bit for bit: fb, the four floats of accum, d_value where a value was
found (missValue elsewhere) and d_level, on the frames tests/test_levels_cpu.py takes its census
of.  Every output goes to a buffer pre-filled with a sentinel, with guard words on both sides."""
import ctypes as C

import numpy as np
import pytest

import irt
import levels_scenes as LS
import sample_scenes as S

pytestmark = pytest.mark.gpu

GUARD = 96
SENT = 0x5EADBEEF  # as a float a large finite number; as an int32 positive and no level index
F = np.float32


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


class Frame:
    """fb, accum, value and level device buffers of W x H pixels between guards, sentinel-filled."""

    def __init__(self, W, H, device=0, prior=None):
        import torch
        self.torch, self.W, self.H, self.n = torch, W, H, W * H
        mk = lambda per: torch.full(((self.n + 2 * GUARD) * per,), SENT, dtype=torch.int32,  # noqa: E731
                                    device=f"cuda:{device}")
        self.fb, self.accum, self.value, self.level = mk(1), mk(4), mk(1), mk(1)
        if prior is not None:
            self.set_accum(prior)

    def set_accum(self, a):
        t = self.torch.from_numpy(np.ascontiguousarray(a, F).reshape(-1).view(np.int32).copy())
        self.accum[4 * GUARD:4 * (GUARD + self.n)] = t.to(self.accum.device)

    def ptr(self, which):
        t = getattr(self, which)
        return t.data_ptr() + 4 * GUARD * (4 if which == "accum" else 1)

    def host(self, which, written=True):
        per = 4 if which == "accum" else 1
        v = getattr(self, which).cpu().numpy().view(np.uint32)
        lo, hi = GUARD * per, (GUARD + self.n) * per
        assert (v[:lo] == SENT).all() and (v[hi:] == SENT).all(), f"{which} guards"
        v = v[lo:hi]
        assert written or (v == SENT).all(), f"{which} was written"
        return v.reshape((self.H, self.W, 4) if per == 4 else (self.H, self.W))


def make_context(name, tf_name, mode=irt.MODE_USER_GEOM):
    cells = S.scene(name)
    ctx = irt.Context(cells, 0)
    lut, vr, scale = LS.transfunc(name, tf_name)
    ctx.set_transfunc(lut, vr, scale)
    if mode != irt.MODE_USER_GEOM:
        ctx.build_wedge_accel(cells)
    return ctx


def render(ctx, frame, lp, radii, back=False, value=True, level=True, stream=0):
    ctx.render_levels(lp, frame.W, frame.H, radii, frame.ptr("fb"), frame.ptr("accum"),
                      frame.ptr("value") if value else 0, frame.ptr("level") if level else 0, back, LS.MISS, stream)
    frame.torch.cuda.synchronize(ctx.device)


def check(frame, want, what, value=True, level=True):
    """The frame's four outputs against the restatement's, as bits."""
    for which, exp in (("fb", want.fb), ("accum", want.accum), ("value", want.value), ("level", want.level)):
        written = {"value": value, "level": level}.get(which, True)
        got = frame.host(which, written)
        if not written:
            continue
        bad = np.argwhere(got != bits(exp).reshape(got.shape))
        assert len(bad) == 0, (f"{what}: {which} differs at {len(bad)} places, first {tuple(bad[0])}: "
                               f"{hex(int(got[tuple(bad[0])]))} vs {hex(int(bits(exp).reshape(got.shape)[tuple(bad[0])]))}")


def run_case(ctx, case, mode=irt.MODE_USER_GEOM):
    name, view_name, levels, tf_name, size, back, accum_id = case
    W, H = LS.SIZES[size]
    want = LS.expected(*case, mode=mode)
    frame = Frame(W, H, prior=LS.prior_accum(W, H) if accum_id else np.zeros((H, W, 4), F))
    render(ctx, frame, LS.launch_params(name, view_name, size, accum_id, mode), LS.levels_of(name, levels), back)
    print(f"{LS.case_id(case)}: {int((want.level >= 0).sum())} of {W * H} pixels found a value")
    check(frame, want, LS.case_id(case))


# ------------------------------------------------------------------ bit equality
@pytest.mark.parametrize("slots", [False, True], ids=["headers", "slots"])
@pytest.mark.parametrize("case", LS.CASES, ids=LS.case_id)
def test_levels_frames_equal_the_restatement(monkeypatch, case, slots):
    """From headers and (IRT_SLOTS=1) from the slot table, where the scene has one (the terrain
    scene's cells have more than three edges: no table, the header form again)."""
    if slots:
        monkeypatch.setenv("IRT_SLOTS", "1")
    with make_context(case[0], case[3]) as ctx:
        assert (ctx.array_bytes("slots") > 0) == (slots and case[0] != "terrain")
        run_case(ctx, case)


SAMPLER_CASES = (("filtered", "outside", "four", "translucent", "odd", True, 0),
                 ("filtered", "inside", "four", "scale3", "odd", True, 3))


@pytest.mark.parametrize("mode", ["cubql", "triangles"])
@pytest.mark.parametrize("case", SAMPLER_CASES, ids=LS.case_id)
def test_levels_frames_of_the_unstructured_samplers(case, mode):
    m = {"cubql": irt.MODE_CUBQL, "triangles": irt.MODE_TRIANGLES}[mode]
    want = LS.expected(*case, mode=m)
    assert (want.level >= 0).sum() >= 40 and not np.isnan(want.value).any()
    with make_context(case[0], case[3], m) as ctx:
        run_case(ctx, case, m)


# ------------------------------------------------------------------ an overlay's probe values
@pytest.mark.parametrize("name,view_name", [("flat", "outside"), ("terrain", "inside"), ("filtered", "under")])
def test_one_opaque_level_holds_the_sampled_values(name, view_name):
    """One level, alpha 1, accumID 0: d_value of every pixel is irt_sample_points' answer at the
    restatement's hit point of that pixel (near hit, or far hit from inside), bit for bit."""
    import torch
    W, H = LS.SIZES["odd"]
    radii = LS.levels_of(name, "midlayer")
    lp = LS.launch_params(name, view_name, "odd")
    r = LS.composite(S.scene(name), lp, W, H, radii, LS.transfunc(name, "opaque"), False)
    near, far = r.slots
    assert not (near.live & far.live).any()
    live = near.live | far.live
    pts = np.where(near.live[..., None], near.points, far.points)[live]
    with make_context(name, "opaque") as ctx:
        frame = Frame(W, H, prior=np.zeros((H, W, 4), F))
        render(ctx, frame, lp, radii)
        xyz = torch.from_numpy(np.ascontiguousarray(pts, F)).to("cuda:0")
        val = torch.zeros(len(pts), dtype=torch.float32, device="cuda:0")
        ctx.sample_points(xyz.data_ptr(), len(pts), val.data_ptr(), 0, irt.MODE_USER_GEOM, LS.MISS)
        torch.cuda.synchronize(0)
        want = np.full((H, W), LS.MISS, F)
        want[live] = val.cpu().numpy()
        assert (want != F(LS.MISS)).sum() >= 100
        assert np.array_equal(frame.host("value"), bits(want))
        a = frame.host("accum").view(F)[..., 3]
        assert np.array_equal(a == 1, want != F(LS.MISS)) and np.isin(a, (0, 1)).all()


# ------------------------------------------------------------------ NULL outputs
def test_null_value_or_level_leaves_the_rest_unchanged():
    case = ("flat", "inside", "four", "scale3", "odd", True, 3)
    W, H = LS.SIZES["odd"]
    want = LS.expected(*case)
    with make_context("flat", "scale3") as ctx:
        for value, level in ((False, True), (True, False), (False, False)):
            frame = Frame(W, H, prior=LS.prior_accum(W, H))
            render(ctx, frame, LS.launch_params("flat", "inside", "odd", 3), LS.levels_of("flat", "four"), True,
                   value, level)
            check(frame, want, f"value {value} level {level}", value, level)


# ------------------------------------------------------------------ progressive accumulation
def test_four_progressive_frames_are_the_four_lerps_in_order():
    name, view_name, levels, tf_name = "terrain", "outside", "four", "translucent"
    W, H = LS.SIZES["odd"]
    accum = np.zeros((H, W, 4), F)
    with make_context(name, tf_name) as ctx:
        frame = Frame(W, H, prior=accum)
        for aid in range(4):
            lp = LS.launch_params(name, view_name, "odd", aid)
            r = LS.composite(S.scene(name), lp, W, H, LS.levels_of(name, levels), LS.transfunc(name, tf_name), True)
            accum = LS.lerp(r.colour, accum, aid)
            render(ctx, frame, lp, LS.levels_of(name, levels), True)
            assert np.array_equal(frame.host("accum"), bits(accum)), f"accumID {aid}"
            assert np.array_equal(frame.host("fb"), LS.pixels(accum)), f"accumID {aid}"
            assert np.array_equal(frame.host("level"), bits(r.level)), f"accumID {aid}"
    assert len({LS.rays(LS.launch_params(name, view_name, "odd", a), W, H).tobytes() for a in range(4)}) == 4


# ------------------------------------------------------------------ the order of radius
def test_permuting_radius_changes_only_the_level_indices():
    name, W, H = "flat", *LS.SIZES["odd"]
    base = np.array(LS.levels_of(name, "four"), F)
    dup = np.array(LS.levels_of(name, "dup"), F)
    lp = LS.launch_params(name, "inside", "odd")
    with make_context(name, "translucent") as ctx:
        def frame_of(radii):
            fr = Frame(W, H, prior=np.zeros((H, W, 4), F))
            render(ctx, fr, lp, radii, True)
            return [fr.host(w).copy() for w in ("fb", "accum", "value", "level")]

        ref = frame_of(base)
        assert np.unique(ref[3].view(np.int32)).size >= 2
        for perm in ([3, 2, 1, 0], [1, 3, 0, 2]):
            got = frame_of(base[perm])
            for k in range(3):
                assert np.array_equal(got[k], ref[k])
            lv = got[3].view(np.int32)
            back_map = np.where(lv >= 0, np.array(perm, np.int32)[np.maximum(lv, 0)], -1)
            assert np.array_equal(back_map, ref[3].view(np.int32))
        # a duplicated radius: the lower index is seen first from outside it, the higher from inside
        lv = frame_of(dup)[3].view(np.int32)  # dup = (a, b, a) with a > b, the camera between them
        want = LS.composite(S.scene(name), lp, W, H, dup, LS.transfunc(name, "translucent"), True).level
        assert np.array_equal(lv, want) and 2 in lv and 1 in lv and 0 not in lv
        lv = frame_of(dup[[1, 0, 2]])[3].view(np.int32)  # (b, a, a)
        assert 2 in lv and 0 in lv and 1 not in lv


# ------------------------------------------------------------------ errors
def test_every_listed_error_is_refused_and_writes_nothing():
    import torch
    W, H = 8, 8
    cells = S.scene("flat")
    lp = LS.launch_params("flat", "outside", "packet")
    good = np.array(LS.levels_of("flat", "four"), F)
    L = irt.lib()
    frame = Frame(W, H)

    def call(h, lp=lp, w=W, hgt=H, radii=good, n=None, flags=0, fb=True, accum=True):
        r = np.ascontiguousarray(radii, F) if radii is not None else None
        return L.irt_render_levels(h, C.byref(lp) if lp is not None else None, w, hgt,
                                   C.c_void_p(r.ctypes.data) if r is not None else None,
                                   len(r) if n is None else n, flags,
                                   C.c_void_p(frame.ptr("fb")) if fb else None,
                                   C.c_void_p(frame.ptr("accum")) if accum else None,
                                   C.c_void_p(frame.ptr("value")), C.c_void_p(frame.ptr("level")), LS.MISS, None)

    def refused(rc, word):
        assert rc == irt.E_INVALID
        assert word in L.irt_last_error().decode(), L.irt_last_error()

    refused(call(None), "null context")
    with irt.Context(cells, 0) as ctx:
        refused(call(ctx._h), "no transfer function")
        lut, vr, scale = LS.transfunc("flat", "default")
        ctx.set_transfunc(lut, vr, scale)
        for mode in (irt.MODE_CUBQL, irt.MODE_TRIANGLES):
            bad = LS.launch_params("flat", "outside", "packet", mode=mode)
            refused(call(ctx._h, lp=bad), "irt_build_wedge_accel")
        refused(call(ctx._h, lp=LS.launch_params("flat", "outside", "packet", mode=7)), "sampler mode 7")
        refused(call(ctx._h, n=0), "levels")
        refused(call(ctx._h, n=-1), "levels")
        refused(call(ctx._h, radii=np.full(17, 6.4e6, F)), "levels")
        for r in (0.0, -6.4e6, np.nan, np.inf, -np.inf):
            refused(call(ctx._h, radii=[good[0], r, good[1]]), "radius[1]")
        refused(call(ctx._h, flags=2), "flag")
        refused(call(ctx._h, flags=-1), "flag")
        for w, h in ((0, 8), (8, 0), (-3, 8), (1 << 14, 1 << 13), (1 << 27, 1)):
            refused(call(ctx._h, w=w, hgt=h), "pixels")
        refused(call(ctx._h, lp=None), "null lp")
        refused(call(ctx._h, radii=None, n=4), "null radius")
        refused(call(ctx._h, fb=False), "null d_fb or d_accum")
        refused(call(ctx._h, accum=False), "null d_fb or d_accum")
        with pytest.raises(irt.IrtError):  # ... and the binding's own check of the radii
            ctx.render_levels(lp, W, H, [6.4e6, -1.0], frame.ptr("fb"), frame.ptr("accum"))
        ctx.update_values(np.ascontiguousarray(cells["value"]))
        refused(call(ctx._h), "update is pending")
        ctx.end_update()
        torch.cuda.synchronize(0)
        for which in ("fb", "accum", "value", "level"):
            frame.host(which, written=False)
        assert call(ctx._h) == 0  # the same call, now valid
        torch.cuda.synchronize(0)
        assert (frame.host("fb") != SENT).all()
    h = C.c_void_p()  # a context still being created; then completed and destroyed as usual
    assert L.irt_create_begin(cells.size, 0, C.byref(h)) == 0
    refused(call(h), "still being created")
    assert L.irt_create_append(h, C.c_void_p(cells.ctypes.data), cells.size) == 0 and L.irt_create_end(h) == 0
    L.irt_destroy(h)
    torch.cuda.synchronize(0)
    for which in ("value", "level"):
        assert (frame.host(which) != SENT).all()  # (the valid call's; the guards once more)


# ------------------------------------------------------------------ updates and the transfer function
def test_levels_follow_value_updates_and_the_transfer_function():
    case = ("flat", "outside", "four", "translucent", "odd", True, 0)
    name, view_name, levels, tf_name, size, back, _ = case
    W, H = LS.SIZES[size]
    cells = np.array(S.scene(name), copy=True)
    new = np.array(cells, copy=True)
    new["value"] = (1.0 - cells["value"][::-1]) * F(0.75) + F(0.125)
    lp, radii = LS.launch_params(name, view_name, size), LS.levels_of(name, levels)
    zero = np.zeros((H, W, 4), F)

    def want(c, tf):
        r = LS.composite(c, lp, W, H, radii, LS.transfunc(name, tf), back)
        r.accum = LS.lerp(r.colour, zero, 0)
        r.fb = LS.pixels(r.accum)
        return r

    before, after, retf = want(cells, tf_name), want(new, tf_name), want(new, "scale3")
    assert not np.array_equal(before.fb, after.fb) and not np.array_equal(after.fb, retf.fb)
    with make_context(name, tf_name) as ctx:
        frame = Frame(W, H, prior=zero)
        render(ctx, frame, lp, radii, back)
        check(frame, before, "before the update")
        ctx.update_values(np.ascontiguousarray(new["value"]))
        frame = Frame(W, H, prior=zero)
        with pytest.raises(irt.IrtError, match="update is pending") as e:
            render(ctx, frame, lp, radii, back)
        assert e.value.code == irt.E_INVALID
        frame.torch.cuda.synchronize(0)
        for which in ("fb", "value", "level"):
            frame.host(which, written=False)
        ctx.end_update()
        render(ctx, frame, lp, radii, back)
        check(frame, after, "after the update")
        lut, vr, scale = LS.transfunc(name, "scale3")
        ctx.set_transfunc(lut, vr, scale)
        frame = Frame(W, H, prior=zero)
        render(ctx, frame, lp, radii, back)
        check(frame, retf, "after irt_set_transfunc")


# ------------------------------------------------------------------ streams
def test_a_levels_call_on_a_second_stream_after_a_sampling_call():
    import torch
    case = ("filtered", "outside", "sixteen", "translucent", "odd", True, 0)
    W, H = LS.SIZES["odd"]
    want = LS.expected(*case)
    pts = S.points("filtered")
    with make_context("filtered", "translucent") as ctx:
        s1, s2 = torch.cuda.Stream(0), torch.cuda.Stream(0)
        xyz = torch.from_numpy(np.ascontiguousarray(np.tile(pts, (64, 1)))).to("cuda:0")
        val = torch.zeros(len(xyz), dtype=torch.float32, device="cuda:0")
        frame = Frame(W, H, prior=np.zeros((H, W, 4), F))
        torch.cuda.synchronize(0)
        ctx.sample_points(xyz.data_ptr(), len(xyz), val.data_ptr(), 0, irt.MODE_USER_GEOM, LS.MISS, s1.cuda_stream)
        render(ctx, frame, LS.launch_params("filtered", "outside", "odd"), LS.levels_of("filtered", "sixteen"), True,
               stream=s2.cuda_stream)
        check(frame, want, "on the second stream")
        f, v = S.cell_answers("filtered")
        got = val.cpu().numpy()[:len(pts)]
        assert np.array_equal(bits(got), bits(np.where(f != 0, v, F(LS.MISS))))


# ------------------------------------------------------------------ rendering is untouched
def test_levels_calls_leave_rendering_alone():
    from helpers import FRAMING, GpuFrame
    cells = S.scene("flat")
    setup = irt.setup_frame(cells, 64, 64, camera=FRAMING)
    W, H = LS.SIZES["odd"]
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
        lv = Frame(W, H, prior=np.zeros((H, W, 4), F))
        for back in (False, True):
            render(ctx, lv, LS.launch_params("flat", "outside", "odd"), LS.levels_of("flat", "four"), back)
        assert ctx.stats_total()[1] == launches
        assert tuple(ctx.stats().asdict()[k] for k in keys) == before[2]
        after = frame()
        assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
        assert before[2] == after[2] and before[2][2] > 0
        assert ctx.chain_errors() == 0


# ------------------------------------------------------------------ the app
def test_icon_rt_levels_flags(tmp_path):
    """icon_rt --levels r0,r1,... --levels-back: the frame loop calls irt_render_levels in place of
    irt_render, and the dumped framebuffer is the restatement's frame (the app's ambient terms are
    1, its transfer function the default one, its one frame accumID 0 onto the cleared buffers)."""
    import os
    import subprocess
    name, W, H = "flat", *LS.SIZES["odd"]
    cells = S.scene(name)
    ic, raw = str(tmp_path / "flat.ic"), str(tmp_path / "fb.raw")
    irt.save_ic(ic, np.array(cells, copy=True))
    vp, vi, vu, fovy = LS.view(name, "outside")
    radii = LS.levels_of(name, "four")
    cmd = [os.path.join(os.path.dirname(irt.LIB_PATH), "icon_rt"), ic, "--size", str(W), str(H), "--true-size",
           "--camera", *[repr(float(v)) for v in (*vp, *vi, *vu)], "-fovy", repr(float(fovy)),
           "--levels", ",".join(repr(float(r)) for r in radii), "--levels-back", "--dump-fb", raw]
    out = subprocess.run(cmd, cwd=tmp_path, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    lp = irt.setup_frame(cells, W, H, camera=(vp, vi, vu, fovy)).lp
    r = LS.composite(cells, lp, W, H, radii, LS.transfunc(name, "default"), True)
    accum = LS.lerp(r.colour, np.zeros((H, W, 4), F), 0)
    fb = np.fromfile(raw, np.uint32).reshape(H, W)
    assert np.array_equal(fb, LS.pixels(accum)) and np.unique(fb).size > 8
