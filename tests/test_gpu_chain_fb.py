"""fb of chained progressive frames: only the launch's last frame converts and stores RGBA8.

In a chained launch of consecutive progressive frames of one camera (irt_render_accumulate, the
tile and tile-list forms) every frame stores accum -- the hand-off to the next frame -- but a
frame that is not the launch's last leaves fb alone: a later frame overwrites the bytes before
anything reads them.  A pixel whose ray misses the world box in the last frame (the raygen then
writes nothing, deviceCode.cu:294-295) gets the bytes of the launch's latest earlier hit from the
last frame's lane, which replays the earlier frames' rays; a pixel no frame hit stays untouched.

Here: fb and accum after the launch, byte for byte, against F single irt_render launches with
the same accumIDs -- whole frames (one whose size cuts 8x8 packets), packed tile lists, the
terrain (miss-mode) kernel, and a camera whose frame the box's silhouette crosses, where the
oracle's box test (on the CPU) says which pixels hit in which frames.  Single-frame launches and
sequences of views keep the pixel write they had.
"""
import functools

import numpy as np
import pytest

import irt
import oracle as O
from helpers import FRAMING, bits

pytestmark = pytest.mark.gpu

SENTINEL = 0xDEADBEEF
VIEW_ALL = None  # Camera::viewAll, fovy 90: the box's silhouette crosses the frame


def _buffers(n, fill):
    import torch
    fb = torch.full((n,), int(np.uint32(fill).view(np.int32)), dtype=torch.int32, device="cuda")
    acc = torch.zeros(n * 4, dtype=torch.float32, device="cuda")
    return fb, acc


def _host(fb, acc):
    import torch
    torch.cuda.synchronize()
    return fb.cpu().numpy().view(np.uint32).copy(), bits(acc.cpu().numpy())


def _singles(ctx, lp, W, H, first, F, fill=0):
    """F single-frame irt_render launches, accumIDs first .. first + F - 1."""
    fb, acc = _buffers(W * H, fill)
    for aid in range(first, first + F):
        lp.accumID = aid
        ctx.render(lp, W, H, fb.data_ptr(), acc.data_ptr())
    return _host(fb, acc)


def _chained(ctx, lp, W, H, first, F, fill=0):
    """The same frames in one irt_render_accumulate launch."""
    fb, acc = _buffers(W * H, fill)
    lp.accumID = first
    ctx.render_accumulate(lp, W, H, F, fb.data_ptr(), acc.data_ptr())
    return _host(fb, acc)


NOMISS_BIT = 262144  # irt.default_kernel_id: the hole-free form of the default kernel


@functools.lru_cache(maxsize=None)
def _cells(terrain=0.0):
    cells = irt.synth_grid(2, 2, 47, terrain=terrain)
    cells.setflags(write=False)
    return cells


def _flat():
    return _cells()


@pytest.fixture(scope="module")
def flat_ctx():
    ctx = irt.Context(_flat(), 0)
    lut, vr = irt.default_transfunc((ctx.info.dataRange.lower, ctx.info.dataRange.upper))
    ctx.set_transfunc(lut, vr)
    assert irt.default_kernel_id(ctx) & NOMISS_BIT, "not the hole-free kernel"
    yield ctx
    assert ctx.chain_errors() == 0
    ctx.close()


@functools.lru_cache(maxsize=None)
def _box_hits(W, H, first, F, terrain=0.0):
    """(F, H, W) bool from the oracle on the CPU: frame first + f's ray of the pixel passes the
    box test.  Each frame rendered on its own over a sentinel fb: the raygen returns before it
    writes anything exactly when boxTest fails (deviceCode.cu:294-295)."""
    S = O.OracleScene(_cells(terrain))
    lut, vr = S.default_lut()
    S.set_transfunc(lut, vr)
    cam = S.camera(W, H, VIEW_ALL)
    hits = np.zeros((F, H, W), bool)
    for f in range(F):
        fb = np.full((H, W), SENTINEL, np.uint32)
        _, fb, st = S.render(S.params(cam, accum_id=first + f), W, H, fb=fb)
        hits[f] = fb != SENTINEL
        assert int(hits[f].sum()) == st.rays_in_box  # (no hit pixel wrote the sentinel's bytes)
    hits.setflags(write=False)
    return hits


@pytest.mark.parametrize("first", [0, 5])
@pytest.mark.parametrize("F", [1, 2, 3, 8])
@pytest.mark.parametrize("W,H,cam", [(96, 80, FRAMING), (100, 70, VIEW_ALL)])
def test_chained_launch_equals_single_frames(flat_ctx, W, H, cam, F, first):
    """Whole frames: 96x80, and 100x70, whose edges cut 8x8 packets and whose camera has rays
    that hit the box in some frames only; F = 1 is a single-frame launch."""
    setup = irt.setup_frame(_flat(), W, H, camera=cam)
    ref = _singles(flat_ctx, setup.lp, W, H, first, F)
    got = _chained(flat_ctx, setup.lp, W, H, first, F)
    assert np.array_equal(got[1], ref[1]), "accum"
    assert np.array_equal(got[0], ref[0]), "fb"


def _unpack(packed, tiles, W, H, fill, per=1):
    """Packed tiles (list order, 64x64 each, `per` words per pixel) -> the frame; pixels of no
    listed tile hold `fill`."""
    tx = (W + 63) // 64
    out = np.full((H, W, per), fill, packed.dtype)
    t = packed.reshape(len(tiles), 64, 64, per)
    for k, tid in enumerate(tiles):
        x0, y0 = (tid % tx) * 64, (tid // tx) * 64
        h, w = min(64, H - y0), min(64, W - x0)
        out[y0:y0 + h, x0:x0 + w] = t[k, :h, :w]
    return out


@pytest.mark.parametrize("F,first", [(3, 0), (8, 2)])
def test_packed_tile_lists_of_two_ranks(flat_ctx, F, first):
    """irt_render_tile_list, chained: two ranks' tile lists (a frame's tiles dealt alternately,
    out of order) over a sentinel, each rank's packed fb and accum unpacked against the frame of F
    single irt_render launches; pixels of a rank's buffer outside the frame stay untouched."""
    W, H = 200, 136  # 4 x 3 tiles, the right column and bottom row cut
    setup = irt.setup_frame(_flat(), W, H, camera=VIEW_ALL)
    ref_fb, ref_acc = _singles(flat_ctx, setup.lp, W, H, first, F, fill=SENTINEL)
    ref_fb, ref_acc = ref_fb.reshape(H, W, 1), ref_acc.reshape(H, W, 4)
    hits = _box_hits(W, H, first, F)
    ranks = [np.array([10, 0, 6, 2, 8, 4], np.int32), np.array([1, 11, 5, 3, 9, 7], np.int32)]
    for tiles in ranks:
        n = len(tiles) * 4096
        fb, acc = _buffers(n, SENTINEL)
        setup.lp.accumID = first
        flat_ctx.render_tile_list(setup.lp, W, H, tiles, F, fb.data_ptr(), acc.data_ptr())
        pf, pa = _host(fb, acc)
        mine = _unpack(np.ones(n, np.uint32), tiles, W, H, 0)[..., 0] == 1
        # the replay in packed form: this rank holds a pixel that misses last after an earlier hit
        assert (hits.any(0) & ~hits[-1] & mine).any()
        got_fb = _unpack(pf, tiles, W, H, 0)
        got_acc = _unpack(pa, tiles, W, H, 0, per=4)
        assert np.array_equal(got_acc[mine], ref_acc[mine]), "accum"
        assert np.array_equal(got_fb[mine], ref_fb[mine]), "fb"
        # what lies outside the frame in a cut tile belongs to no pixel: nothing written
        ys, xs = np.mgrid[0:64, 0:64]
        cut = 0
        for k, tid in enumerate(tiles):
            outside = ((tid % 4) * 64 + xs >= W) | ((tid // 4) * 64 + ys >= H)
            cut += int(outside.sum())
            assert np.all(pf.reshape(-1, 64, 64)[k][outside] == SENTINEL)
        assert cut > 0


@pytest.mark.parametrize("F", [3, 8])
def test_terrain_kernel(F):
    """The miss-mode kernel (a terrain grid: voids under land) runs the same epilogue."""
    cells = _cells(4000.0)
    W, H = 96, 80
    hits = _box_hits(W, H, 0, F, terrain=4000.0)
    assert (hits.any(0) & ~hits[-1]).any(), "no pixel misses the box in the last frame after an earlier hit"
    setup = irt.setup_frame(cells, W, H, camera=VIEW_ALL)
    ctx = irt.Context(cells, 0)
    ctx.set_transfunc(setup.lut, setup.value_range)
    assert irt.default_kernel_id(ctx) & NOMISS_BIT == 0, "not the miss-mode kernel"
    ref = _singles(ctx, setup.lp, W, H, 0, F, fill=SENTINEL)
    got = _chained(ctx, setup.lp, W, H, 0, F, fill=SENTINEL)
    assert np.array_equal(got[1], ref[1]), "accum"
    assert np.array_equal(got[0], ref[0]), "fb"
    assert ctx.chain_errors() == 0
    ctx.close()


@pytest.mark.parametrize("fill", [0, SENTINEL])
@pytest.mark.parametrize("F,first", [(3, 0), (8, 0), (8, 5)])
def test_box_silhouette_across_the_frame(flat_ctx, F, first, fill):
    """Pixels on the box's silhouette hit the box in some frames of the launch and miss it in
    others (the jitter moves the ray).  The oracle's box test picks them out: the launch must
    hold a pixel that misses in its last frame after hitting earlier -- its fb is the earlier
    frame's, which only the last frame's lane can write now -- and pixels no frame hits, which
    must keep what fb held before the launch."""
    W, H = 96, 80
    hits = _box_hits(W, H, first, F)
    ever, last = hits.any(0), hits[-1]
    late_miss = ever & ~last
    assert late_miss.any(), "no pixel misses the box in the last frame after an earlier hit"
    assert (~ever).any() and (hits[:-1].any(0) & last).any() and (~hits[:-1].any(0) & last).any()
    setup = irt.setup_frame(_flat(), W, H, camera=VIEW_ALL)
    ref = _singles(flat_ctx, setup.lp, W, H, first, F, fill=fill)
    got = _chained(flat_ctx, setup.lp, W, H, first, F, fill=fill)
    assert np.array_equal(got[1], ref[1]), "accum"
    gfb, rfb = got[0].reshape(H, W), ref[0].reshape(H, W)
    assert np.array_equal(gfb[late_miss], rfb[late_miss]), "fb of a last-frame miss after a hit"
    assert np.array_equal(gfb, rfb), "fb"
    assert np.all(gfb[~ever] == fill), "a pixel no frame hit was written"
    assert np.all(got[1].reshape(H, W, 4)[~ever] == 0)
    if fill == SENTINEL:
        assert np.all(gfb[ever] != SENTINEL)


def _orbit(setup, W, H, n):
    """n views on an orbit close enough that the box's silhouette is in the frame and moves."""
    out = []
    for k in range(n):
        th = 2.0 * np.pi * k / 24.0
        c = irt.camera_look_at((1.4e7 * np.sin(th), 0.0, 1.4e7 * np.cos(th)), (0.0, 0.0, 0.0),
                               (0.0, 1.0, 0.0), 60.0, W, H)
        q = irt.LaunchParams.from_buffer_copy(setup.lp)
        q.org, q.dir_00, q.dir_du, q.dir_dv = c.org, c.dir_00, c.dir_du, c.dir_dv
        q.accumID = 0
        out.append(q)
    return out


def test_single_frames_and_view_sequences_keep_their_fb(flat_ctx):
    """A sequence of views (each view an image of its own: a pixel a later view's ray misses
    keeps the earlier view's bytes) writes fb in every frame, as single-frame launches do: after
    1 .. n views of one chained launch, fb and accum equal the views rendered one irt_render each."""
    W, H, n = 96, 80, 4
    setup = irt.setup_frame(_flat(), W, H, camera=FRAMING)
    lps = _orbit(setup, W, H, n)
    # each view's box hits, from a launch of its own over a sentinel: some pixel must miss in
    # the last view after hitting in an earlier one
    hit = []
    for q in lps:
        fb, acc = _buffers(W * H, SENTINEL)
        flat_ctx.render(q, W, H, fb.data_ptr(), acc.data_ptr())
        hit.append(_host(fb, acc)[0] != SENTINEL)
    assert (np.any(hit[:-1], axis=0) & ~hit[-1]).any()
    fb, acc = _buffers(W * H, SENTINEL)
    ref = []
    for q in lps:
        flat_ctx.render(q, W, H, fb.data_ptr(), acc.data_ptr())
        ref.append(_host(fb, acc))
    for m in range(1, n + 1):
        fb, acc = _buffers(W * H, SENTINEL)
        flat_ctx.render_sequence(lps[:m], W, H, fb.data_ptr(), acc.data_ptr())
        got = _host(fb, acc)
        assert np.array_equal(got[1], ref[m - 1][1]), ("accum", m)
        assert np.array_equal(got[0], ref[m - 1][0]), ("fb", m)
