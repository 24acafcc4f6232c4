"""The packet classifier on the device, over cameras and boxes of classifier_cameras' battery that
no other device test renders: a far eye (71.5 R), an eye just above the shell (1.0011 R), an
axis-aligned view (the centre rays under the 1e-5 clamp), a rolled off-centre view, both eyes of the
lat/lon window (a context created from the filtered records: the box does not contain the sphere;
WINDOW_EYE has no void packet at 96x72, so its launches carry no void data and must classify
nothing, and it is the second eye, with 17 void and 16 interior packets, that takes the interior
packets certified by section 4(c)'s second rule through the kernel),
the terrain scene (the bitmap form), ragged frames, a tile list and four of the seeded random
cameras; and the two cameras just beyond the certificate's limits, which must classify nothing.

test_gpu_interior._run's procedure: three chained launches of 4 frames of one camera (the
classification applies from the second) against a second context that renders the same accumIDs one
irt_render per frame and never classifies -- accum bits, fb bytes and the five event counts after
every launch; the use queries against the host bitmaps test_classifier_sweep_cpu.py certifies.  The
far camera and a window eye also against the oracle's frames.  Every case is a normal render.
"""
import functools

import numpy as np
import pytest

import classifier_cameras as CC
import irt
from helpers import bits, oracle_frame

pytestmark = pytest.mark.gpu

F = 4
LAUNCHES = 3
VOID_BITMAP, VOID_LIST = 16, 64  # irt_kernels.h OPT_*: kernel id bits of the void data's two forms

CASES = [
    ("P71.5", "flat", 96, 72, None),
    ("P1.0011", "flat", 96, 72, None),
    ("axis+z", "flat", 96, 72, None),
    ("roll30look", "flat", 96, 72, None),
    ("window", "window", 96, 72, None),
    ("window2", "window", 96, 72, None),
    ("P3", "terrain", 96, 72, None),
    ("P3", "flat", 203, 71, None),
    ("look0.8", "flat", 67, 33, None),
    ("P3", "flat", 96, 72, (3, 0)),
    ("random01", "flat", 96, 72, None),
    ("random04", "flat", 96, 72, None),
    ("random14", "flat", 96, 72, None),
    ("random23", "flat", 96, 72, None),
    ("P1.0009", "flat", 96, 72, None),
    ("P72.5", "flat", 96, 72, None),
]


def _context(scene):
    ctx = irt.Context(CC.cells(scene), 0)
    lut, vr = irt.default_transfunc((ctx.info.dataRange.lower, ctx.info.dataRange.upper))
    ctx.set_transfunc(lut, vr)
    return ctx


def _buffers(pixels):
    import torch
    return torch.zeros(pixels, dtype=torch.int32).cuda(), torch.zeros(pixels * 4, dtype=torch.float32).cuda()


def _host(fb, acc):
    import torch
    torch.cuda.synchronize()
    return fb.cpu().numpy().view(np.uint32).copy(), bits(acc.cpu().numpy())


def _counts(st):
    return np.array((st.raysLaunched, st.raysInBox, st.locateCalls, st.samplesFound, st.candidatesTested), np.int64)


@functools.lru_cache(maxsize=None)
def _run(name, scene, W, H, tiles):
    """Returns (the kernel ids of the classified launches, the first launch's fb, accum bits and
    counts)."""
    lp = CC.launch_params(name, scene, W, H)
    chained, single = _context(scene), _context(scene)
    try:
        return _compare(name, lp, chained, single, W, H, tiles)
    finally:
        chained.close()
        single.close()


def _compare(name, lp, chained, single, W, H, tiles):
    sel = {} if tiles is None else {"tiles": np.array(tiles, np.int32)}
    interior = irt.interior_packets(lp, chained.info, W, H, **sel)
    void = irt.void_packets(lp, chained.info, W, H, **sel)
    if CC.refuses(name):
        assert not void.any() and not interior.any()
    else:
        assert void.any() or interior.any(), "the case carries no class"
    if name == "window2":  # the one case that takes section 4(c)'s second rule to the device
        assert void.any() and interior.any(), "the second window eye lost a class"
    nvoid = int(void.sum())
    ninterior = int(interior.sum()) if nvoid else 0  # the interior bitmap rides on the void data
    pixels = W * H if tiles is None else len(tiles) * 4096

    def launch(ctx, frames, fb, acc):
        if tiles is None:
            if frames == 1:
                ctx.render(lp, W, H, fb.data_ptr(), acc.data_ptr())
            else:
                ctx.render_accumulate(lp, W, H, frames, fb.data_ptr(), acc.data_ptr())
        else:
            ctx.render_tile_list(lp, W, H, sel["tiles"], frames, fb.data_ptr(), acc.data_ptr())

    fb_c, acc_c = _buffers(pixels)
    fb_s, acc_s = _buffers(pixels)
    kernels, first = [], None
    for k in range(LAUNCHES):
        sums = np.zeros(5, np.int64)
        for aid in range(k * F, (k + 1) * F):
            lp.accumID = aid
            launch(single, 1, fb_s, acc_s)
            assert single.interior_use() == 0 and single.void_use() == 0, "a single frame classified"
            sums += _counts(single.stats())
        lp.accumID = k * F
        launch(chained, F, fb_c, acc_c)
        if k == 0:
            assert chained.void_use() == 0 and chained.interior_use() == 0, "classified at the request's first launch"
        else:
            assert chained.void_use() == nvoid
            assert chained.interior_use() == ninterior
            kernels.append(chained.last_plan()[0])
        got, ref = _host(fb_c, acc_c), _host(fb_s, acc_s)
        assert np.array_equal(_counts(chained.stats()), sums), f"event counts, launch {k}"
        assert np.array_equal(got[1], ref[1]), f"accum, launch {k}"
        assert np.array_equal(got[0], ref[0]), f"fb, launch {k}"
        if k == 0:
            first = (got[0], got[1], sums)
    assert chained.chain_errors() == 0
    return tuple(kernels), first


@pytest.mark.parametrize("name,scene,W,H,tiles", CASES,
                         ids=[f"{n}-{s}-{W}x{H}" + ("-tiles" if t else "") for n, s, W, H, t in CASES])
def test_chained_launches_equal_single_frames(name, scene, W, H, tiles):
    _, first = _run(name, scene, W, H, tiles)
    if not CC.refuses(name) and scene != "window":
        assert first[0].any(), "an empty frame"


def test_both_forms_of_the_void_data_ran():
    """The flat scene's ragged frame takes the work-item list, the terrain scene the bitmap on the
    plain grid (irt_debug_last_plan's kernel id)."""
    flat, _ = _run("P3", "flat", 203, 71, None)
    terrain, _ = _run("P3", "terrain", 96, 72, None)
    assert all(k & VOID_LIST for k in flat), flat
    assert all(k & VOID_BITMAP and not k & VOID_LIST for k in terrain), terrain


@pytest.mark.parametrize("name,scene", [("P71.5", "flat"), ("window", "window")])
def test_first_launch_equals_the_oracle(name, scene):
    """A camera and a box no other device test renders: the chained launch's four frames against the
    oracle's, bit for bit, with the counts both keep."""
    W = H = 64
    _, (fb, acc, counts) = _run(name, scene, W, H, None)
    a_ref, f_ref, stats, _ = oracle_frame(CC.cells(scene), W, H, camera=CC.camera(name, scene), accum_ids=range(F))
    assert np.array_equal(acc.reshape(H, W, 4), bits(a_ref)), "accum"
    assert np.array_equal(fb.reshape(H, W), f_ref), "fb"
    want = [sum(getattr(s, f) for s in stats) for f in ("rays_launched", "rays_in_box", "locate_calls", "samples_found")]
    assert list(counts[:4]) == want
    assert f_ref.any()
