"""Frames whose sizes are no multiples of 8, on the device against the oracle.

At every other size the GPU suite renders, each wave (an 8 x 8 pixel packet, pixel_of in
csrc/irt_render.hip) lies wholly inside the frame or wholly outside it.  Here the frame edge cuts
through waves, blocks and tiles (tests/ragged_scenes.py: the sizes, scenes, cameras and the
oracle's frames; tests/test_ragged_cpu.py: the census that keeps these comparisons from passing
vacuously), so a lane without a pixel travels through the wave-cooperative loop beside lanes with
rays: the accum prefetch under a partial exec mask, raysLaunched, split packets' parts at the
frame edge, the chained publish and wait of a wave some of whose pixels do not exist, k_accumulate,
packed tile buffers whose out-of-frame slots must stay as they were, the persistent launch and the
A/B variants, the seed accumID * W * H + x with W * H odd.

Every comparison is bit for bit -- accum bit patterns, fb words and the counts raysLaunched,
raysInBox, locateCalls, samplesFound -- with one exception stated in
test_ragged_frame_over_prior_contents (the payload of a NaN the lerp produces).  Every device
buffer lies between two guards of GUARD elements holding a sentinel, checked after each use; and
frames are rendered not only into zeroed buffers but over prior contents (random fb words, random
accum floats with -0.0, a subnormal, +inf and NaN), which a ray that misses the box must leave
alone (deviceCode.cu:294-295) and the single-frame lerp with accumID > 0 must read."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import irt
import ragged_scenes as R
from helpers import bits

pytestmark = pytest.mark.gpu

GUARD = 4096  # elements (fb words, accum float4s) before and after every device buffer
GUARD_FB = np.uint32(0x6A6A6A6A)
GUARD_ACC = np.uint32(0xC2F6E979)  # a finite float, about -123.456
NOMISS, VOIDLOC = 262144, 1073741824  # render variant bits (tests/test_gpu_views.py)


class Buf:
    """A device fb / accum pair of n pixels holding (accum bits (n, 4), fb words (n,)), each
    between two guards."""

    def __init__(self, accum, fb):
        import torch
        self.torch = torch
        a = np.ascontiguousarray(accum)
        a = (a if a.dtype == np.uint32 else bits(a)).reshape(-1, 4)
        f = np.ascontiguousarray(fb, dtype=np.uint32).reshape(-1)
        self.n = f.size
        assert a.shape[0] == self.n
        ha = np.full((self.n + 2 * GUARD, 4), GUARD_ACC, np.uint32)
        hf = np.full(self.n + 2 * GUARD, GUARD_FB, np.uint32)
        ha[GUARD:GUARD + self.n] = a
        hf[GUARD:GUARD + self.n] = f
        self._a = torch.from_numpy(ha.view(np.int32).reshape(-1)).cuda()
        self._f = torch.from_numpy(hf.view(np.int32)).cuda()
        self.acc = self._a.data_ptr() + GUARD * 16
        self.fb = self._f.data_ptr() + GUARD * 4

    @classmethod
    def prior(cls, size, seed=None):
        return cls(*R.prior(size[0], size[1], seed))

    @classmethod
    def filled(cls, n, acc_word, fb_word):
        return cls(np.full((n, 4), acc_word, np.uint32), np.full(n, fb_word, np.uint32))

    def host(self, shape=None):
        """(accum bits, fb words) as the device holds them now; asserts the guards are intact."""
        self.torch.cuda.synchronize()
        ha = self._a.cpu().numpy().view(np.uint32).reshape(-1, 4)
        hf = self._f.cpu().numpy().view(np.uint32)
        for g in (ha[:GUARD], ha[GUARD + self.n:]):
            assert (g == GUARD_ACC).all(), f"accum guard overwritten at {np.argwhere(g != GUARD_ACC)[:4].tolist()}"
        for g in (hf[:GUARD], hf[GUARD + self.n:]):
            assert (g == GUARD_FB).all(), f"fb guard overwritten at {np.argwhere(g != GUARD_FB)[:4].tolist()}"
        a, f = ha[GUARD:GUARD + self.n], hf[GUARD:GUARD + self.n]
        if shape is not None:
            a, f = a.reshape(shape[1], shape[0], 4), f.reshape(shape[1], shape[0])
        return a, f


def counts_of(st):
    return (st.raysLaunched, st.raysInBox, st.locateCalls, st.samplesFound)


def assert_same(got, want, label):
    """got, want: (accum bits, fb words[, counts])."""
    bad = np.any(got[0] != want[0], axis=-1) | (got[1] != want[1])
    assert not bad.any(), (f"{label}: {int(bad.sum())} of {bad.size} pixels differ, first (y, x) "
                           f"{np.argwhere(bad)[:4].tolist()}")
    if len(want) > 2:
        assert tuple(got[2]) == tuple(want[2]), f"{label}: counts {tuple(got[2])}, oracle {tuple(want[2])}"


def primary(size):
    return "near" if size in R.NEAR_SIZES else "framing"


def make_context(scene, tf="default", wedges=False):
    cells = R.cells(scene)
    ctx = irt.Context(cells, 0)
    if tf == "default":
        su = irt.setup_frame(cells, 8, 8)
        ctx.set_transfunc(su.lut, su.value_range)
    else:
        ctx.set_transfunc(*R.transfer(scene, tf))
    if wedges:
        ctx.build_wedge_accel(cells)
    return ctx


@pytest.fixture(scope="module")
def contexts():
    """scene -> its context with the default transfer function, built once."""
    made = {}

    def get(scene):
        if scene not in made:
            made[scene] = make_context(scene)
        return made[scene]

    yield get
    for ctx in made.values():
        ctx.close()


def lp_of(scene, cam, size, accum_id=0, **kw):
    lp = R.setup(scene, cam, size, raygen=kw.pop("raygen", 0)).lp
    lp.accumID = accum_id
    for k, v in kw.items():
        setattr(lp, k, v)
    return lp


def render(ctx, lp, size, buf):
    ctx.render(lp, size[0], size[1], buf.fb, buf.acc)
    a, f = buf.host(size)
    return a, f, counts_of(ctx.stats())


# ---- 1. single frames into zeroed buffers
FRAME_CASES = ([(s, "framing") for s in R.SIZES] + [(s, "near") for s in R.NEAR_SIZES]
               + [(s, c) for s in ((67, 33), (203, 71)) for c in ("viewall", "south_oblique", "shell_down")])


@pytest.mark.parametrize("size,cam", FRAME_CASES, ids=[f"{s[0]}x{s[1]}-{c}" for s, c in FRAME_CASES])
@pytest.mark.parametrize("scene", R.SCENES)
def test_ragged_frame_matches_oracle(contexts, scene, size, cam):
    want = R.oracle_frames(scene, cam, size)
    got = render(contexts(scene), lp_of(scene, cam, size), size, Buf.prior(size))
    assert got[2][0] == size[0] * size[1], f"raysLaunched {got[2][0]} at {size}"
    assert_same(got, (want[0], want[1], want[2][0]), f"{scene} {size} {cam}")


# ---- 2. a single frame with accumID > 0 over prior contents
@pytest.mark.parametrize("size", [(13, 5), (67, 33), (203, 71)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("scene", R.SCENES)
def test_ragged_frame_over_prior_contents(contexts, scene, size):
    """accumID 3 under viewAll over ragged_scenes.prior(seed 7).  Pixels whose ray misses the box
    must hold the prior contents byte for byte (checked first, so a failure names the cause); the
    whole frame must equal the oracle's.

    NaN: where the prior accum word is a NaN, the lerp w * c + (1 - w) * old yields a NaN on the
    host and on the device, but IEEE 754 leaves its sign and payload open (an x86 mulss / addss
    and a GPU v_mul_f32 / v_add_f32 need not pass the same bits on).  On the words the oracle's
    frame holds a NaN in -- hit pixels only: a missed pixel's NaN was never computed -- the device
    word must be a NaN, its bits are not compared (their agreement is printed: on an MI355X all 1,
    30 and 138 such words of the three sizes carried the oracle's bits); every other word, and
    every fb word, is compared bit for bit."""
    seed, aid = 7, 3
    want = R.oracle_frames(scene, "viewall", size, (aid,), prior_seed=seed)
    miss = R.miss_mask(scene, "viewall", size, (aid,))
    pa, pf = R.prior(size[0], size[1], seed)
    a, f, n = render(contexts(scene), lp_of(scene, "viewall", size, aid), size, Buf.prior(size, seed))
    assert np.array_equal(a[miss], bits(pa)[miss]), "a ray that missed the box changed accum"
    assert np.array_equal(f[miss], pf[miss]), "a ray that missed the box changed fb"
    nan = np.isnan(want[0].view(np.float32)) & ~miss[..., None]
    assert np.isnan(a.view(np.float32)[nan]).all()
    print(f"{scene} {size}: {int(nan.sum())} NaN words lerped, device bits equal the oracle's on "
          f"{int((a[nan] == want[0][nan]).sum())}")
    assert_same((np.where(nan, want[0], a), f, n), (want[0], want[1], want[2][0]), f"{scene} {size} over prior contents")


# ---- 3. the other raygen, accelerator and samplers
@pytest.mark.parametrize("size", [(67, 33), (13, 5)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("form", ["ae", "grid", "cubql", "triangles"])
def test_ragged_kernel_forms(contexts, form, size):
    """woodcockTrackingAE, GRID_ACCEL_MODE, and the MODE_CUBQL and MODE_TRIANGLES samplers (these
    two under the constant-alpha transfer function), flat scene."""
    kw = {"ae": dict(raygen=irt.RAYGEN_AE), "grid": dict(accelMode=irt.ACCEL_GRID),
          "cubql": dict(mode=irt.MODE_CUBQL), "triangles": dict(mode=irt.MODE_TRIANGLES)}[form]
    okw = {"ae": dict(raygen=1), "grid": dict(accel_mode=1), "cubql": dict(mode=irt.MODE_CUBQL),
           "triangles": dict(mode=irt.MODE_TRIANGLES)}[form]
    cam = primary(size)
    want = R.oracle_frames("flat", cam, size, **okw)
    assert (want[0].view(np.float32)[..., 3] > 0).any() and want[2][0][3] > 0
    sampler = "mode" in kw
    ctx = make_context("flat", "alpha", wedges=True) if sampler else contexts("flat")
    try:
        got = render(ctx, lp_of("flat", cam, size, **kw), size, Buf.prior(size))
        assert got[2][0] == size[0] * size[1]
        assert_same(got, (want[0], want[1], want[2][0]), f"{form} {size}")
    finally:
        if sampler:
            ctx.close()


# ---- 4. progressive batches, chained and through the sample buffer
@pytest.mark.parametrize("chain", [True, False], ids=["chained", "unchained"])
@pytest.mark.parametrize("size", [(9, 1), (67, 33), (203, 71)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("scene", R.SCENES)
def test_ragged_progressive(contexts, scene, size, chain):
    """irt_render_accumulate: 4 frames from accumID 0, then 3 more from accumID 4 on the same
    buffers == the oracle's seven sequential frames, after each launch, with the summed counts.
    Then the same two launches from accumID 2 under viewAll over the prior contents: a pixel whose
    ray misses the box in every frame keeps them (NaN words as in
    test_ragged_frame_over_prior_contents)."""
    ctx = contexts(scene)
    ctx.set_chain(chain)
    W, H = size
    try:
        for cam, first, seed in ((primary(size), 0, None), ("viewall", 2, 7)):
            buf = Buf.prior(size, seed)
            for start, k in ((first, 4), (first + 4, 3)):
                ids = tuple(range(first, start + k))
                want = R.oracle_frames(scene, cam, size, ids, prior_seed=seed)
                ctx.render_accumulate(lp_of(scene, cam, size, start), W, H, k, buf.fb, buf.acc)
                a, f = buf.host(size)
                n = counts_of(ctx.stats())
                nan = np.isnan(want[0].view(np.float32)) if seed is not None else np.zeros(a.shape, bool)
                if seed is not None:
                    never = R.miss_mask(scene, cam, size, ids)
                    pa, pf = R.prior(W, H, seed)
                    assert np.array_equal(a[never], bits(pa)[never]) and np.array_equal(f[never], pf[never])
                    nan &= ~never[..., None]
                    assert np.isnan(a.view(np.float32)[nan]).all()
                assert_same((np.where(nan, want[0], a), f, n), (want[0], want[1], R.summed(want[2][-k:])),
                            f"{scene} {size} {cam} frames {start}..{start + k - 1} chain={chain}")
                assert n[0] == k * W * H
        assert ctx.chain_errors() == 0
    finally:
        ctx.set_chain(True)


# ---- 5. a sequence of views in one launch
@pytest.mark.parametrize("scene", R.SCENES)
def test_ragged_sequence(contexts, scene):
    """irt_render_sequence of 5 orbit views (tests/test_gpu_chain.py::_views) at 67 x 33 == five
    oracle frames, each with its view's own camera, one over the other."""
    size, n = (67, 33), 5
    W, H = size
    ctx = contexts(scene)
    lps, cams = [], []
    for k in range(n):
        th = 2.0 * np.pi * k / 60.0
        c = irt.camera_look_at((1.4e7 * np.sin(th), 0.0, 1.4e7 * np.cos(th)), (0.0, 0.0, 0.0),
                               (0.0, 1.0, 0.0), 60.0, W, H)
        q = lp_of(scene, "framing", size)
        q.org, q.dir_00, q.dir_du, q.dir_dv = c.org, c.dir_00, c.dir_du, c.dir_dv
        lps.append(q)
        cams.append(tuple(tuple(v.tolist()) for v in (c.org, c.dir_00, c.dir_du, c.dir_dv)))
    want = R.oracle_frames(scene, tuple(cams), size, (0,) * n)
    for chain in (True, False):
        ctx.set_chain(chain)
        buf = Buf.prior(size)
        ctx.render_sequence(lps, W, H, buf.fb, buf.acc)
        a, f = buf.host(size)
        if chain:  # unchained, the sequence is one launch per view: the last launch's counts
            assert_same((a, f, counts_of(ctx.stats())), (want[0], want[1], R.summed(want[2])), f"{scene} sequence")
        else:
            assert_same((a, f, counts_of(ctx.stats())), (want[0], want[1], want[2][-1]), f"{scene} sequence, unchained")
    ctx.set_chain(True)
    assert ctx.chain_errors() == 0


# ---- 6. packed tile buffers
TILE_ACC = np.uint32(0xC0E80000)  # -7.25: what the packed buffers hold before (ragged_scenes.TILE)
TILE_FB = np.uint32(0xDEADBEEF)


def packed_want(size, tiles, frame):
    """The packed buffers of `tiles` (64 x 64 slots in list order) after a launch: the oracle's
    frame (rendered over the same sentinel) inside the frame, the sentinel in every out-of-frame
    slot of a partial tile."""
    W, H = size
    tx = (W + 63) // 64
    a = np.full((len(tiles), 64, 64, 4), TILE_ACC, np.uint32)
    f = np.full((len(tiles), 64, 64), TILE_FB, np.uint32)
    for k, t in enumerate(tiles):
        x0, y0 = (t % tx) * 64, (t // tx) * 64
        w, h = min(64, W - x0), min(64, H - y0)
        a[k, :h, :w] = frame[0][y0:y0 + h, x0:x0 + w]
        f[k, :h, :w] = frame[1][y0:y0 + h, x0:x0 + w]
    return a.reshape(-1, 4), f.reshape(-1)


@pytest.mark.parametrize("size", [(65, 63), (129, 7), (203, 71)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("scene", R.SCENES)
def test_ragged_tiles(contexts, scene, size):
    """irt_render_tiles (strides 1, 2, 3), irt_render_tile_list over a shuffled list and
    irt_render_tiles_accumulate (3 frames, chained and not) into packed buffers prefilled with a
    sentinel: in-frame pixels == the oracle's full frame, out-of-frame slots of partial tiles keep
    the sentinel, in fb and accum.  irt_unpack_tiles / irt_unpack_tile_table then give the
    oracle's fb in a guarded linear buffer."""
    W, H = size
    ctx = contexts(scene)
    cam = "south_oblique" if size == (203, 71) else primary(size)  # box misses inside tiles too
    ntot = irt.num_tiles(W, H)
    assert ntot == ((W + 63) // 64) * ((H + 63) // 64)
    one = R.oracle_frames(scene, cam, size, (0,), prior_seed=R.TILE)
    three = R.oracle_frames(scene, cam, size, (0, 1, 2), prior_seed=R.TILE)
    in_frame = W * H

    def unpacked(gathered, ranks, maxt, table=None):
        out = Buf.filled(W * H, GUARD_ACC, np.uint32(0x0BADF00D))
        if table is None:
            ctx.unpack_tiles(gathered, ranks, maxt, W, H, out.fb)
        else:
            ctx.unpack_tile_table(gathered, table, W, H, out.fb)
        return out.host(size)[1]

    for stride in (1, 2, 3):
        maxt = -(-ntot // stride)
        buf = Buf.filled(stride * maxt * 4096, TILE_ACC, TILE_FB)
        rays = 0
        for r in range(min(stride, ntot)):  # 65 x 63 has two tiles: stride 3's last rank has none
            n = ctx.render_tiles(lp_of(scene, cam, size), W, H, r, stride, buf.fb + r * maxt * 4096 * 4,
                                 buf.acc + r * maxt * 4096 * 16)
            assert n == len(range(r, ntot, stride))
            rays += ctx.stats().raysLaunched
        assert rays == in_frame
        a, f = buf.host()
        slots = [t for r in range(stride) for t in list(range(r, ntot, stride))
                 + [None] * (maxt - len(range(r, ntot, stride)))]
        wa, wf = packed_want(size, [t for t in slots if t is not None], one)
        keep = np.repeat([t is not None for t in slots], 4096)
        assert np.array_equal(a[keep], wa) and np.array_equal(f[keep], wf), f"stride {stride}"
        assert (a[~keep] == TILE_ACC).all() and (f[~keep] == TILE_FB).all()  # slots of no tile
        assert np.array_equal(unpacked(buf.fb, stride, maxt), one[1]), f"unpack, stride {stride}"
    # a shuffled tile list
    tiles = [int(t) for t in np.random.default_rng(W * 1000 + H).permutation(ntot)]
    buf = Buf.filled(ntot * 4096, TILE_ACC, TILE_FB)
    ctx.render_tile_list(lp_of(scene, cam, size), W, H, tiles, 1, buf.fb, buf.acc)
    a, f = buf.host()
    wa, wf = packed_want(size, tiles, one)
    assert np.array_equal(a, wa) and np.array_equal(f, wf), "tile list"
    assert counts_of(ctx.stats()) == one[2][0]
    assert np.array_equal(unpacked(buf.fb, 1, ntot, np.array([tiles], np.int32)), one[1])
    # three frames per tile, interleaved over two ranks
    for chain in (True, False):
        ctx.set_chain(chain)
        maxt = -(-ntot // 2)
        buf = Buf.filled(2 * maxt * 4096, TILE_ACC, TILE_FB)
        total = np.zeros(4, np.int64)
        for r in range(2):
            n = ctx.render_tiles_accumulate(lp_of(scene, cam, size), W, H, r, 2, 3, buf.fb + r * maxt * 4096 * 4,
                                            buf.acc + r * maxt * 4096 * 16)
            if n:
                total += counts_of(ctx.stats())
        a, f = buf.host()
        slots = [t for r in range(2) for t in list(range(r, ntot, 2)) + [None] * (maxt - len(range(r, ntot, 2)))]
        wa, wf = packed_want(size, [t for t in slots if t is not None], three)
        keep = np.repeat([t is not None for t in slots], 4096)
        assert np.array_equal(a[keep], wa) and np.array_equal(f[keep], wf), f"3 frames, chain={chain}"
        assert (a[~keep] == TILE_ACC).all() and (f[~keep] == TILE_FB).all()
        assert tuple(int(t) for t in total) == R.summed(three[2])
        assert np.array_equal(unpacked(buf.fb, 2, maxt), three[1])
    ctx.set_chain(True)
    assert ctx.chain_errors() == 0


# ---- 7. measured-cost scheduling with split packets
@pytest.mark.parametrize("lg", [1, 2])
@pytest.mark.parametrize("size", [(203, 71), (67, 33)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_ragged_scheduled_and_split(monkeypatch, size, lg):
    """As tests/test_gpu_views.py::test_scheduled_frames_of_view_equal_unscheduled: 24 launches of
    one frame on the terrain scene with IRT_SCHED=1 and a split factor that splits the costliest
    tenth of the packets into 2^lg parts once measured costs exist.  Every launch == the oracle's
    frame and counts, and launches did split (numSplit > 0), among them parts of packets the
    frame edge cuts."""
    monkeypatch.setenv("IRT_SCHED", "1")
    monkeypatch.setenv("IRT_SPLIT_FACTOR", "1e-6")
    monkeypatch.setenv("IRT_SPLIT_LG", str(lg))
    cam = primary(size)
    want = R.oracle_frames("terrain", cam, size)
    ctx = make_context("terrain")
    try:
        lp = lp_of("terrain", cam, size)
        splits = []
        for k in range(24):
            got = render(ctx, lp, size, Buf.prior(size))
            splits.append(ctx.sched_split())
            assert_same(got, (want[0], want[1], want[2][0]), f"{size} lg {lg} launch {k}, split {splits[-1]}")
        print(size, lg, splits)
        assert max(s[0] for s in splits) > 0 and max(s[0] for s in splits) % 8 == 0, splits
        assert all(s[1] == lg for s in splits if s[0]), splits
    finally:
        ctx.close()


# ---- 8. every compiled variant, and the persistent launch
def test_ragged_variants():
    """Every variant irt_debug_variants reports (the product library's; the A/B library's when
    test_ragged_variants_ab_library runs this test on it), the scenes' other hole forms, and, on the
    A/B library, the persistent launch: single frames and a 3-frame batch at 67 x 33 and 13 x 5, each
    against the oracle."""
    L = irt.lib()
    L.irt_debug_set_variant.argtypes = [C.c_void_p, C.c_int]
    d = L.irt_debug_default_variant()
    ab = irt.LIB_PATH == irt.ALL_LIB_PATH
    for scene in R.SCENES:
        forms = list(irt.compiled_variants())
        assert d in forms
        for v in (d | NOMISS, d | VOIDLOC) if scene == "terrain" else (d | NOMISS,):
            if v not in forms:
                forms.append(v)
        ctx = make_context(scene)
        try:
            for size in ((67, 33), (13, 5)):
                W, H = size
                cam = primary(size)
                one = R.oracle_frames(scene, cam, size)
                three = R.oracle_frames(scene, cam, size, (0, 1, 2))
                for v, queue in [(v, False) for v in forms] + ([(5376, True)] if ab else []):
                    assert L.irt_debug_set_variant(ctx._h, v) == 0, v
                    if ab:
                        ctx.set_queue(queue)
                    label = f"{scene} {size} variant {v}" + (" persistent" if queue else "")
                    got = render(ctx, lp_of(scene, cam, size), size, Buf.prior(size))
                    assert_same(got, (one[0], one[1], one[2][0]), label)
                    buf = Buf.prior(size)
                    ctx.render_accumulate(lp_of(scene, cam, size), W, H, 3, buf.fb, buf.acc)
                    a, f = buf.host(size)
                    assert_same((a, f, counts_of(ctx.stats())), (three[0], three[1], R.summed(three[2])),
                                label + ", 3 frames")
            if not ab:
                with pytest.raises(irt.IrtError):
                    ctx.set_queue(True)
            assert ctx.chain_errors() == 0
        finally:
            ctx.close()


@pytest.mark.skipif(not os.path.exists(irt.ALL_LIB_PATH), reason="make VARIANTS=all not built")
def test_ragged_variants_ab_library():
    """test_ragged_variants on the A/B library (every variant and the persistent launch), in a
    child process: one HIP library per process (IRT_LIB_PATH selects it at load)."""
    env = dict(os.environ, IRT_LIB_PATH=irt.ALL_LIB_PATH)
    r = subprocess.run([sys.executable, "-u", "-m", "pytest", "-x", "-q", "-p", "no:cacheprovider",
                        f"{__file__}::test_ragged_variants"],
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "1 passed" in r.stdout


# ---- 9. statistics off
@pytest.mark.parametrize("scene", R.SCENES)
def test_ragged_statistics_off(contexts, scene):
    """irt_set_statistics(0) at 67 x 33: the same frame, the counts read 0; on again, the oracle's."""
    size = (67, 33)
    ctx = contexts(scene)
    want = R.oracle_frames(scene, "near", size)
    try:
        ctx.set_statistics(False)
        got = render(ctx, lp_of(scene, "near", size), size, Buf.prior(size))
        assert_same(got[:2], want[:2], f"{scene} statistics off")
        assert got[2] == (0, 0, 0, 0)
    finally:
        ctx.set_statistics(True)
    got = render(ctx, lp_of(scene, "near", size), size, Buf.prior(size))
    assert_same(got, (want[0], want[1], want[2][0]), f"{scene} statistics on again")
