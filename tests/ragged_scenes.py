"""Frames whose width or height is no multiple of 8: scenes, sizes, cameras, prior buffer contents
and the oracle's frames, shared by tests/test_ragged_cpu.py (the census, no GPU) and
tests/test_gpu_ragged.py.

The render kernels map one wave to an 8 x 8 pixel packet, one 256-thread workgroup to a 16 x 16
block and one launch tile to 64 x 64 pixels (pixel_of, csrc/irt_render.hip).  At a size that is a
multiple of 8 every wave lies wholly inside the frame or wholly outside it; at the sizes here the
frame edge cuts through waves (a "partial packet": an 8 x 8 packet with at least one pixel inside
the frame and at least one outside), through blocks and through tiles.

Scenes   flat = synth_grid(2, 1, 20); terrain = synth_grid(2, 2, 65, terrain=4000) (holes: the
         miss mode, measured-cost scheduling on by default).
Sizes    SIZES, see there.
Cameras  framing, viewall (None: the frame corners miss the box), south_oblique (box misses along
         an edge) and shell_down (from inside the shell) of helpers.view_battery.
Prior    prior(W, H, seed): what fb and accum hold before the first frame -- random fb words;
         accum random finite floats in [-2, 2] with -0.0, a subnormal, +inf and NaN sprinkled in.
         MARK: zeroed accum under an fb word no frame can write, which shows the pixels a frame
         left alone (miss_mask).
Frames   oracle_frames(...): the oracle's accum bits, fb words and per-frame counts, rendered once
         per session (functools.lru_cache); the arrays are read-only and shared.

Transfer functions: the default one; for the sampler modes (MODE_CUBQL, MODE_TRIANGLES) the default
colours at a constant alpha of ALPHA, as tests/test_gpu_samplers.py uses, so that oracle frames
take seconds.

Census (tests/test_ragged_cpu.py checks these figures and the conditions they stand for).  Pixels
inside partial packets, over all sizes: 3842 of 25922 (PARTIAL_PIXELS).  In-frame pixels of partial
packets that end with alpha > 0 at accumID 0 (CENSUS_ALPHA), under FRAMING -- or under `near`
(FRAMING's eye moved in to 7.5e6) at the four sizes where FRAMING covers none of them, NEAR_SIZES --
flat | terrain:
  1x1 1 | 1 (near)    1x9 4 | 4      9x1 9 | 9 (near)    7x7 32 | 32    8x9 8 | 8 (near)
  13x5 41 | 41        63x65 61 | 61  65x63 60 | 60       67x33 163 | 163 (near: all of them)
  129x7 549 | 561     203x71 145 | 143
Partial packets holding box hits beside box misses under south_oblique (the oracle's frames), flat |
terrain: 67x33 5 | 4, 129x7 9 | 9, 203x71 8 | 8; under viewAll only 129x7 has any (8 | 8).
"""
import functools

import numpy as np

import helpers
import irt
import oracle as O

SCENES = ("flat", "terrain")
SIZES = (
    (1, 1), (1, 9), (9, 1), (7, 7), (8, 9), (13, 5),  # single packets and strips
    (63, 65), (65, 63),                               # one pixel short of, or past, a tile edge
    (67, 33),                                         # partial packet, block and tile at once
    (129, 7),                                         # three tiles wide, one partial packet high
    (203, 71),                                        # the size the unpack tests use
)
MIXED_SIZES = ((67, 33), (129, 7), (203, 71))  # where partial packets must mix box hits and misses
CAMERAS = ("framing", "near", "viewall", "south_oblique", "shell_down")
# FRAMING with the eye moved in along its axis, from 1.4e7 to 7.5e6: the globe's disc (27 degrees
# of FRAMING's 30 to the frame edge) then covers the frame's last column and row, and the ray of a
# one-pixel frame, which leaves up to a frame width beside the centre ((x + .5 + jitter) * du).
NEAR = ((0.0, 0.0, 7.5e6), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 60.0)
# At these sizes no in-frame pixel of a partial packet ends covered under FRAMING (at 67 x 33 the
# partial packets are columns 64..66 and row 32, outside the disc): the census conditions are met
# by `near` there, and the GPU tests render both cameras.
NEAR_SIZES = ((1, 1), (9, 1), (8, 9), (67, 33))
ALPHA = 0.02  # tests/test_gpu_samplers.py FRAME_ALPHA
MARK = "mark"  # prior seed: accum zeroed, fb MARK_WORD everywhere
TILE = "tile"  # prior seed: accum -7.25, fb 0xDEADBEEF: the sentinel of the packed-tile tests
# No frame writes this word over zeroed accum: its alpha byte would be make_8bit(alpha / (accumID
# + 1)) with alpha 0 or 1, which is 0, 255, 128, 85, 64, ... and 1 only at accumID 255.
MARK_WORD = np.uint32(0x01ABCDEF)

PARTIAL_PIXELS = (3842, 25922)  # in-frame pixels of partial packets, all pixels, over SIZES
# size: (flat, terrain) in-frame pixels of partial packets with alpha > 0, framing, accumID 0
CENSUS_ALPHA = {}  # filled in below


def ragged(size):
    return bool(size[0] % 8 or size[1] % 8)


def partial_packet_pixels(W, H):
    """(H, W) bool: the in-frame pixels of partial packets."""
    ys, xs = np.mgrid[0:H, 0:W]
    return ((W % 8 != 0) & (xs // 8 == W // 8)) | ((H % 8 != 0) & (ys // 8 == H // 8))


def packet_ids(W, H):
    """(H, W) int: the 8 x 8 packet each pixel lies in."""
    ys, xs = np.mgrid[0:H, 0:W]
    return (ys // 8) * ((W + 7) // 8) + xs // 8


def _frozen(a):
    a = np.ascontiguousarray(a)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def cells(scene):
    c = {"flat": lambda: irt.synth_grid(2, 1, 20),
         "terrain": lambda: irt.synth_grid(2, 2, 65, terrain=4000.0)}[scene]()
    c.setflags(write=False)
    return c


def camera(scene, name):
    """The (vp, vi, vu, fovy) camera `name` of `scene`, None for viewAll."""
    if name == "framing":
        return helpers.FRAMING
    if name == "near":
        return NEAR
    if name == "viewall":
        return None
    return helpers.view_battery(cells(scene))[name]


@functools.lru_cache(maxsize=None)
def transfer(scene, tf):
    """(lut, value range) of transfer function tf ("default" or "alpha") as the device gets it."""
    info = irt.volume_info(cells(scene))
    lut, vr = irt.default_transfunc((info.dataRange.lower, info.dataRange.upper))
    if tf == "alpha":
        lut = lut.copy()
        lut[:, 3] = ALPHA
    return _frozen(lut), vr


def tf_of(mode):
    return "default" if mode == irt.MODE_USER_GEOM else "alpha"


@functools.lru_cache(maxsize=None)
def _oracle_scene(scene, tf):
    S = O.OracleScene(cells(scene))
    if tf == "default":
        lut, vr = S.default_lut()
    else:
        lut, vr = transfer(scene, tf)
    S.set_transfunc(lut, vr)
    return S


@functools.lru_cache(maxsize=None)
def prior(W, H, seed):
    """(accum (H, W, 4) float32, fb (H, W) uint32) before the first frame; seed None: zeros;
    MARK: zeroed accum under MARK_WORD.  Read-only."""
    if seed is None:
        return _frozen(np.zeros((H, W, 4), np.float32)), _frozen(np.zeros((H, W), np.uint32))
    if seed == MARK:
        return _frozen(np.zeros((H, W, 4), np.float32)), _frozen(np.full((H, W), MARK_WORD, np.uint32))
    if seed == TILE:
        return _frozen(np.full((H, W, 4), -7.25, np.float32)), _frozen(np.full((H, W), 0xDEADBEEF, np.uint32))
    rng = np.random.default_rng([seed, W, H])
    fb = rng.integers(0, 2**32, (H, W), dtype=np.uint32)
    accum = rng.uniform(-2.0, 2.0, (H, W, 4)).astype(np.float32)
    flat = accum.reshape(-1)
    specials = np.array([-0.0, 1e-41, np.inf, np.nan], np.float32)  # 1e-41: a subnormal
    n = max(4, flat.size // 16)
    where = rng.choice(flat.size, min(n, flat.size), replace=False)
    flat[where] = specials[np.arange(where.size) % 4]
    return _frozen(accum), _frozen(fb)


def host_threads():
    from test_gpu_scale import host_threads as ht
    return ht()


@functools.lru_cache(maxsize=None)
def oracle_frames(scene, cam, size, accum_ids=(0,), raygen=0, accel_mode=0, mode=0, prior_seed=None):
    """The oracle's frames accum_ids of (scene, camera, size), one over the other, starting from
    prior(W, H, prior_seed): (accum bit patterns (H, W, 4) uint32, fb (H, W) uint32, per-frame
    counts [(raysLaunched, raysInBox, locateCalls, samplesFound)]).  cam: a name of CAMERAS, or a
    tuple of tuples (org, dir_00, dir_du, dir_dv) per frame (a sequence of views).  Shared: the
    arrays are read-only."""
    W, H = size
    S = _oracle_scene(scene, tf_of(mode))
    pa, pf = prior(W, H, prior_seed)
    accum, fb = np.array(pa, copy=True), np.array(pf, copy=True)
    counts = []
    for k, aid in enumerate(accum_ids):
        if isinstance(cam, str):
            c = S.camera(W, H, camera(scene, cam))
        else:
            c = tuple(np.array(v, np.float32) for v in cam[k])
        p = S.params(c, accum_id=aid, raygen=raygen, accel_mode=accel_mode, mode=mode)
        _, _, st = S.render(p, W, H, accum=accum, fb=fb, threads=host_threads(),
                            fast=1 if mode != irt.MODE_USER_GEOM else 2)
        counts.append((st.rays_launched, st.rays_in_box, st.locate_calls, st.samples_found))
    return _frozen(helpers.bits(accum)), _frozen(fb), tuple(counts)


def summed(counts):
    return tuple(int(sum(c[k] for c in counts)) for k in range(4))


@functools.lru_cache(maxsize=None)
def miss_mask(scene, cam, size, accum_ids=(0,), raygen=0, accel_mode=0, mode=0):
    """(H, W) bool: the pixels whose ray misses the box in every frame of accum_ids (the raygen
    returns before it writes anything, deviceCode.cu:294-295), from frames the oracle renders over
    MARK: a pixel that still holds MARK_WORD was never written.  Independent of what the random
    prior contents show."""
    _, fb, counts = oracle_frames(scene, cam, size, accum_ids, raygen, accel_mode, mode, MARK)
    miss = fb == MARK_WORD
    if len(accum_ids) == 1:
        assert int((~miss).sum()) == counts[0][1], "MARK_WORD was written, or a hit pixel kept it"
    return _frozen(miss)


def setup(scene, cam, size, raygen=0):
    """irt.setup_frame of (scene, camera, size): the device's LaunchParams and volume facts."""
    return irt.setup_frame(cells(scene), size[0], size[1], camera=camera(scene, cam), raygen=raygen)


CENSUS_ALPHA.update({
    (1, 1): (1, 1), (1, 9): (4, 4), (9, 1): (9, 9), (7, 7): (32, 32), (8, 9): (8, 8), (13, 5): (41, 41),
    (63, 65): (61, 61), (65, 63): (60, 60), (67, 33): (163, 163), (129, 7): (549, 561),
    (203, 71): (145, 143),
})
