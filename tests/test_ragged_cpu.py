"""The census of tests/ragged_scenes.py: conditions on the inputs of tests/test_gpu_ragged.py,
checked on the oracle's frames without a GPU, so that the GPU comparisons cannot pass vacuously --
the partial packets of every ragged size hold covered pixels, some hold box hits beside box misses,
the terrain scene's rays meet voids, and the prior buffer contents survive exactly where a ray
misses the box.  Where a condition fails the camera changes (ragged_scenes.NEAR_SIZES), never the
condition."""
import numpy as np
import pytest

import helpers
import ragged_scenes as R


def primary(size):
    return "near" if size in R.NEAR_SIZES else "framing"


def test_sizes_and_partial_pixels():
    assert len(R.SIZES) == 11 and all(R.ragged(s) for s in R.SIZES)
    inside = sum(int(R.partial_packet_pixels(*s).sum()) for s in R.SIZES)
    assert (inside, sum(w * h for w, h in R.SIZES)) == R.PARTIAL_PIXELS
    # the definition, restated pixel by pixel at one size
    W, H = 13, 5
    m = R.partial_packet_pixels(W, H)
    for y in range(H):
        for x in range(W):
            px, py = x // 8, y // 8
            cut = (8 * px + 8 > W) or (8 * py + 8 > H)
            assert m[y, x] == cut


@pytest.mark.parametrize("scene", R.SCENES)
def test_partial_packets_hold_covered_pixels(scene):
    """Every ragged size, under its primary camera (FRAMING, or `near` where FRAMING's disc does
    not reach the partial packets): an in-frame pixel of a partial packet ends with alpha > 0, and
    samples are found.  The figures are recorded in ragged_scenes.CENSUS_ALPHA."""
    got = {}
    for size in R.SIZES:
        a, _, counts = R.oracle_frames(scene, primary(size), size)
        covered = (a.view(np.float32)[..., 3] > 0) & R.partial_packet_pixels(*size)
        got[size] = int(covered.sum())
        assert covered.any(), (scene, size)
        assert counts[0][0] == size[0] * size[1] and counts[0][3] > 0, (scene, size, counts)
    print(scene, got)
    k = R.SCENES.index(scene)
    assert got == {s: v[k] for s, v in R.CENSUS_ALPHA.items()}
    # FRAMING falls short exactly at NEAR_SIZES (else `near` would not be needed there)
    for size in R.NEAR_SIZES:
        a, _, _ = R.oracle_frames(scene, "framing", size)
        assert not ((a.view(np.float32)[..., 3] > 0) & R.partial_packet_pixels(*size)).any(), size


@pytest.mark.parametrize("size", R.MIXED_SIZES)
@pytest.mark.parametrize("scene", R.SCENES)
def test_partial_packets_mix_box_hits_and_misses(scene, size):
    """Under south_oblique a partial packet holds a pixel whose ray hits the box beside one whose
    ray misses it -- by the oracle's own frame (miss_mask) and by helpers.range_census's ray through
    the middle of the jitter footprint; on the terrain scene the rays meet voids."""
    W, H = size
    pp, ids = R.partial_packet_pixels(W, H), R.packet_ids(W, H)
    su = R.setup(scene, "south_oblique", size)
    _, _, in_box = helpers.range_census(su.lp, W, H, su.info)
    miss = R.miss_mask(scene, "south_oblique", size)
    for what, hit in (("oracle", ~miss), ("range_census", in_box)):
        mixed = [p for p in np.unique(ids[pp]) if hit[ids == p].any() and not hit[ids == p].all()]
        assert mixed, (scene, size, what)
    for cam in ("viewall", "south_oblique"):
        _, _, counts = R.oracle_frames(scene, cam, size)
        assert 0 < counts[0][1] < W * H, (cam, counts)  # some rays hit the box, some miss it
        if scene == "terrain":
            assert counts[0][2] > counts[0][3], (cam, counts)  # locate_calls > samples_found


@pytest.mark.parametrize("size", [(13, 5), (67, 33), (203, 71)])
@pytest.mark.parametrize("scene", R.SCENES)
def test_prior_contents_survive_where_the_ray_misses(scene, size):
    """accumID 3 under viewAll over the random prior contents: every box-miss pixel's accum bits
    and fb word are the prior's after the oracle's frame, every other pixel's fb word changed, and
    the prior holds each special value on hit and on missed pixels alike (where the frame has
    both)."""
    W, H = size
    pa, pf = R.prior(W, H, 7)
    a, f, counts = R.oracle_frames(scene, "viewall", size, (3,), prior_seed=7)
    miss = R.miss_mask(scene, "viewall", size, (3,))
    assert int((~miss).sum()) == counts[0][1] and miss.any() and not miss.all()
    assert np.array_equal(a[miss], helpers.bits(pa)[miss]) and np.array_equal(f[miss], pf[miss])
    assert (f[~miss] != pf[~miss]).mean() > 0.99
    b = helpers.bits(pa)
    for word in (0x80000000, 0x7F800000):  # -0.0, +inf
        assert (b == word).any()
    assert np.isnan(pa).any() and ((b & 0x7F800000) == 0)[b & 0x7FFFFFFF != 0].any()  # NaN, subnormal
    assert np.isfinite(pa).mean() > 0.9 and np.abs(pa[np.isfinite(pa)]).max() <= 2.0
    if W * H > 1000:
        for special in (np.isnan(pa), np.isposinf(pa)):
            assert special[~miss].any() and special[miss].any()


def test_progressive_prior_contents_keep_never_hit_pixels():
    """Frames 2..8 under viewAll at 67 x 33 over the prior contents: some pixels miss the box in
    every frame (and keep the prior), some hit it in some frames only (the jitter)."""
    size, ids = (67, 33), tuple(range(2, 9))
    never = R.miss_mask("flat", "viewall", size, ids)
    each = [R.miss_mask("flat", "viewall", size, (k,)) for k in ids]
    assert never.any() and not never.all()
    assert np.array_equal(never, np.logical_and.reduce(each))
    assert (np.logical_or.reduce(each) & ~never).any()
    pa, pf = R.prior(67, 33, 7)
    a, f, _ = R.oracle_frames("flat", "viewall", size, ids, prior_seed=7)
    assert np.array_equal(a[never], helpers.bits(pa)[never]) and np.array_equal(f[never], pf[never])
