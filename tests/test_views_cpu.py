"""The oracle stays pinned to the reference at the cameras of helpers.view_battery: inside the
shell (looking down, along the horizon and up), under the inner sphere, at the centre, south of
the globe and off every axis, in the box but past the sphere, facing away, and grazing -- the
views at which the raygen's ray setup (boxTest, the sphere tests, sdda's range selection and its
first leaf behind the camera) takes the branches the framing and view-all cameras never reach.
tests/test_gpu_views.py compares the GPU with the oracle at these views; here the oracle is
compared with the reference's own raygen (oracle/_ref) and its two locators with each other, and
range_census shows that the battery does reach every branch.
"""
import functools

import numpy as np
import pytest

import irt
import oracle as O
from helpers import (FAR_ONLY, LIMB_ONLY, NO_RANGE, RANGE_LABELS, TWO_RANGES, VIEW_NAMES, bits,
                     range_census, view_battery)

W = 48
VIEWS = list(VIEW_NAMES)
SCENES = {"flat": lambda: irt.synth_grid(2, 1, 31),
          "terrain": lambda: irt.synth_grid(2, 1, 90, terrain=4000.0)}
needs_ref = pytest.mark.skipif(not O.have_ref(), reason="oracle/_ref not built (needs /root/reference)")


@functools.lru_cache(maxsize=None)
def _scene(name):
    cells = SCENES[name]()
    S = O.OracleScene(cells)
    lut, vr = S.default_lut()
    S.set_transfunc(lut, vr)
    return S, view_battery(cells)


def test_battery_names_and_order():
    assert list(_scene("flat")[1]) == VIEWS and len(set(VIEWS)) == 10


@needs_ref
@pytest.mark.parametrize("view", VIEWS)
@pytest.mark.parametrize("scene", sorted(SCENES))
def test_reference_raygen_matches_oracle(scene, view):
    """The reference's own raygen over a strided pixel list == the oracle's literal scan:
    accum bits, fb and both counts."""
    S, views = _scene(scene)
    p = S.params(S.camera(W, W, views[view]))
    ys, xs = np.mgrid[0:W:3, 1:W:3]
    xy = np.stack([xs.ravel(), ys.ravel()], 1).astype(np.int32)
    a1, f1, cnt = O.ref_render_pixels(S, p, W, W, xy, threads=4)
    a2, f2, st = S.render_pixels(p, W, W, xy, threads=4, fast=False)
    assert np.array_equal(bits(a1), bits(a2)) and np.array_equal(f1, f2)
    assert (int(cnt[0]), int(cnt[1])) == (st.locate_calls, st.samples_found)


@pytest.mark.parametrize("view", VIEWS)
@pytest.mark.parametrize("scene", sorted(SCENES))
def test_oracle_locators_agree(scene, view):
    """Whole frames: the oracle's scan (fast=1) == its direction-voxel locator (fast=2), which
    the GPU tests compare with."""
    S, views = _scene(scene)
    p = S.params(S.camera(W, W, views[view]))
    a1, f1, s1 = S.render(p, W, W, threads=4, fast=1)
    a2, f2, s2 = S.render(p, W, W, threads=4, fast=2)
    assert np.array_equal(bits(a1), bits(a2)) and np.array_equal(f1, f2)
    assert s1.asdict() == s2.asdict()


@needs_ref
@pytest.mark.parametrize("form", ["ae", "grid"])
@pytest.mark.parametrize("view", [v for v in VIEWS if v != "framing"])
@pytest.mark.parametrize("scene", sorted(SCENES))
def test_reference_ae_and_grid_match_oracle(scene, view, form):
    """woodcockTrackingAE (raygen 1) and GRID_ACCEL_MODE (accelMode 1) of the reference's own
    code == the oracle's, accum bits, fb and both counts.  AE tracks the whole box interval at
    majorant 1 (thousands of sampleVolume scans per ray from inside the globe), so it runs on a
    strided list of 64 pixels; the grid (no cheaper from inside: its dda3 cells are small) on
    a band of six rows across the frame."""
    S, views = _scene(scene)
    cam = S.camera(W, W, views[view])
    if form == "ae":
        p = S.params(cam, raygen=1)
        ys, xs = np.mgrid[0:W:6, 1:W:6]
        xy = np.stack([xs.ravel(), ys.ravel()], 1).astype(np.int32)
        a1, f1, cnt = O.ref_render_pixels(S, p, W, W, xy, threads=8)
        a2, f2, st = S.render_pixels(p, W, W, xy, threads=8, fast=True)
    else:
        p = S.params(cam, accel_mode=1)
        band = (0, 20, W, 26)
        # one thread: the reference's thread_pool can lose a wake-up (see oracle/ref_harness.cpp)
        a1, f1, cnt = O.ref_render(S, p, W, W, rect=band, threads=1)
        a2, f2, st = S.render(p, W, W, rect=band, threads=8, fast=1)
    assert np.array_equal(bits(a1), bits(a2)) and np.array_equal(f1, f2)
    assert (int(cnt[0]), int(cnt[1])) == (st.locate_calls, st.samples_found)


def test_battery_reaches_every_range_case():
    """Every branch of the ray setup, the forms whose first range starts behind the camera
    included, is taken by at least 64 rays of some view, on each of the GPU tests' two scenes
    at their frame size (tests/test_gpu_views.py).  A condition on the battery, not a
    measurement: where a view falls short, its camera moves.  (Rays of the best view, flat /
    terrain: box miss 6336 away; in the box without a range 6336 corner_away; limb 1085 / 1023
    graze; two ranges 3891 framing; far only 6336 underground; limb from behind the camera
    788 / 740 shell_horizon; two ranges from behind 6336 shell_down; far only from behind 6336
    shell_up.)"""
    Wg, Hg = 88, 72
    for cells in (irt.synth_grid(2, 2, 47), irt.synth_grid(2, 2, 65, terrain=4000.0)):
        best = {}
        for name, cam in view_battery(cells).items():
            setup = irt.setup_frame(cells, Wg, Hg, camera=cam)
            label, behind, in_box = range_census(setup.lp, Wg, Hg, setup.info)
            n = {"box miss": ~in_box, "in the box, no range": in_box & (label == NO_RANGE)}
            for k in (LIMB_ONLY, TWO_RANGES, FAR_ONLY):
                n[RANGE_LABELS[k]] = (label == k) & ~behind
                n[RANGE_LABELS[k] + ", from behind the camera"] = (label == k) & behind
            for case, mask in n.items():
                if int(mask.sum()) > best.get(case, (0, ""))[0]:
                    best[case] = (int(mask.sum()), name)
            if name == "away":
                assert not in_box.any()
            if name == "corner_away":
                assert in_box.all() and (label == NO_RANGE).all()
            if name in ("underground", "centre"):
                assert ((label == FAR_ONLY) & ~behind).all()
            if name == "shell_down":
                assert ((label == TWO_RANGES) & behind).all()
        print(best)
        assert len(best) == 8 and all(v[0] >= 64 for v in best.values()), best
