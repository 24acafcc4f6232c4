"""The device point location of the two unstructured samplers -- Tracer::locate_wedge
(CUBQL_MODE) and Tracer::locate_tri (TRIANGLE_MODE), csrc/irt_render.hip -- point by point
against the oracle's brute-force scans, through irt_debug_locate_sampler, which runs the Tracer
instantiation of the samplers' frames over the context's own wedge locator and blocks.  Scenes
and points: tests/sampler_scenes.py (unsorted, reversed, repeated and zero-thickness records,
0 / 1 / 2 layers, the convert_icon layout, non-finite values, points exactly on layer radii,
shared edges and corners); the same comparison on the host twins, and the oracle against the
reference's own wedge scan, are in tests/test_samplers_cpu.py.  Bar: found flags equal, values
equal as bits, NaN equal to NaN (sampler_scenes.first_difference).

TRIANGLE_MODE's parity with the reference stays unpinned (OptiX's triangle test is not
reproducible): device, host twin and oracle share one ray_triangle definition."""
import numpy as np
import pytest

import accel_scenes
import irt
import sampler_scenes as S
from helpers import FRAMING, gpu_frame, oracle_frame, view_battery
from test_gpu_parity import assert_same_frame

pytestmark = pytest.mark.gpu

MODES = {"cubql": irt.MODE_CUBQL, "triangles": irt.MODE_TRIANGLES}


@pytest.fixture(scope="module")
def contexts():
    """name -> a context of scene(name) with its wedge accel, built once."""
    made = {}

    def get(name):
        if name not in made:
            cells = S.scene(name)
            made[name] = irt.Context(cells, 0)
            made[name].build_wedge_accel(cells)
        return made[name]

    yield get
    for ctx in made.values():
        ctx.close()


def _want(name, mode):
    return S.oracle_answers(name)[0 if mode == irt.MODE_CUBQL else 1]


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", S.SCENE_NAMES)
def test_device_sampler_matches_oracle_point_by_point(name, mode, contexts):
    ps = S.points(name)
    got = contexts(name).locate_sampler(ps.points, MODES[mode])
    want = _want(name, MODES[mode])
    print(f"{name} {mode}: {len(ps.points)} points, device found {int(got[0].sum())}, oracle {int(want[0].sum())}")
    S.assert_same_samples(name, ps, got, want, f"device {mode} sampler vs oracle")


def test_device_samplers_after_value_update():
    """The wedge accel holds the box, the layer count and the corner trig; the wedge scalars and
    the triangle sampler's getValue read the context's blocks.  A context of heights() geometry
    starts from other values, builds its accel, and is then updated in place to heights()'s and to
    nonfinite_values()'s values: both samplers must answer as the oracle does on the new records."""
    cells = np.array(S.scene("heights"), copy=True)
    cells["value"] = accel_scenes.untreated_values("heights")
    with irt.Context(cells, 0) as ctx:
        ctx.build_wedge_accel(cells)
        for name in ("heights", "nonfinite"):
            new = S.scene(name)
            assert new["height"].tobytes() == cells["height"].tobytes()
            ctx.update_values(np.ascontiguousarray(new["value"]))
            ctx.end_update()
            ps = S.points(name)
            for mode, m in MODES.items():
                S.assert_same_samples(name, ps, ctx.locate_sampler(ps.points, m), _want(name, m),
                                      f"device {mode} sampler after irt_update_values vs oracle")
    # the starting values answer differently: the update is what the comparison saw
    stale = S.oracle_answers("heights")[1]
    import oracle as O
    old = O.triangle_sample_points(cells, S.points("heights").points)
    assert S.first_difference(old[0], old[1], stale[0], stale[1]) >= 0


FRAME_SCENES = ("heights", "convert_icon")
FRAME_ALPHA = 0.02


@pytest.mark.parametrize("accel", [irt.ACCEL_SPHERE, irt.ACCEL_GRID], ids=["sphere", "grid"])
@pytest.mark.parametrize("view", ["framing", "shell_down"])
@pytest.mark.parametrize("name", FRAME_SCENES)
@pytest.mark.parametrize("mode", list(MODES))
def test_sampler_frames_on_edge_records(mode, name, view, accel):
    """48 x 48 frames of the edge-record scene and of the convert_icon layout through both
    samplers and both accelerators, accumIDs (0, 2), against the oracle: bit-identical, with equal
    sampleVolume calls and hits.  Each frame has covered pixels in the oracle (else it pins
    nothing).

    The transfer function is the default colours at a constant alpha of FRAME_ALPHA.  Every
    sampleVolume call of the oracle costs Newton iterations on each wedge whose box holds the
    point (about 0.5 ms), and the default alphas take up to 1.8 M calls for one grid-accel frame
    of these scenes, minutes on the CPU; a constant small alpha keeps the majorants low (a tenth
    of the calls or fewer), while every located sample is still accepted, so the frames stay
    covered (340 to 2300 of 2304 pixels in the oracle, 1 k to 100 k calls per frame)."""
    cells = S.scene(name)
    cam = FRAMING if view == "framing" else view_battery(cells)[view]
    W, ids = 48, (0, 2)
    setup = irt.setup_frame(cells, W, W, camera=cam)
    lut = setup.lut.copy()
    lut[:, 3] = FRAME_ALPHA
    a_ref, f_ref, st_ref, _ = oracle_frame(cells, W, W, camera=cam, accum_ids=ids, accel_mode=accel,
                                           mode=MODES[mode], threads=16, lut=lut,
                                           value_range=setup.value_range)
    assert (a_ref[..., 3] > 0).any(), "the oracle frame is empty: choose another camera"
    a_gpu, f_gpu, st_gpu, ctx = gpu_frame(cells, W, W, camera=cam, accum_ids=ids, accel_mode=accel,
                                          mode=MODES[mode], lut=lut, value_range=setup.value_range)
    try:
        assert_same_frame(a_gpu, f_gpu, a_ref, f_ref, f"{mode} {name} {view} accel {accel}")
        for g, o in zip(st_gpu, st_ref):
            assert (g.locateCalls, g.samplesFound) == (o.locate_calls, o.samples_found)
    finally:
        ctx.close()


def test_locate_sampler_argument_errors():
    cells = S.scene("single")
    pts = S.points("single").points[:8]
    with irt.Context(cells, 0) as ctx:
        with pytest.raises(irt.IrtError, match="irt_build_wedge_accel"):
            ctx.locate_sampler(pts, irt.MODE_CUBQL)
        with pytest.raises(irt.IrtError, match="irt_build_wedge_accel"):
            ctx.locate_sampler(pts, irt.MODE_TRIANGLES)
        ctx.build_wedge_accel(cells)
        for bad in (irt.MODE_USER_GEOM, 7):
            with pytest.raises(irt.IrtError, match="sampler mode"):
                ctx.locate_sampler(pts, bad)
        found, value = ctx.locate_sampler(pts[:0], irt.MODE_CUBQL)  # n == 0 is fine
        assert found.size == 0 and value.size == 0
        ctx.update_values(np.ascontiguousarray(cells["value"]))
        with pytest.raises(irt.IrtError, match="update is pending"):
            ctx.locate_sampler(pts, irt.MODE_CUBQL)
        ctx.end_update()
        ctx.locate_sampler(pts, irt.MODE_CUBQL)
