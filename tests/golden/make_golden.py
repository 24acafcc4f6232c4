#!/usr/bin/env python3
"""Generate tests/golden/*.npz from the REFERENCE's own code (oracle/_ref/libiconref.so,
compiled from /root/reference headers by oracle/Makefile `ref`).

Run in the build container (the only place /root/reference exists):
    make -C oracle ref && python tests/golden/make_golden.py

Each frame fixture holds its inputs (the `.ic` records, the LUT/value range, the camera
LaunchParams, accumIDs) and the reference outputs (accumBuffer float32 RGBA, fbPointer
RGBA8, sampleVolume call counts).  kats.npz holds single-function known answers from the
reference functions (LCG, sample, findHeight, intersectSphere, boxTest, sdda,
linear_to_srgb/make_rgba, toSpherical/toCartesian, getBounds, resampleLUT, Camera);
kats_grid.npz + f6_*_grid.npz the GRID_ACCEL_MODE path (dda3, buildGrid_ICON, a frame);
kats_wedge.npz + f7_*_wedge.npz the CUBQL_MODE sampler (intersectWedgeEXT, the wedge
sampleVolume, a frame); kats_wedge_edges.npz (`make_golden.py wedge_edges`) the wedge
sampleVolume on the edge records and points of tests/sampler_scenes.py.
f8_terrain_*.npz + kats_terrain.npz (`make_golden.py terrain`, which writes these files only)
pin the record layout convert_icon writes for real fields -- terrain-following heights, an
inverted first layer over land (height[0] > height[1]), zero-thickness top records (65
levels), voids under land: five frames of the reference raygen, and findHeight / sample /
sampleVolume known answers at the radii where that layout is unobvious.
f9_view_*.npz (`make_golden.py views`): four frames of the terrain scene from cameras of
helpers.view_battery -- inside the shell, under it, south of the globe (AE) and along the horizon
(grid).  Seventeen golden frames in all (f1 x 2, f2..f7, f8 x 5, f9 x 4) come from the reference's
own code.
ragged_frames.npz (`make_golden.py ragged`): eight more reference frames in one file, at 37 x 29
and 67 x 33 -- sizes that are no multiples of 8, where the frame edge cuts the kernels' 8 x 8
packets -- which pin the oracle the ragged-frame GPU tests compare with.
The `.ic` inputs are synthetic grids from icon-ray-tracing_amd's generator (real DWD data
is not available offline); they are stored verbatim, so the fixtures do not depend on it.
"""
import ctypes as C
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [os.path.join(ROOT, "icon-ray-tracing_amd", "python"), os.path.join(ROOT, "oracle"),
                os.path.join(ROOT, "tests")]

import irt  # noqa: E402  (grid generator only)
import oracle as O  # noqa: E402

FRAMING = irt.FRAMING_CAMERA

FRAMES = {
    # name: (rootN, bisections, levels, numCells cap, W, H, camera, accumIDs, raygen, tf
    #        [, terrain: max HSURF in metres of irt.synth_grid(..., terrain=), default 0])
    "f1_ico12_viewall": (1, 0, 4, 12, 256, 256, None, (0,), 0, "default"),
    "f1_ico12_framing": (1, 0, 4, 12, 256, 256, FRAMING, (0,), 0, "default"),
    "f2_r2b02_l90": (2, 2, 90, -1, 128, 128, FRAMING, (0,), 0, "default"),
    "f3_r2b00_l10_ae": (2, 0, 10, -1, 64, 64, FRAMING, (0,), 1, "default"),
    "f4_r2b01_l31_progressive": (2, 1, 31, -1, 64, 64, FRAMING, (0, 2, 3), 0, "default"),
    "f5_r2b01_l40_sparse": (2, 1, 40, -1, 64, 64, FRAMING, (0,), 0, "sparse"),
}

SPARSE_LUT5 = np.array([[0.1, 0.2, 0.9, 0.05], [0.9, 0.9, 0.2, 0.02], [0.8, 0.1, 0.1, 0.3]],
                       np.float32)


def make_frame(name, spec, mode=0, check=None, accel_mode=0, save=True, each=None):
    """save=False: nothing is written, the fixture's arrays are returned; each: a list that gets
    (accum, fb) copies after every accumID."""
    rn, bis, L, cap, W, H, cam, ids, raygen, tf = spec[:10]
    terrain = float(spec[10]) if len(spec) > 10 else 0.0
    cells = irt.synth_grid(rn, bis, L, noise=0.1 if tf == "sparse" else 0.0, terrain=terrain)
    if cap >= 0:
        cells = cells[:cap].copy()  # --num-cells (hostCode.cu:112-113,728-730)
    if isinstance(cam, str):  # a view of helpers.view_battery, from this scene's radii
        from helpers import view_battery
        cam = view_battery(cells)[cam]
    S = O.OracleScene(cells)
    # host setup restated with the reference's types (oracle/_ref)
    R = O.rlib()
    sb6, vb6, dr = np.zeros(6, np.float32), np.zeros(6, np.float32), np.zeros(2, np.float32)
    R.ref_compute_bounds(cells.ctypes.data, cells.size, sb6.ctypes.data, vb6.ctypes.data,
                         dr.ctypes.data)
    vr_ref = np.zeros((S.num_mcs, 2), np.float32)
    R.ref_build_shell(cells.ctypes.data, cells.size, S.dims.ctypes.data, sb6.ctypes.data,
                      vr_ref.ctypes.data)
    if tf == "sparse":
        lut = np.zeros((300, 4), np.float32)
        R.ref_resample_lut(SPARSE_LUT5.ctypes.data, 3, lut.ctypes.data, 300)
        vrange, opacity = (float(dr[0]), float(dr[1])), 0.5
    else:
        lut5 = np.array([[0.149, 0.015, 0.705, 1.0], [0.486, 0.603, 0.956, 0.75],
                         [0.866, 0.866, 0.866, 0.5], [0.996, 0.690, 0.552, 0.25],
                         [0.752, 0.298, 0.231, 0.0]], np.float32)
        lut = np.zeros((300, 4), np.float32)
        R.ref_resample_lut(lut5.ctypes.data, 5, lut.ctypes.data, 300)
        vrange = (float(dr[0]), float(dr[1])) if dr[1] > dr[0] else (0.0, 1.0)
        opacity = 1.0
    maxop = np.zeros(S.num_mcs, np.float32)
    R.ref_max_opacities(vr_ref.ctypes.data, S.num_mcs, lut.ctypes.data, 300, vrange[0],
                        vrange[1], maxop.ctypes.data)
    cam12 = np.zeros(12, np.float32)
    if cam is None:
        R.ref_camera(1, vb6.ctypes.data, np.zeros(9, np.float32).ctypes.data, 90.0,
                     cam12.ctypes.data)
    else:
        vp9 = np.array(list(cam[0]) + list(cam[1]) + list(cam[2]), np.float32)
        R.ref_camera(0, vb6.ctypes.data, vp9.ctypes.data, cam[3], cam12.ctypes.data)
    # hostCode.cu:944-945 divides by the image size
    cam12[6:9] = cam12[6:9] / np.float32(W)
    cam12[9:12] = cam12[9:12] / np.float32(H)
    # unitDistance = powf(10, floorf(log10f(R_inner)) - 3) (hostCode.cu:838-840)
    unit_c = C.c_float(O.olib().oracle_unit_distance(float(sb6[0]))).value
    S.set_transfunc(lut, vrange, opacity)
    S.max_op[:] = maxop
    S.value_ranges[:] = vr_ref
    accum = np.zeros((H, W, 4), np.float32)
    fb = np.zeros((H, W), np.uint32)
    counts = []
    if accel_mode == 1:  # GRID_ACCEL_MODE: the reference's own 256^3 grid and majorants
        S.build_grid()
        R.ref_build_grid(cells.ctypes.data, cells.size, S.grid_dims.ctypes.data, vb6.ctypes.data,
                         S.grid_vr.ctypes.data)
        R.ref_max_opacities(S.grid_vr.ctypes.data, S.grid_vr.shape[0], lut.ctypes.data, 300,
                            vrange[0], vrange[1], S.grid_max_op.ctypes.data)
    p = S.params((cam12[0:3], cam12[3:6], cam12[6:9], cam12[9:12]), raygen=raygen,
                 unit_distance=unit_c, mode=mode, accel_mode=accel_mode)
    for aid in ids:
        p.accumID = aid
        _, _, c = O.ref_render(S, p, W, H, accum=accum, fb=fb, threads=1)
        counts.append(c.copy())
        if each is not None:
            each.append((accum.copy(), fb.copy()))
    out = dict(
        cells=cells.view(np.uint8).reshape(cells.size, 284),
        width=W, height=H, camera12=cam12, accum_ids=np.array(ids, np.int32), raygen=raygen,
        lut=lut, value_range=np.array(vrange, np.float32), opacity_scale=np.float32(opacity),
        unit_distance=np.float32(unit_c), spherical_bounds=sb6, volume_bounds=vb6,
        data_range=dr, value_ranges=vr_ref, max_opacities=maxop, accum=accum, fb=fb,
        counts=np.array(counts, np.uint64), mode=mode)
    if accel_mode:
        out["accel_mode"] = accel_mode
    if check is not None:
        check(name, cells, out)  # before anything is written
    if not save:
        return out
    np.savez_compressed(os.path.join(HERE, name + ".npz"), **out)
    print(f"{name}: {cells.size} records {W}x{H}, hit {(accum[..., 3] > 0).mean():.3f}, "
          f"samples {counts}")


def make_kats():
    R = O.rlib()
    rng = np.random.default_rng(20261015)
    out = {}
    # LCG (dvr_course-common-both.h:41-86)
    seeds = np.array([[0, 0], [1, 0], [12345, 678], [0xFFFFFFFF, 7], [1048576 * 3 + 17, 511]],
                     np.uint32)
    lcg = np.zeros((len(seeds), 16), np.float32)
    for i, (a, b) in enumerate(seeds):
        R.ref_lcg(int(a), int(b), 16, lcg[i].ctypes.data)
    out["lcg_seeds"], out["lcg"] = seeds, lcg
    # cells for sample / findHeight / getBounds
    cells = irt.synth_grid(2, 1, 45, noise=0.3)[:200].copy()
    out["cells"] = cells.view(np.uint8).reshape(cells.size, 284)
    pts, idx = [], []
    for i in range(cells.size):
        c = cells[i]
        lat, lon = c["lat"].astype(np.float64), c["lon"].astype(np.float64)
        d = np.stack([np.cos(lat) * np.cos(lon), np.cos(lat) * np.sin(lon), np.sin(lat)], 1)
        for _ in range(6):
            w = rng.dirichlet([1, 1, 1]) * 1.3 - 0.1  # some outside the triangle
            r = rng.uniform(c["height"][0] - 500, c["height"][c["numLayers"]] + 500)
            v = (w @ d)
            pts.append((v / np.linalg.norm(v) * r).astype(np.float32))
            idx.append(i)
        # exactly on layer boundary heights
        v = d.mean(0)
        for j in (0, 1, c["numLayers"]):
            pts.append((v / np.linalg.norm(v) * np.float64(c["height"][j])).astype(np.float32))
            idx.append(i)
    pts, idx = np.array(pts, np.float32), np.array(idx, np.int32)
    hit, val = np.zeros(len(pts), np.int32), np.zeros(len(pts), np.float32)
    for k, (p, i) in enumerate(zip(pts, idx)):
        v = C.c_float(0)
        hit[k] = R.ref_sample(cells[i:i + 1].ctypes.data, p.ctypes.data, C.byref(v))
        val[k] = v.value
    out["sample_points"], out["sample_cell"], out["sample_hit"], out["sample_value"] = pts, idx, hit, val
    fh_h = np.concatenate([cells[i]["height"][:cells[i]["numLayers"] + 1] for i in range(20)])
    fh_i = np.concatenate([[i] * (cells[i]["numLayers"] + 1) for i in range(20)]).astype(np.int32)
    fh_h = np.concatenate([fh_h, fh_h + 0.25, fh_h - 0.25]).astype(np.float32)
    fh_i = np.concatenate([fh_i, fh_i, fh_i])
    out["fh_cell"], out["fh_h"] = fh_i, fh_h
    out["fh_result"] = np.array([R.ref_find_height(cells[i:i + 1].ctypes.data, float(h))
                                 for i, h in zip(fh_i, fh_h)], np.int32)
    gb = np.zeros((cells.size, 6), np.float32)
    for i in range(cells.size):
        R.ref_get_bounds(cells[i:i + 1].ctypes.data, gb[i].ctypes.data)
    out["get_bounds"] = gb
    # rays: intersectSphere, boxTest, sdda
    n = 300
    org = np.zeros((n, 3), np.float32)
    org[:] = (rng.normal(size=(n, 3)) * 1e7).astype(np.float32)
    org[:20] = (rng.normal(size=(20, 3)) * 2e6).astype(np.float32)  # inside the inner sphere
    tgt = (rng.normal(size=(n, 3)) * 5e6).astype(np.float32)
    dirs = (tgt - org)
    dirs = (dirs / np.linalg.norm(dirs, axis=1, keepdims=True)).astype(np.float32)
    out["ray_org"], out["ray_dir"] = org, dirs
    sph = np.zeros((n, 4), np.float32)
    for k in range(n):
        tn, tf = C.c_float(), C.c_float()
        h = R.ref_intersect_sphere(org[k].ctypes.data, dirs[k].ctypes.data, 6.4e6, C.byref(tn), C.byref(tf))
        sph[k] = [h, tn.value, tf.value, 0]
    out["sphere"] = sph
    box6 = np.array([-6.5e6, -6.4e6, -6.3e6, 6.5e6, 6.4e6, 6.3e6], np.float32)
    bt = np.zeros((n, 3), np.float32)
    for k in range(n):
        t0, t1 = C.c_float(), C.c_float()
        h = R.ref_box_test(org[k].ctypes.data, dirs[k].ctypes.data, 0.0, 1e10, box6.ctypes.data,
                           C.byref(t0), C.byref(t1))
        bt[k] = [h, t0.value, t1.value]
    out["box6"], out["box_test"] = box6, bt
    dims = np.array([1, 1024, 1024], np.int32)
    sb6 = np.array([6.371229e6, -1.5707964, -3.1415927, 6.446229e6, 1.5707964, 3.1415927], np.float32)
    maxo = 2048
    leaves = np.full((n, maxo), -1, np.int32)
    lt0 = np.zeros((n, maxo), np.float32)
    lt1 = np.zeros((n, maxo), np.float32)
    cnt = np.zeros(n, np.int32)
    for k in range(n):
        cnt[k] = R.ref_sdda_trace(org[k].ctypes.data, dirs[k].ctypes.data, 0.0, 1e10,
                                  dims.ctypes.data, sb6.ctypes.data, maxo, leaves[k].ctypes.data,
                                  lt0[k].ctypes.data, lt1[k].ctypes.data)
    out["sdda_dims"], out["sdda_sb6"], out["sdda_count"] = dims, sb6, cnt
    out["sdda_leaf"], out["sdda_t0"], out["sdda_t1"] = leaves, lt0, lt1
    # shading
    xs = np.concatenate([rng.uniform(-0.1, 1.2, 4000), np.linspace(0, 0.01, 500),
                         [0.0031308, 0.0031309, 1.0, 0.0]]).astype(np.float32)
    out["srgb_x"] = xs
    out["srgb"] = np.array([R.ref_linear_to_srgb(float(x)) for x in xs], np.float32)
    cols = rng.uniform(-0.2, 1.2, (1000, 4)).astype(np.float32)
    out["rgba_in"] = cols
    out["rgba"] = np.array([R.ref_make_rgba(c.ctypes.data) for c in cols], np.uint32)
    # toSpherical / toCartesian
    cart = (rng.normal(size=(2000, 3)) * 6.4e6).astype(np.float32)
    out["cart"], out["to_spherical"] = cart, np.zeros_like(cart)
    for k in range(len(cart)):
        R.ref_to_spherical(cart[k].ctypes.data, out["to_spherical"][k].ctypes.data)
    sp = np.stack([rng.uniform(6.3e6, 6.5e6, 2000), rng.uniform(-1.6, 1.6, 2000),
                   rng.uniform(-3.2, 3.2, 2000)], 1).astype(np.float32)
    out["sph"], out["to_cartesian"] = sp, np.zeros_like(sp)
    for k in range(len(sp)):
        R.ref_to_cartesian(sp[k].ctypes.data, out["to_cartesian"][k].ctypes.data)
    # resampleLUT + Camera
    src = rng.uniform(0, 1, (7, 4)).astype(np.float32)
    dst = np.zeros((300, 4), np.float32)
    R.ref_resample_lut(src.ctypes.data, 7, dst.ctypes.data, 300)
    out["lut_src"], out["lut_300"] = src, dst
    cams = []
    vb6 = np.array([-6.4e6, -6.4e6, -6.4e6, 6.4e6, 6.4e6, 6.4e6], np.float32)
    c12 = np.zeros(12, np.float32)
    R.ref_camera(1, vb6.ctypes.data, np.zeros(9, np.float32).ctypes.data, 90.0, c12.ctypes.data)
    cams.append(c12.copy())
    for vp9, fov in [([0, 0, 1.4e7, 0, 0, 0, 0, 1, 0], 60.0), ([3e6, -2e7, 1e6, 1e5, 0, -2e5, 0, 0, 1], 35.0),
                     ([1e7, 1e7, 1e7, 0, 0, 0, 0, 1, 0], 0.0)]:
        v = np.array(vp9, np.float32)
        R.ref_camera(0, vb6.ctypes.data, v.ctypes.data, fov, c12.ctypes.data)
        cams.append(c12.copy())
    out["camera_box6"], out["cameras"] = vb6, np.array(cams)
    out["camera_specs"] = np.array([[0, 0, 1.4e7, 0, 0, 0, 0, 1, 0, 60.0],
                                    [3e6, -2e7, 1e6, 1e5, 0, -2e5, 0, 0, 1, 35.0],
                                    [1e7, 1e7, 1e7, 0, 0, 0, 0, 1, 0, 0.0]], np.float32)
    np.savez_compressed(os.path.join(HERE, "kats.npz"), **out)
    print("kats:", {k: v.shape for k, v in out.items()})


def make_grid_fixtures(frame=True):
    """GRID_ACCEL_MODE (Params.h:34): dda3 known answers from DDA.h itself, the 256^3
    buildGrid_ICON value ranges (hostCode.cu:205-297) as a digest plus sampled entries, and
    one frame of woodcockTrackingWithAccel with accelMode = GRID_ACCEL_MODE."""
    import hashlib
    R = O.rlib()
    rng = np.random.default_rng(20261016)
    out = {}
    n = 400
    org = (rng.normal(size=(n, 3)) * 1.4e7).astype(np.float32)
    org[:30] = (rng.normal(size=(30, 3)) * 2e6).astype(np.float32)  # starting inside the grid
    tgt = (rng.normal(size=(n, 3)) * 3e6).astype(np.float32)
    dirs = tgt - org
    dirs = (dirs / np.linalg.norm(dirs, axis=1, keepdims=True)).astype(np.float32)
    dirs[:10, 0] = np.float32(1e-5)  # generateRay's clamped components
    tmin = rng.uniform(0, 1e7, n).astype(np.float32)
    tmin[:100] = 0.0
    tmax = (tmin + rng.uniform(1e3, 3e7, n)).astype(np.float32)
    dims_all = np.zeros((n, 3), np.int32)
    dims_all[:] = (256, 256, 256)
    dims_all[300:] = rng.integers(1, 40, (n - 300, 3))  # ragged grids
    wb6 = np.array([-6.45e6, -6.44e6, -6.43e6, 6.45e6, 6.44e6, 6.43e6], np.float32)
    maxo = 2048
    leaves = np.full((n, maxo), -1, np.int32)
    lt0 = np.zeros((n, maxo), np.float32)
    lt1 = np.zeros((n, maxo), np.float32)
    cnt = np.zeros(n, np.int32)
    for k in range(n):
        cnt[k] = R.ref_dda3_trace(org[k].ctypes.data, dirs[k].ctypes.data, float(tmin[k]),
                                  float(tmax[k]), dims_all[k].ctypes.data, wb6.ctypes.data, maxo,
                                  leaves[k].ctypes.data, lt0[k].ctypes.data, lt1[k].ctypes.data)
    out.update(dda3_org=org, dda3_dir=dirs, dda3_tmin=tmin, dda3_tmax=tmax, dda3_dims=dims_all,
               dda3_wb6=wb6, dda3_count=cnt, dda3_leaf=leaves, dda3_t0=lt0, dda3_t1=lt1)
    # buildGrid_ICON over a synthetic R2B02 x 60 scene
    cells = irt.synth_grid(2, 2, 60, noise=0.2)
    sb6, vb6, dr = np.zeros(6, np.float32), np.zeros(6, np.float32), np.zeros(2, np.float32)
    R.ref_compute_bounds(cells.ctypes.data, cells.size, sb6.ctypes.data, vb6.ctypes.data,
                         dr.ctypes.data)
    gdims = np.array([256, 256, 256], np.int32)
    gvr = np.zeros((256 ** 3, 2), np.float32)
    R.ref_build_grid(cells.ctypes.data, cells.size, gdims.ctypes.data, vb6.ctypes.data,
                     gvr.ctypes.data)
    pick = np.sort(np.concatenate([rng.choice(256 ** 3, 20000, replace=False),
                                   rng.choice(np.flatnonzero(gvr[:, 1] >= gvr[:, 0]), 20000,
                                              replace=False)]))
    out.update(grid_cells=cells.view(np.uint8).reshape(cells.size, 284), grid_vb6=vb6,
               grid_sha256=np.frombuffer(hashlib.sha256(gvr.tobytes()).digest(), np.uint8),
               grid_nonempty=np.int64((gvr[:, 1] >= gvr[:, 0]).sum()), grid_pick=pick,
               grid_pick_vr=gvr[pick])
    lut5 = np.array([[0.149, 0.015, 0.705, 1.0], [0.486, 0.603, 0.956, 0.75],
                     [0.866, 0.866, 0.866, 0.5], [0.996, 0.690, 0.552, 0.25],
                     [0.752, 0.298, 0.231, 0.0]], np.float32)
    lut = np.zeros((300, 4), np.float32)
    R.ref_resample_lut(lut5.ctypes.data, 5, lut.ctypes.data, 300)
    gmo = np.zeros(256 ** 3, np.float32)
    R.ref_max_opacities(gvr.ctypes.data, 256 ** 3, lut.ctypes.data, 300, float(dr[0]),
                        float(dr[1]), gmo.ctypes.data)
    out.update(grid_lut=lut, grid_value_range=dr.copy(),
               grid_maxop_sha256=np.frombuffer(hashlib.sha256(gmo.tobytes()).digest(), np.uint8),
               grid_pick_maxop=gmo[pick])
    np.savez_compressed(os.path.join(HERE, "kats_grid.npz"), **out)
    print("kats_grid:", cnt.sum(), "dda3 leaves;", int(out["grid_nonempty"]), "non-empty MCs")
    if not frame:
        return
    # one GRID_ACCEL_MODE frame (the sphere-mode machinery of make_frame, accelMode 1)
    W = H = 80
    S = O.OracleScene(cells)
    vr_ref = np.zeros((S.num_mcs, 2), np.float32)
    R.ref_build_shell(cells.ctypes.data, cells.size, S.dims.ctypes.data, sb6.ctypes.data,
                      vr_ref.ctypes.data)
    S.value_ranges[:] = vr_ref
    S.set_transfunc(lut, (float(dr[0]), float(dr[1])), 1.0)
    S.build_grid()
    S.grid_vr[:] = gvr
    S.grid_max_op[:] = gmo
    cam12 = np.zeros(12, np.float32)
    vp9 = np.array(list(FRAMING[0]) + list(FRAMING[1]) + list(FRAMING[2]), np.float32)
    R.ref_camera(0, vb6.ctypes.data, vp9.ctypes.data, FRAMING[3], cam12.ctypes.data)
    cam12[6:9] = cam12[6:9] / np.float32(W)
    cam12[9:12] = cam12[9:12] / np.float32(H)
    unit_c = C.c_float(O.olib().oracle_unit_distance(float(sb6[0]))).value
    p = S.params((cam12[0:3], cam12[3:6], cam12[6:9], cam12[9:12]), raygen=0,
                 unit_distance=unit_c, accel_mode=1)
    accum = np.zeros((H, W, 4), np.float32)
    fb = np.zeros((H, W), np.uint32)
    _, _, c = O.ref_render(S, p, W, H, accum=accum, fb=fb, threads=1)
    np.savez_compressed(
        os.path.join(HERE, "f6_r2b02_l60_grid.npz"),
        cells=cells.view(np.uint8).reshape(cells.size, 284), width=W, height=H, camera12=cam12,
        accum_ids=np.array([0], np.int32), raygen=0, accel_mode=1, lut=lut,
        value_range=dr.copy(), opacity_scale=np.float32(1.0), unit_distance=np.float32(unit_c),
        spherical_bounds=sb6, volume_bounds=vb6, data_range=dr, accum=accum, fb=fb,
        counts=np.array([c.copy()], np.uint64))
    print(f"f6_r2b02_l60_grid: {cells.size} records {W}x{H}, "
          f"hit {(accum[..., 3] > 0).mean():.3f}, samples {c}")


def make_wedge_fixtures():
    """CUBQL_MODE (Params.h:31): intersectWedgeEXT known answers from UElems.h itself, the
    wedge sampleVolume of deviceCode.cu:90-115 over buildCuBQLAccel's wedges (hostCode.cu:
    557-600) at points around a scene, and one frame with volume.mode = CUBQL_MODE."""
    R = O.rlib()
    rng = np.random.default_rng(20261017)
    out = {}
    # single wedges: random prisms (general, thin/flat, and Earth-scale ICON-like)
    nW = 600
    V = np.zeros((nW, 6, 4), np.float32)
    P = np.zeros((nW, 3), np.float32)
    for k in range(nW):
        if k < 200:
            tri = rng.normal(size=(3, 3))
            off = rng.normal(size=3) * 0.3 + np.array([0, 0, 1.0])
            V[k, :3, :3] = tri
            V[k, 3:, :3] = tri + off
            scale = 1.0
        else:
            lat = rng.uniform(-1.5, 1.5) + rng.normal(size=3) * (0.02 if k < 400 else 0.2)
            lon = rng.uniform(-3.1, 3.1) + rng.normal(size=3) * (0.02 if k < 400 else 0.2)
            h0 = 6.371229e6 + rng.uniform(0, 7e4)
            h1 = h0 + rng.uniform(10, 3000)
            d = np.stack([np.cos(lat) * np.cos(lon), np.cos(lat) * np.sin(lon), np.sin(lat)], 1)
            V[k, :3, :3] = d * h0
            V[k, 3:, :3] = d * h1
            scale = 0.0
        V[k, :, 3] = rng.uniform(0, 1)
        w = rng.dirichlet([1, 1, 1]) * 1.3 - 0.1
        tt = rng.uniform(-0.2, 1.2)
        P[k] = ((1 - tt) * (w @ V[k, :3, :3]) + tt * (w @ V[k, 3:, :3])).astype(np.float32)
        del scale
    hit = np.zeros(nW, np.int32)
    val = np.zeros(nW, np.float32)
    for k in range(nW):
        v = C.c_float(0)
        hit[k] = R.ref_intersect_wedge(V[k].ctypes.data, P[k].ctypes.data, C.byref(v))
        val[k] = v.value
    out.update(wedge_v=V, wedge_p=P, wedge_hit=hit, wedge_value=val)
    # sampleVolume in CUBQL_MODE over a scene's wedges
    cells = irt.synth_grid(2, 2, 20, noise=0.3)
    pts = []
    for _ in range(4000):
        c = cells[rng.integers(cells.size)]
        lat, lon = c["lat"].astype(np.float64), c["lon"].astype(np.float64)
        d = np.stack([np.cos(lat) * np.cos(lon), np.cos(lat) * np.sin(lon), np.sin(lat)], 1)
        w = rng.dirichlet([1, 1, 1]) * 1.4 - 0.13
        r = rng.uniform(c["height"][0] - 2000, c["height"][c["numLayers"]] + 2000)
        v = w @ d
        pts.append((v / np.linalg.norm(v) * r).astype(np.float32))
    pts = np.array(pts, np.float32)
    shit = np.zeros(len(pts), np.int32)
    sval = np.zeros(len(pts), np.float32)
    for k in range(len(pts)):
        v = C.c_float(0)
        shit[k] = R.ref_wedge_sample(cells.ctypes.data, cells.size, pts[k].ctypes.data, C.byref(v))
        sval[k] = v.value
    out.update(scene_cells=cells.view(np.uint8).reshape(cells.size, 284), scene_points=pts,
               scene_hit=shit, scene_value=sval)
    np.savez_compressed(os.path.join(HERE, "kats_wedge.npz"), **out)
    print("kats_wedge:", int(hit.sum()), "of", nW, "wedge hits;", int(shit.sum()), "of",
          len(pts), "scene hits")
    # one CUBQL_MODE frame
    make_frame("f7_r2b02_l20_wedge", (2, 2, 20, -1, 64, 64, FRAMING, (0,), 0, "default"),
               mode=2)
    make_wedge_edge_fixture()


WEDGE_EDGE_SCENES = ("heights", "nonfinite", "convert_icon")  # of tests/sampler_scenes.py
WEDGE_EDGE_POINTS = 1000  # per scene, a seeded subset of sampler_scenes.points(name)


def make_wedge_edge_fixture():
    """kats_wedge_edges.npz (`make_golden.py wedge_edges` writes this file only): the reference's
    wedge sampleVolume (ref_wedge_sample) on the edge records of tests/sampler_scenes.py --
    unsorted, reversed and repeated heights, records of 0, 1 and 2 layers, NaN / inf / FLT_MAX
    values, the convert_icon layout -- at a subset of those scenes' points.  Per scene: the
    records as bytes (transposed: byte k of every record in row k), the points, their indices in the scene's point set, hit and value."""
    import sampler_scenes as S
    out = {}
    for name in WEDGE_EDGE_SCENES:
        cells, ps = S.scene(name), S.points(name)
        rng = np.random.default_rng(20261019)
        pick = np.sort(rng.choice(len(ps.points), WEDGE_EDGE_POINTS, replace=False))
        pts = np.ascontiguousarray(ps.points[pick])
        hit, val = O.ref_wedge_sample_points(cells, pts)
        # the records' bytes transposed (284, n): byte planes deflate to about half
        out.update({f"cells_{name}": np.ascontiguousarray(np.array(cells).view(np.uint8).reshape(cells.size, 284).T),
                    f"points_{name}": pts, f"index_{name}": pick.astype(np.int32),
                    f"hit_{name}": hit, f"value_{name}": val})
        print(f"kats_wedge_edges {name}: {int(hit.sum())} of {len(pts)} hits, "
              f"{int(np.isnan(val).sum())} NaN values")
    path = os.path.join(HERE, "kats_wedge_edges.npz")
    np.savez_compressed(path, **out)
    n = os.path.getsize(path)
    print(f"kats_wedge_edges.npz: {n} bytes")
    assert n <= os.path.getsize(os.path.join(HERE, "kats_wedge.npz")), n


TERRAIN_FRAMES = {
    "f8_terrain_r2b02_l90": (2, 2, 90, -1, 128, 128, FRAMING, (0,), 0, "default", 4000.0),
    "f8_terrain_r2b02_l65_progressive": (2, 2, 65, -1, 96, 96, FRAMING, (0, 2, 3), 0, "default",
                                         4000.0),
    "f8_terrain_r2b01_l90_viewall": (2, 1, 90, -1, 96, 96, None, (0,), 0, "default", 4000.0),
    "f8_terrain_r2b01_l90_ae": (2, 1, 90, -1, 64, 64, FRAMING, (0,), 1, "default", 4000.0),
    "f8_terrain_r2b01_l65_sparse": (2, 1, 65, -1, 64, 64, FRAMING, (0,), 0, "sparse", 4000.0),
}
MAX_FIXTURE_BYTES = 1263401  # kats_grid.npz, the largest fixture before the terrain ones


def check_terrain_frame(name, cells, out):
    """The properties a terrain frame fixture exists for, asserted on the reference's data."""
    nl = cells["numLayers"]
    inverted = int(((nl > 0) & (cells["height"][:, 0] > cells["height"][:, 1])).sum())
    zero = int((nl == 0).sum())
    vr, mo = out["value_ranges"], out["max_opacities"]
    inv_mc = int((vr[:, 1] < vr[:, 0]).sum())  # (FLT_MAX, -FLT_MAX): no record reached it
    nonempty_zero_majorant = int(((vr[:, 1] >= vr[:, 0]) & (mo == 0)).sum())
    counts = out["counts"]
    voids = [int(c[0] - c[1]) for c in counts]
    hit = float((out["accum"][..., 3] > 0).mean())
    # pixels whose centre ray meets the scene's outer sphere: the most a frame can hit
    c, W, H = out["camera12"].astype(np.float64), int(out["width"]), int(out["height"])
    ys, xs = np.mgrid[0:H, 0:W]
    d = c[3:6] + (xs[..., None] + 1.0) * c[6:9] + (ys[..., None] + 1.0) * c[9:12]
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    b = d @ c[0:3]
    disc = float((b * b - (c[0:3] @ c[0:3] - float(out["spherical_bounds"][3]) ** 2) > 0).mean())
    print(f"{name}: inverted records {inverted}, zero-thickness records {zero}, void samples "
          f"{voids}, inverted macrocells {inv_mc}, non-empty macrocells with majorant 0 "
          f"{nonempty_zero_majorant}, hit fraction {hit:.3f} (globe covers {disc:.3f})")
    assert inverted >= 1, name
    if "_l65" in name:
        assert zero >= 1, name
    assert all(c[0] > c[1] for c in counts), name
    # at least 0.3 of the frame; the view-all camera (90 degrees, the whole box in view) shows
    # the globe on ~0.1 of the frame, so there the bound is 0.3 of the pixels that can hit
    assert hit >= (0.3 * disc if "_viewall" in name else 0.3), name
    assert inv_mc >= 1, name


def _corner_dirs(c):
    lat, lon = c["lat"].astype(np.float64), c["lon"].astype(np.float64)
    return np.stack([np.cos(lat) * np.cos(lon), np.cos(lat) * np.sin(lon), np.sin(lat)], 1)


def _radius32(p):
    """|p| as toSpherical computes it: sqrtf(x*x + y*y + z*z) in float."""
    p = np.asarray(p, np.float32)
    return np.sqrt(np.float32(np.float32(p[0] * p[0] + p[1] * p[1]) + p[2] * p[2]))


def make_terrain_kats_grid(cells, rng, zero_thickness):
    """Known answers on one convert_icon-layout grid: see make_terrain_kats."""
    from golden_util import terrain_fh_probes
    from helpers import on_radius
    import hashlib
    R = O.rlib()
    up, dn = np.float32(np.inf), np.float32(-np.inf)
    out = {"cells": cells.view(np.uint8).reshape(cells.size, 284)}
    # ---- findHeight
    fi, fh = terrain_fh_probes(cells)
    res = np.array([R.ref_find_height(cells[i:i + 1].ctypes.data, float(h))
                    for i, h in zip(fi, fh)], np.int32)
    assert res.min() >= 0 and res.max() <= 31
    out["fh_result"] = res.astype(np.int8)
    out["fh_sha256"] = np.frombuffer(hashlib.sha256(fi.tobytes() + fh.tobytes()).digest(), np.uint8)
    # ---- per-cell sample(): inside and just outside the triangle, at the radii that matter
    H0 = cells["height"][:, 0]
    top = cells["height"][np.arange(cells.size), cells["numLayers"]]
    inverted = (cells["numLayers"] > 0) & (H0 > cells["height"][:, 1])
    pts, idx = [], []
    ncol = cells.size // 3
    for c in range(0, ncol, 4):
        for i in range(3 * c, 3 * c + 3):
            cell = cells[i]
            cd = _corner_dirs(cell)
            nl = int(cell["numLayers"])
            h = cell["height"]
            base = [h[0], h[1], h[nl]] if nl > 0 else [h[0]]
            radii = [r for b in base for r in (b, np.nextafter(b, up), np.nextafter(b, dn))]
            if nl > 0 and h[0] > h[1]:  # inside the inverted first layer
                radii.append(np.float32((np.float64(h[0]) + np.float64(h[1])) * 0.5))
            e = 2e-2 if i % 2 else 1e-4
            k = int(rng.integers(3))
            w_out = np.full(3, 0.5 + e / 2)
            w_out[k] = -e  # just beyond the edge opposite corner k
            for w in (rng.dirichlet([2, 2, 2]), w_out):
                for r in radii:
                    pts.append(on_radius(w @ cd, r))
                    idx.append(i)
    pts, idx = np.array(pts, np.float32), np.array(idx, np.int32)
    hit, val = np.zeros(len(pts), np.uint8), np.zeros(len(pts), np.float32)
    for k, (p, i) in enumerate(zip(pts, idx)):
        v = C.c_float(0)
        hit[k] = R.ref_sample(cells[i:i + 1].ctypes.data, p.ctypes.data, C.byref(v))
        val[k] = v.value if hit[k] else 0.0
    out.update(sample_points=pts, sample_cell=idx, sample_hit=hit, sample_value=val)
    # ---- scene-level sampleVolume
    sbl, sbu = float(H0.min()), float(top.max())
    sp = list(pts[::3])
    land = [c for c in range(ncol) if inverted[3 * c]]
    assert len(land) > ncol // 4
    for c in rng.choice(ncol, 100, replace=False):  # shared edges and a corner
        cell = cells[3 * c]
        cd = _corner_dirs(cell)
        hs = float(H0[3 * c]) - sbl  # this column's surface above the lowest one
        for a, b in ((0, 1), (1, 2), (2, 0)):
            for r in (H0[3 * c], np.float32(sbl + 0.5 * hs + 1.0), top[3 * c + 2]):
                sp.append(on_radius(cd[a] + cd[b], r))
        sp.append(on_radius(cd[0], np.nextafter(H0[3 * c], up)))
    for c in rng.choice(land, 260):  # the void under a land column, and inside its first record
        cd = _corner_dirs(cells[3 * c])
        w = rng.dirichlet([3, 3, 3])
        sp.append(on_radius(w @ cd, np.float32(rng.uniform(sbl, float(H0[3 * c])))))
        w = rng.dirichlet([3, 3, 3])
        sp.append(on_radius(w @ cd, np.float32(rng.uniform(float(H0[3 * c]), float(top[3 * c])))))
    for c in rng.choice(land, 80):  # the void over a land column's top
        cd = _corner_dirs(cells[3 * c])
        sp.append(on_radius(rng.dirichlet([3, 3, 3]) @ cd,
                            np.float32(rng.uniform(float(top[3 * c + 2]) + 1.0, sbu))))
    for c in rng.choice(ncol, 120):  # above the top of everything, below the bottom
        cd = _corner_dirs(cells[3 * c])
        off = rng.uniform(1.0, 500.0)
        sp.append(((rng.dirichlet([3, 3, 3]) @ cd) * (sbu + off if c % 3 else sbl - off)).astype(np.float32))
    if zero_thickness:  # a zero-thickness record accepts every direction at its one radius
        for c in rng.choice(ncol, 60, replace=False):
            i = 3 * c + 2
            assert cells["numLayers"][i] == 0
            cd = _corner_dirs(cells[i])
            for r in (H0[i], np.nextafter(H0[i], up), np.nextafter(H0[i], dn)):
                sp.append(on_radius(cd.sum(0), r))
            sp.append(on_radius(rng.normal(size=3), H0[i]))
    d = rng.normal(size=(300, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    sp += list((d * rng.uniform(sbl - 50, sbu + 50, (300, 1))).astype(np.float32))
    sp = np.array(sp, np.float32)
    found, value, index = O.ref_sample_volume(cells, sp)
    out.update(scene_points=sp, scene_found=found.astype(np.uint8), scene_value=value,
               scene_index=index)
    rad = np.array([_radius32(p) for p in sp], np.float32)
    stats = dict(points=len(sp), hits=int(found.sum()),
                 voids=int(((found == 0) & (rad >= np.float32(sbl)) & (rad <= np.float32(sbu))).sum()),
                 inverted_hits=int(inverted[index[found == 1]].sum()),
                 zero_thickness=int(np.isin(rad, H0[cells["numLayers"] == 0]).sum()),
                 fh_probes=len(fh), sample_probes=len(pts), sample_hits=int(hit.sum()))
    return out, stats


def make_terrain_kats():
    """kats_terrain.npz: ICONCell::findHeight, sample() and the CPU sampleVolume loop
    (ICONGrid.h:117-145, 181-208; deviceCode.cu:119-122) from the reference's own code on the
    records of synth_grid(2, 1, 90 | 65, terrain=4000): 960 records each, stored in the file."""
    rng = np.random.default_rng(20261019)
    out, total = {}, {}
    for tag, L in (("l90", 90), ("l65", 65)):
        cells = irt.synth_grid(2, 1, L, terrain=4000.0)
        assert cells.size == 960
        o, st = make_terrain_kats_grid(cells, rng, zero_thickness=(L == 65))
        print(f"kats_terrain {tag}: {st}")
        out.update({f"{k}_{tag}": v for k, v in o.items()})
        for k, v in st.items():
            total[k] = total.get(k, 0) + v
    print(f"kats_terrain: {total}")
    # conditions on the inputs (the point recipe above is chosen so the reference meets them)
    assert 3 * total["hits"] >= total["points"], total
    assert total["voids"] >= 200 and total["inverted_hits"] >= 200, total
    assert total["zero_thickness"] >= 50, total
    np.savez_compressed(os.path.join(HERE, "kats_terrain.npz"), **out)


def make_terrain_fixtures():
    for name, spec in TERRAIN_FRAMES.items():
        make_frame(name, spec, check=check_terrain_frame)
    make_terrain_kats()
    for name in list(TERRAIN_FRAMES) + ["kats_terrain"]:
        n = os.path.getsize(os.path.join(HERE, name + ".npz"))
        print(f"{name}.npz: {n} bytes")
        assert n <= MAX_FIXTURE_BYTES, (name, n)


VIEW_FRAMES = {
    # name: (FRAMES-style spec whose camera names a view of helpers.view_battery, accelMode)
    "f9_view_shell_down": ((2, 1, 90, -1, 48, 40, "shell_down", (0, 2, 3), 0, "default", 4000.0), 0),
    "f9_view_underground": ((2, 1, 90, -1, 48, 40, "underground", (0,), 0, "default", 4000.0), 0),
    "f9_view_south_oblique_ae": ((2, 1, 90, -1, 48, 40, "south_oblique", (0,), 1, "default", 4000.0), 0),
    "f9_view_shell_horizon_grid": ((2, 1, 90, -1, 48, 40, "shell_horizon", (0,), 0, "default", 4000.0), 1),
}


def make_view_fixtures():
    largest = max(os.path.getsize(os.path.join(HERE, f)) for f in os.listdir(HERE)
                  if f.endswith(".npz") and not f.startswith("f9_view_"))
    for name, (spec, accel) in VIEW_FRAMES.items():
        make_frame(name, spec, accel_mode=accel)
        n = os.path.getsize(os.path.join(HERE, name + ".npz"))
        print(f"{name}.npz: {n} bytes")
        assert n <= min(largest, 1 << 20), (name, n, largest)


RAGGED_SIZES = ((37, 29), (67, 33))  # no multiples of 8: the frame edge cuts 8 x 8 packets


def make_ragged_fixture():
    """ragged_frames.npz (`make_golden.py ragged` writes this file only): the reference's raygen
    on the flat scene of tests/ragged_scenes.py, synth_grid(2, 1, 20), at sizes that are no
    multiples of 8, under FRAMING and viewAll, accumIDs 0 and 1: accum, fb and (sampleVolume calls,
    found) after each frame.  The scene's inputs are stored once (records as transposed bytes),
    the camera per frame."""
    out = {}
    for W, H in RAGGED_SIZES:
        for tag, cam in (("framing", FRAMING), ("viewall", None)):
            each = []
            d = make_frame("", (2, 1, 20, -1, W, H, cam, (0, 1), 0, "default"), save=False, each=each)
            if not out:
                out.update(cells=np.ascontiguousarray(d["cells"].T), lut=d["lut"], value_range=d["value_range"],
                           opacity_scale=d["opacity_scale"], unit_distance=d["unit_distance"],
                           raygen=d["raygen"], accum_ids=d["accum_ids"])
            key = f"{W}x{H}_{tag}"
            out.update({f"camera12_{key}": d["camera12"], f"accum_{key}": np.array([e[0] for e in each]),
                        f"fb_{key}": np.array([e[1] for e in each]), f"counts_{key}": d["counts"]})
            print(f"ragged {key}: hit {(each[-1][0][..., 3] > 0).mean():.3f}, counts {d['counts'].tolist()}")
    path = os.path.join(HERE, "ragged_frames.npz")
    np.savez_compressed(path, **out)
    n = os.path.getsize(path)
    print(f"ragged_frames.npz: {n} bytes")
    assert n <= 1 << 19, n


def make_raymath_kats():
    """kats_raymath.npz (`make_golden.py raymath` writes this file only): the reference build's answers on
    the cases of tests/raymath_cases.py -- its f32 division on the division pairs (every
    raymath_cases.KAT_STRIDE-th pair of each list), postClassify under every transfer function on the
    thinned value lists (every edge case kept), boxTest / intersectSphere on the rays, generateRay per
    pixel (16 x 16 whole, every seventh pixel of 67 x 33)."""
    import raymath_cases as RC
    R = O.rlib()
    p = lambda a: a.ctypes.data  # noqa: E731
    out = {}
    for name, (a, b) in RC.div_pairs().items():
        a, b = a[::RC.KAT_STRIDE[name]].copy(), b[::RC.KAT_STRIDE[name]].copy()
        q = np.zeros(a.size, np.float32)
        R.ref_div_n(p(a), p(b), a.size, p(q))
        out.update({f"div_a_{name}": a, f"div_b_{name}": b, f"div_q_{name}": q})
    for name, tf in RC.transfer_functions().items():
        t, lo, hi, scale = tf
        v = RC.classify_values(tf, thin=True)
        o = np.zeros((v.size, 4), np.float32)
        R.ref_post_classify_n(p(t), len(t), float(lo), float(hi), float(scale), p(v), v.size, p(o))
        out.update({f"tf_lut_{len(t)}_{int(np.isnan(t).any())}": t, f"tf_range_{name}": np.float32([lo, hi, scale]), f"tf_v_{name}": v,
                    f"tf_out_{name}": o})
    for w in (False, True):
        box, rA, rB = RC.ray_scene(w)
        r = RC.rays(box, rA, rB)
        fl, o = np.zeros(len(r), np.int32), np.zeros((len(r), 6), np.float32)
        R.ref_ray_tests_n(p(r), len(r), p(box), float(rA), float(rB), p(fl), p(o))
        out.update({f"ray_scene_{int(w)}": np.float32(list(box) + [rA, rB]), f"ray_rays_{int(w)}": r,
                    f"ray_flags_{int(w)}": fl.astype(np.int8), f"ray_out_{int(w)}": o})
    for name, cam, W, H, aid in RC.gen_ray_cases():
        d, st = np.zeros((H, W, 3), np.float32), np.zeros((H, W), np.uint32)
        R.ref_generate_ray_n(p(cam), aid, W, H, p(d), p(st))
        step = 1 if W * H <= 256 else 7
        out.update({f"gen_cam_{name}": cam, f"gen_dir_{name}": d.reshape(-1, 3)[::step].copy(),
                    f"gen_state_{name}": st.ravel()[::step].copy()})
    path = os.path.join(HERE, "kats_raymath.npz")
    np.savez_compressed(path, **out)
    n = os.path.getsize(path)
    print(f"kats_raymath.npz: {n} bytes")
    assert n <= 1 << 19, n


if __name__ == "__main__":
    if not O.have_ref():
        sys.exit("oracle/_ref/libiconref.so missing: make -C oracle ref (needs /root/reference)")
    if len(sys.argv) > 1 and sys.argv[1] == "raymath":
        make_raymath_kats()
        sys.exit(0)
    if len(sys.argv) > 1 and sys.argv[1] == "ragged":
        make_ragged_fixture()
        sys.exit(0)
    if len(sys.argv) > 1 and sys.argv[1] == "terrain":
        make_terrain_fixtures()
        sys.exit(0)
    if len(sys.argv) > 1 and sys.argv[1] == "views":
        make_view_fixtures()
        sys.exit(0)
    if len(sys.argv) > 1 and sys.argv[1] == "grid":
        make_grid_fixtures()
        sys.exit(0)
    if len(sys.argv) > 1 and sys.argv[1] == "wedge":
        make_wedge_fixtures()
        sys.exit(0)
    if len(sys.argv) > 1 and sys.argv[1] == "wedge_edges":
        make_wedge_edge_fixture()
        sys.exit(0)
    for name, spec in FRAMES.items():
        make_frame(name, spec)
    make_kats()
    make_grid_fixtures()
    make_wedge_fixtures()
    make_terrain_fixtures()
    make_view_fixtures()
    make_ragged_fixture()
    make_raymath_kats()
