"""Loading helpers for tests/golden/*.npz (made by tests/golden/make_golden.py)."""
import glob
import os

import numpy as np

import oracle as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FRAME_FIXTURES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "f*.npz")))


def load(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False)
    d = {k: z[k] for k in z.files}
    d["cells"] = np.ascontiguousarray(d["cells"]).view(O.CELL_DTYPE).ravel()
    return d


def load_kats_terrain():
    """kats_terrain.npz: reference known answers on convert_icon-layout records, per grid
    ("l90", "l65"); the records come back as CELL_DTYPE."""
    z = np.load(os.path.join(GOLDEN, "kats_terrain.npz"), allow_pickle=False)
    d = {k: z[k] for k in z.files}
    for tag in ("l90", "l65"):
        d["cells_" + tag] = np.ascontiguousarray(d["cells_" + tag]).view(O.CELL_DTYPE).ravel()
    return d


def terrain_fh_probes(cells):
    """The findHeight probe radii of kats_terrain.npz, a pure function of the stored records
    (the file keeps the answers and a digest of these radii, not the radii): for every record
    with numLayers > 0, every height[j], height[0] - 1, height[numLayers] + 1 and, on records
    with an inverted first layer, the midpoint of height[1]..height[0] -- each with its two
    float neighbours.  Returns (record index int32, radius float32)."""
    idx, hs = [], []
    up, dn = np.float32(np.inf), np.float32(-np.inf)
    for i in range(cells.size):
        nl = int(cells["numLayers"][i])
        if nl <= 0:
            continue
        h = cells["height"][i][:nl + 1].astype(np.float32)
        base = list(h) + [h[0] - np.float32(1), h[nl] + np.float32(1)]
        if h[0] > h[1]:
            base.append(np.float32((np.float64(h[0]) + np.float64(h[1])) * 0.5))
        base = np.array(base, np.float32)
        r = np.concatenate([base, np.nextafter(base, up), np.nextafter(base, dn)])
        hs.append(r)
        idx.append(np.full(r.size, i, np.int32))
    return np.concatenate(idx), np.concatenate(hs).astype(np.float32)


def oracle_scene(d):
    """An OracleScene configured exactly like the fixture (its own LUT and value range)."""
    S = O.OracleScene(d["cells"])
    S.set_transfunc(d["lut"], tuple(d["value_range"]), float(d["opacity_scale"]))
    return S


def params(S, d, accum_id):
    c = d["camera12"]
    return S.params((c[0:3], c[3:6], c[6:9], c[9:12]), accum_id=int(accum_id),
                    raygen=int(d["raygen"]), unit_distance=float(d["unit_distance"]),
                    accel_mode=int(d.get("accel_mode", 0)), mode=int(d.get("mode", 0)))
