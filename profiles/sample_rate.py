#!/usr/bin/env python3
"""profiles/sample_rate.py -- the rates of irt_sample_points / irt_sample_latlon on the C3 scene
(R2B07 x 90, irt_create_synth), timed with HIP events on torch's current stream:

  (a) 2^24 uniformly random points in the shell through irt_sample_points
  (b) the same points sorted by cube-map cell
  (c) a 0.1 degree grid (1800 x 3600) x 8 levels through irt_sample_latlon, 8 x 8 patches per wave
  (d) the (c) grid's points, row-major (64 consecutive points per wave), through irt_sample_points

Five rounds, the runs interleaved in each, --reps calls inside one event pair; per run the median
per call and the spread.  Prints M points/s
and the 128-B lines per point implied by the random-line ceiling of DESIGN.md section 5.4
(48 G lines/s), and writes the same as JSON (--out)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "icon-ray-tracing_amd", "python"))
import irt  # noqa: E402

CEILING_LINES = 48e9


def cubemap_cell(p, G):
    """irt_common.h cubemap_cell of (n, 3) torch points, as a sort key."""
    import torch
    a = p.abs()
    face_axis = torch.where((a[:, 0] >= a[:, 1]) & (a[:, 0] >= a[:, 2]), 0, torch.where(a[:, 1] >= a[:, 2], 1, 2))
    idx = torch.arange(len(p), device=p.device)
    den = a[idx, face_axis]
    face = 2 * face_axis + (p[idx, face_axis] < 0).long()
    u = torch.where(face_axis == 0, p[:, 1], p[:, 0]) / den
    v = torch.where(face_axis == 2, p[:, 1], p[:, 2]) / den
    i = ((u + 1) * 0.5 * G).long().clamp(0, G - 1)
    j = ((v + 1) * 0.5 * G).long().clamp(0, G - 1)
    return (face * G + j) * G + i


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=8, help="calls inside one event pair")
    ap.add_argument("--bisections", type=int, default=7)
    ap.add_argument("--log2-points", type=int, default=24)
    ap.add_argument("--grid", type=int, nargs=3, default=(8, 1800, 3600), metavar=("LEVELS", "LAT", "LON"))
    args = ap.parse_args()
    import torch
    dev = "cuda:0"
    ctx = irt.Context.synth(2, args.bisections, 90, 0)
    lo, hi = float(ctx.info.sphericalBounds.lower.x), float(ctx.info.sphericalBounds.upper.x)
    G = int(ctx.info.locatorFaceRes)
    g = torch.Generator(device=dev).manual_seed(7)
    n = 1 << args.log2_points
    d = torch.randn(n, 3, device=dev, generator=g)
    d /= d.norm(dim=1, keepdim=True)
    pts = (d * (lo + (hi - lo) * torch.rand(n, 1, device=dev, generator=g))).contiguous()
    srt = pts[torch.argsort(cubemap_cell(pts, G))].contiguous()
    L, nlat, nlon = args.grid
    lat = np.deg2rad(-90 + (np.arange(nlat) + 0.5) * (180.0 / nlat)).astype(np.float32)
    lon = np.deg2rad(-180 + (np.arange(nlon) + 0.5) * (360.0 / nlon)).astype(np.float32)
    rad = (lo + (hi - lo) * (np.arange(L) + 0.5) / L).astype(np.float32)
    gpts = torch.from_numpy(irt.latlon_points(lat, lon, rad).reshape(-1, 3)).to(dev)
    m = L * nlat * nlon
    value = torch.empty(max(n, m), dtype=torch.float32, device=dev)
    found = torch.empty(max(n, m), dtype=torch.uint8, device=dev)
    s = torch.cuda.current_stream(0).cuda_stream

    def points(x, count):
        return lambda: ctx.sample_points(x.data_ptr(), count, value.data_ptr(), found.data_ptr(), 0, float("nan"), s)

    def latlon():
        ctx.sample_latlon(lat, lon, rad, value.data_ptr(), found.data_ptr(), 0, float("nan"), s)

    runs = {"a_random": (points(pts, n), n), "b_sorted": (points(srt, n), n),
            "c_latlon_patch": (latlon, m), "d_grid_points": (points(gpts, m), m)}
    answers = {}
    for name, (fn, count) in runs.items():  # warm-up, and the answers
        fn()
        torch.cuda.synchronize()
        answers[name] = (value[:count].clone().view(torch.int32), found[:count].clone())
    assert torch.equal(answers["c_latlon_patch"][0], answers["d_grid_points"][0])
    assert torch.equal(answers["c_latlon_patch"][1], answers["d_grid_points"][1])
    ms = {k: [] for k in runs}
    for _ in range(args.rounds):
        for name, (fn, count) in runs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.reps):
                fn()
            e1.record()
            e1.synchronize()
            ms[name].append(e0.elapsed_time(e1) / args.reps)
    out = {"scene": f"R2B0{args.bisections} x 90", "records": int(ctx.info.numCells), "locatorFaceRes": G,
           "grid": [L, nlat, nlon], "rounds": args.rounds, "reps": args.reps, "ceiling_lines_per_s": CEILING_LINES, "runs": {}}
    for name, (fn, count) in runs.items():
        t = sorted(ms[name])
        med = t[len(t) // 2]
        rate = count / (med * 1e-3)
        out["runs"][name] = {"points": count, "found": int(answers[name][1].sum()), "ms": ms[name], "median_ms": med,
                             "mpoints_per_s": rate / 1e6, "lines_per_point_at_ceiling": CEILING_LINES / rate}
        print(f"{name:16s} {count:9d} points  median {med:8.3f} ms  (min {t[0]:.3f} max {t[-1]:.3f})  "
              f"{rate / 1e6:9.1f} M points/s  {CEILING_LINES / rate:6.2f} lines/point at the ceiling  "
              f"found {out['runs'][name]['found']}")
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
