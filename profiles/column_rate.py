#!/usr/bin/env python3
"""profiles/column_rate.py -- the time of the column products on the C3 scene (R2B07 x 90,
irt_create_synth), timed with HIP events on torch's current stream:

  one_pass   irt_column_latlon on a 0.25 degree grid (720 x 1440) x the 90 layer mid-radii, all six
             outputs: 24 B written per column
  two_pass   the existing path on the same grid: irt_sample_latlon (90 floats and 90 flag bytes per
             column to HBM), then a torch reduction over the level axis to the same six outputs
             (its two halves are also timed apart: two_pass_sample, two_pass_reduce)
  render_column   irt_render_column at 1024^2 with the framing camera, the weighted sum over the
                  same 90 levels drawn on the mid-shell sphere
  render_levels   irt_render_levels with that one level, as a reference point: one located point
                  per pixel against 90

Before timing, the one-pass outputs are compared, as bits, with irt_column_reduce (host) of the
two-pass values; the torch reduction, whose sum is not sequential, is only timed.  Five rounds, the
runs interleaved in each, --reps calls inside one event pair; per run the median per call and the
range.  Writes the times, the one-pass / two-pass ratio and both paths' output bytes as JSON
(--out)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "icon-ray-tracing_amd", "python"))
import irt  # noqa: E402


def torch_reduce(value, found, weight, miss):
    """The six outputs from (levels, columns) value / found with torch reductions over axis 0."""
    import torch
    f = found != 0
    count = f.sum(0, dtype=torch.int32)
    none = count == 0
    wsum = torch.where(f, value * weight[:, None], 0.0).sum(0)
    vmax, kmax = torch.where(f, value, -torch.inf).max(0)
    vmin, kmin = torch.where(f, value, torch.inf).min(0)
    m = torch.full_like(wsum, miss)
    return {"wsum": torch.where(none, m, wsum), "vmax": torch.where(none, m, vmax), "vmin": torch.where(none, m, vmin),
            "kmax": torch.where(none, -1, kmax).int(), "kmin": torch.where(none, -1, kmin).int(), "count": count}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=4, help="calls inside one event pair")
    ap.add_argument("--bisections", type=int, default=7)
    ap.add_argument("--grid", type=int, nargs=2, default=(720, 1440), metavar=("LAT", "LON"))
    ap.add_argument("--levels", type=int, default=90)
    ap.add_argument("--size", type=int, default=1024)
    args = ap.parse_args()
    import torch
    dev = "cuda:0"
    ctx = irt.Context.synth(2, args.bisections, 90, 0)
    info = ctx.info
    lo, hi = float(info.sphericalBounds.lower.x), float(info.sphericalBounds.upper.x)
    nlat, nlon = args.grid
    L = args.levels
    lat = np.deg2rad(-90 + (np.arange(nlat) + 0.5) * (180.0 / nlat)).astype(np.float32)
    lon = np.deg2rad(-180 + (np.arange(nlon) + 0.5) * (360.0 / nlon)).astype(np.float32)
    rad = (lo + (hi - lo) * (np.arange(L) + 0.5) / L).astype(np.float32)  # the layers are evenly spaced
    weight = np.linspace(0.5, 1.5, L).astype(np.float32)
    cols = nlat * nlon
    miss = -1.0
    value = torch.empty((L, cols), dtype=torch.float32, device=dev)
    found = torch.empty((L, cols), dtype=torch.uint8, device=dev)
    d_weight = torch.from_numpy(weight).to(dev)
    out = {k: torch.empty(cols, dtype=torch.float32 if t is np.float32 else torch.int32, device=dev)
           for k, t in irt.COLUMN_OUTPUTS.items()}
    ptrs = {k: t.data_ptr() for k, t in out.items()}
    s = torch.cuda.current_stream(0).cuda_stream

    W = H = args.size
    setup = irt.setup_frame(None, W, H, camera=irt.FRAMING_CAMERA, info=info)
    ctx.set_transfunc(setup.lut, setup.value_range)
    surface = np.array([0.5 * (lo + hi)], np.float32)
    mean = (weight / weight.sum()).astype(np.float32)  # a weighted mean stays inside the value range
    fb = torch.zeros(W * H, dtype=torch.int32, device=dev)
    accum = torch.zeros(W * H * 4, dtype=torch.float32, device=dev)
    val = torch.empty(W * H, dtype=torch.float32, device=dev)

    def one_pass():
        ctx.column_latlon(lat, lon, rad, ptrs, weight, 0, miss, s)

    def sample():
        ctx.sample_latlon(lat, lon, rad, value.data_ptr(), found.data_ptr(), 0, miss, s)

    kept = {}

    def reduce():
        kept["two"] = torch_reduce(value, found, d_weight, miss)

    def two_pass():
        sample()
        reduce()

    runs = {
        "one_pass": one_pass, "two_pass": two_pass, "two_pass_sample": sample, "two_pass_reduce": reduce,
        "render_column": lambda: ctx.render_column(setup.lp, W, H, float(surface[0]), rad, fb.data_ptr(),
                                                   accum.data_ptr(), val.data_ptr(), mean, irt.COLUMN_WSUM, miss, s),
        "render_levels": lambda: ctx.render_levels(setup.lp, W, H, surface, fb.data_ptr(), accum.data_ptr(),
                                                   val.data_ptr(), 0, False, miss, s),
    }
    for fn in runs.values():  # warm-up
        fn()
    torch.cuda.synchronize()
    # the one-pass result against the definition on the two-pass values, as bits
    want = irt.column_reduce(value.cpu().numpy().reshape(L, nlat, nlon), found.cpu().numpy().reshape(L, nlat, nlon),
                             weight, miss)
    equal = {}
    for k, t in out.items():
        got = t.cpu().numpy().reshape(nlat, nlon)
        equal[k] = bool(np.array_equal(got.view(np.uint32), want[k].view(np.uint32)))
    assert all(equal.values()), f"one-pass outputs differ from irt_column_reduce of the two-pass values: {equal}"
    torch_sum_equal = int((kept["two"]["wsum"].cpu().numpy().view(np.uint32) == want["wsum"].reshape(-1).view(np.uint32)).sum())
    full = int((want["count"] == L).sum())

    ms = {k: [] for k in runs}
    for _ in range(args.rounds):
        for name, fn in runs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.reps):
                fn()
            e1.record()
            e1.synchronize()
            ms[name].append(e0.elapsed_time(e1) / args.reps)
    res = {"scene": f"R2B0{args.bisections} x 90", "records": int(info.numCells), "grid": [L, nlat, nlon],
           "frame": [W, H], "rounds": args.rounds, "reps": args.reps, "columns": cols, "full_columns": full,
           "one_pass_bits_equal_column_reduce_of_two_pass": equal,
           "torch_wsum_bits_equal_sequential": [torch_sum_equal, cols],
           "output_bytes": {"one_pass": 24 * cols, "two_pass": (5 * L + 24) * cols}, "runs": {}}
    for name in runs:
        t = sorted(ms[name])
        med = t[len(t) // 2]
        res["runs"][name] = {"ms": ms[name], "median_ms": med, "min_ms": t[0], "max_ms": t[-1]}
        print(f"{name:16s} median {med:8.3f} ms  (min {t[0]:.3f} max {t[-1]:.3f})")
    r = res["runs"]
    res["one_pass_over_two_pass"] = r["one_pass"]["median_ms"] / r["two_pass"]["median_ms"]
    res["one_pass_over_sample_alone"] = r["one_pass"]["median_ms"] / r["two_pass_sample"]["median_ms"]
    res["render_column_over_render_levels"] = r["render_column"]["median_ms"] / r["render_levels"]["median_ms"]
    res["mpoints_per_s"] = {"one_pass": L * cols / r["one_pass"]["median_ms"] / 1e3,
                            "two_pass_sample": L * cols / r["two_pass_sample"]["median_ms"] / 1e3}
    print(f"one pass / two pass: {res['one_pass_over_two_pass']:.3f}   one pass / irt_sample_latlon alone: "
          f"{res['one_pass_over_sample_alone']:.3f}   render_column / render_levels(1): "
          f"{res['render_column_over_render_levels']:.2f}")
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
