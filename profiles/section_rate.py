#!/usr/bin/env python3
"""profiles/section_rate.py -- the time of irt_section on the C3 scene (R2B07 x 90,
irt_create_synth) on the 90 layer mid-radii, for a great-circle track of 4,096 columns and for 2^20
random stations, against the existing path; timed with HIP events on torch's current stream:

  section         irt_section with every output: value, found, rgba and the six column outputs
  section_values  irt_section with value and found alone (what irt_sample_points writes)
  section_columns irt_section with the six column outputs alone (24 B per column)
  points          the existing path: irt_sample_points on irt_section_points' output, uploaded before
                  the clock starts (12 B per point read from HBM)
  points_torch    that path plus, in torch, a classification of the values to RGBA8 through the
                  transfer function's table and the reduction over the level axis to the six outputs

Before timing, irt_section's value and found are compared, as bits, with irt_sample_points' and its
column outputs with irt_column_reduce (host) of them; the torch classification and reduction, which
are not bit-exact restatements, are only timed.  Five rounds, the runs interleaved in each, --reps
calls inside one event pair; per run the median per call and the range.  irt_section makes its trig
table on the host (cosf and sinf of every lat and lon, per call): the host time of one call is
measured too (section_host_ms, wall clock around the call alone), since at 2^20 columns it, not the
kernel, is what back-to-back calls wait for; and so is the device side alone (section_device_ms: one
call queued behind a backlog of irt_sample_points calls long enough to hide its host side, the
event pair around that call: its table upload and its kernel).  Writes everything as JSON (--out)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "icon-ray-tracing_amd", "python"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import irt  # noqa: E402
from column_rate import torch_reduce  # noqa: E402


def torch_classify(value, found, lut, lo, hi, amb, radiance):
    """RGBA8 of (levels, columns) values through the table, as postClassify and the pixel write do it
    (not their bits: torch's pow in place of the thresholds)."""
    import torch
    n = lut.shape[0]
    x = (value - lo) / (hi - lo) * n
    i = torch.floor(x)
    frac = (x - i)[..., None]
    i1 = i.long().clamp(0, n - 1)
    i2 = (i.long() + 1).clamp(0, n - 1)
    s = lut[i1] * frac + lut[i2] * (1 - frac)
    a = s[..., 3:4].clamp(0, 1)
    c = a * (s[..., :3] * amb * radiance)
    srgb = torch.where(c <= 0.0031308, 12.92 * c, 1.055 * c.clamp_min(1e-12).pow(1 / 2.4) - 0.055)
    px = (torch.cat([srgb, a], -1) * 256).clamp(0, 255).to(torch.uint8)
    return torch.where((found != 0)[..., None], px, torch.zeros_like(px))


def measure(ctx, torch, name, lat, lon, rad, weight, tf, args):
    dev = "cuda:0"
    L, n = rad.size, lat.size
    miss = -1.0
    amb, radiance = (0.9, 0.8, 0.7), 1.25
    s = torch.cuda.current_stream(0).cuda_stream
    xyz = torch.from_numpy(irt.section_points(lat, lon, rad).reshape(-1, 3)).to(dev)
    mk = lambda shape, dt: torch.empty(shape, dtype=dt, device=dev)  # noqa: E731
    sec = {"value": mk((L, n), torch.float32), "found": mk((L, n), torch.uint8), "rgba": mk((L, n), torch.int32)}
    sec.update({k: mk((n,), torch.float32 if t is np.float32 else torch.int32) for k, t in irt.COLUMN_OUTPUTS.items()})
    pv, pf = mk((L, n), torch.float32), mk((L, n), torch.uint8)
    d_weight = torch.from_numpy(weight).to(dev)
    d_lut = torch.from_numpy(np.ascontiguousarray(tf[0], np.float32)).to(dev)
    d_amb = torch.tensor(amb, dtype=torch.float32, device=dev)
    ptr = lambda ks: {k: sec[k].data_ptr() for k in ks}  # noqa: E731
    every, vals, cols = ptr(sec), ptr(("value", "found")), ptr(irt.COLUMN_OUTPUTS)

    def call(out):
        ctx.section_raw(lat, lon, rad, out, weight, amb, radiance, 0, miss, s)

    def points():
        ctx.sample_points(xyz.data_ptr(), L * n, pv.data_ptr(), pf.data_ptr(), 0, miss, s)

    kept = {}

    def points_torch():
        points()
        kept["rgba"] = torch_classify(pv, pf, d_lut, tf[1][0], tf[1][1], d_amb, radiance)
        kept["col"] = torch_reduce(pv, pf, d_weight, miss)

    runs = {"section": lambda: call(every), "section_values": lambda: call(vals),
            "section_columns": lambda: call(cols), "points": points, "points_torch": points_torch}
    for fn in runs.values():  # warm-up
        fn()
    torch.cuda.synchronize()
    # bit equality before timing: value / found with irt_sample_points', the columns with the host reduction
    equal = {"value": bool(torch.equal(sec["value"].view(torch.int32), pv.view(torch.int32))),
             "found": bool(torch.equal(sec["found"], pf))}
    want = irt.column_reduce(pv.cpu().numpy(), pf.cpu().numpy(), weight, miss)
    for k in irt.COLUMN_OUTPUTS:
        equal[k] = bool(np.array_equal(sec[k].cpu().numpy().view(np.uint32), want[k].view(np.uint32)))
    assert all(equal.values()), f"{name}: irt_section differs from the existing path: {equal}"
    found_points = int(pf.sum().item())
    close = int(((kept["rgba"].view(torch.int32).reshape(L, n) == sec["rgba"])).sum().item())

    ms = {k: [] for k in runs}
    for _ in range(args.rounds):
        for run, fn in runs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.reps):
                fn()
            e1.record()
            e1.synchronize()
            ms[run].append(e0.elapsed_time(e1) / args.reps)
    host = []
    for _ in range(args.rounds):  # the host side of one call, the device idle before and after
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call(every)
        host.append(1e3 * (time.perf_counter() - t0))
        torch.cuda.synchronize()
    device = {k: [] for k in ("section", "section_values", "section_columns")}
    backlog = max(2, int(np.ceil(3.0 * sorted(host)[len(host) // 2] / max(sorted(ms["points"])[0], 1e-3))))
    for _ in range(args.rounds):  # the device side of one call: queued while the device is still busy
        for run in device:
            torch.cuda.synchronize()
            for _ in range(min(backlog, 64)):
                points()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            runs[run]()
            e1.record()
            e1.synchronize()
            device[run].append(e0.elapsed_time(e1))
    res = {"columns": n, "levels": L, "points": L * n, "found_points": found_points,
           "section_device_ms": {k: {"ms": v, "median_ms": sorted(v)[len(v) // 2]} for k, v in device.items()},
           "backlog_calls": min(backlog, 64),
           "bits_equal_existing_path": equal, "torch_rgba_words_equal": [close, L * n],
           "output_bytes": {"section": (9 * L + 24) * n, "section_values": 5 * L * n, "section_columns": 24 * n,
                            "points": 5 * L * n},
           "input_bytes": {"section": 16 * n + 8 * L, "points": 12 * L * n},
           "section_host_ms": {"ms": host, "median_ms": sorted(host)[len(host) // 2]}, "runs": {}}
    for run in runs:
        t = sorted(ms[run])
        med = t[len(t) // 2]
        res["runs"][run] = {"ms": ms[run], "median_ms": med, "min_ms": t[0], "max_ms": t[-1]}
        print(f"{name:9s} {run:16s} median {med:9.3f} ms  (min {t[0]:.3f} max {t[-1]:.3f})")
    r = res["runs"]
    res["section_over_points_torch"] = r["section"]["median_ms"] / r["points_torch"]["median_ms"]
    res["section_values_over_points"] = r["section_values"]["median_ms"] / r["points"]["median_ms"]
    for k, v in res["section_device_ms"].items():
        print(f"{name:9s} {k:16s} device side alone {v['median_ms']:9.3f} ms")
    print(f"{name:9s} host side of one call {res['section_host_ms']['median_ms']:.3f} ms;  section / points+torch "
          f"{res['section_over_points_torch']:.3f};  section (value, found) / points {res['section_values_over_points']:.3f}")
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=4, help="calls inside one event pair")
    ap.add_argument("--bisections", type=int, default=7)
    ap.add_argument("--levels", type=int, default=90)
    ap.add_argument("--track", type=int, default=4096)
    ap.add_argument("--stations", type=int, default=1 << 20)
    args = ap.parse_args()
    import torch
    ctx = irt.Context.synth(2, args.bisections, 90, 0)
    info = ctx.info
    lo, hi = float(info.sphericalBounds.lower.x), float(info.sphericalBounds.upper.x)
    L = args.levels
    rad = (lo + (hi - lo) * (np.arange(L) + 0.5) / L).astype(np.float32)  # the layers are evenly spaced
    weight = np.linspace(0.5, 1.5, L).astype(np.float32)
    setup = irt.setup_frame(None, 64, 64, camera=irt.FRAMING_CAMERA, info=info)
    ctx.set_transfunc(setup.lut, setup.value_range)
    tf = (setup.lut, (float(setup.value_range[0]), float(setup.value_range[1])))
    res = {"scene": f"R2B0{args.bisections} x 90", "records": int(info.numCells), "rounds": args.rounds,
           "reps": args.reps, "cases": {}}
    lat, lon, arc = irt.great_circle(np.radians(52.0), np.radians(-10.0), np.radians(-33.0), np.radians(151.0), args.track)
    res["track_arc_rad"] = arc
    res["cases"]["track"] = measure(ctx, torch, "track", lat, lon, rad, weight, tf, args)
    rng = np.random.default_rng(20)
    lat = np.arcsin(rng.uniform(-1, 1, args.stations)).astype(np.float32)
    lon = rng.uniform(-np.pi, np.pi, args.stations).astype(np.float32)
    res["cases"]["stations"] = measure(ctx, torch, "stations", lat, lon, rad, weight, tf, args)
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
