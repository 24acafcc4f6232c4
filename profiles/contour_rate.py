#!/usr/bin/env python3
"""profiles/contour_rate.py -- the time of irt_contour_grid on a 720 x 1440 wrapped grid of the C3
scene's field (R2B07 x 90, irt_create_synth) at one radius, with 1 threshold and with 16, timed with
HIP events on torch's current stream, against three yardsticks taken in the same run:

  sample   irt_sample_latlon of the same single level: the cost of producing the call's input
  copy     the bytes the call cannot avoid -- the value and found grids read (5 B per point), the
           emitted segments written (64 B each) -- at the 6.29 TB/s a float4 copy measures on this
           chip (computed), and a device-to-device copy of half that many bytes (a copy reads and
           writes each byte once), measured
  host     irt_contour_cells on the host for the same input, by the host clock

irt_contour_grid synchronises its stream to return the counts, so an event pair around it times the
call as a user sees it: the three passes, the two small copies and the host's wait between them.  The
count-only form (d_out NULL: two passes) is timed as well.  Before timing, the device's segments are
compared with irt_contour_cells byte for byte.

Five rounds, the runs interleaved in each, --reps calls inside one event pair; per run the median per
call and the range.  Writes the same as JSON (--out)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "icon-ray-tracing_amd", "python"))
import irt  # noqa: E402

F = np.float32
COPY_RATE = 6.29e12  # bytes per second, a float4 copy on the MI355X


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=8, help="calls inside one event pair")
    ap.add_argument("--bisections", type=int, default=7)
    ap.add_argument("--lat", type=int, default=720)
    ap.add_argument("--lon", type=int, default=1440)
    args = ap.parse_args()
    import torch
    dev = "cuda:0"
    ctx = irt.Context.synth(2, args.bisections, 90, 0)
    info = ctx.info
    lo, hi = float(info.sphericalBounds.lower.x), float(info.sphericalBounds.upper.x)
    radius = F(0.5 * (lo + hi))
    nlat, nlon = args.lat, args.lon
    lat = np.linspace(-0.5 * np.pi, 0.5 * np.pi, nlat).astype(F)
    lon = (-np.pi + 2.0 * np.pi * np.arange(nlon) / nlon).astype(F)
    value = torch.empty((nlat, nlon), dtype=torch.float32, device=dev)
    found = torch.empty((nlat, nlon), dtype=torch.uint8, device=dev)
    s = torch.cuda.current_stream(0).cuda_stream
    ctx.sample_latlon(lat, lon, [radius], value.data_ptr(), found.data_ptr(), irt.MODE_USER_GEOM, float("nan"), s)
    torch.cuda.synchronize()
    v, fd = value.cpu().numpy(), found.cpu().numpy()
    q = np.quantile(v[fd == 1].astype(np.float64), np.linspace(0.05, 0.95, 16)).astype(F)
    cases = {"T1": q[7:8], "T16": q}
    res = {"scene": f"R2B0{args.bisections} x 90", "grid": [nlat, nlon], "radius": float(radius), "rounds": args.rounds,
           "reps": args.reps, "found": int(fd.sum()), "cases": {}, "runs": {}}
    outs, runs = {}, {}
    for name, thr in cases.items():
        sty = np.arange(thr.size) % irt.OVERLAY_MAX_STYLES
        t0 = time.perf_counter()
        want, per = irt.contour_cells(v, fd, lat, lon, thr, sty, True, return_counts=True)
        host_ms = (time.perf_counter() - t0) * 1e3 / 2  # (contour_cells makes the count and the fill call)
        n, dper = ctx.contour_grid(value.data_ptr(), found.data_ptr(), lat, lon, thr, sty, 0, 0, True, s)
        out = torch.empty((max(n, 1), 64), dtype=torch.uint8, device=dev)
        ctx.contour_grid(value.data_ptr(), found.data_ptr(), lat, lon, thr, sty, out.data_ptr(), n, True, s)
        torch.cuda.synchronize()
        got = out[:n].cpu().numpy().reshape(-1).view(irt.SEGMENT_DTYPE)
        if n != want.size or dper.tolist() != per.tolist() or got.tobytes() != want.tobytes():
            raise SystemExit(f"{name}: the device's segments differ from irt_contour_cells ({n} vs {want.size})")
        moved = 5 * nlat * nlon + 64 * n
        res["cases"][name] = {"thresholds": thr.tolist(), "segments": int(n), "bytes": moved,
                              "copy_floor_ms": moved / COPY_RATE * 1e3, "host_ms": host_ms}
        print(f"{name}: {n} segments equal irt_contour_cells byte for byte; {moved} bytes, "
              f"{moved / COPY_RATE * 1e6:.2f} us at the copy rate; host {host_ms:.1f} ms")
        outs[name] = out
        src = torch.empty(moved // 2, dtype=torch.uint8, device=dev)
        dst = torch.empty_like(src)

        def full(thr=thr, sty=sty, out=out, n=n):
            ctx.contour_grid(value.data_ptr(), found.data_ptr(), lat, lon, thr, sty, out.data_ptr(), n, True, s)

        def count(thr=thr, sty=sty):
            ctx.contour_grid(value.data_ptr(), found.data_ptr(), lat, lon, thr, sty, 0, 0, True, s)

        runs[f"{name}/grid"] = full
        runs[f"{name}/count-only"] = count
        runs[f"{name}/copy"] = lambda src=src, dst=dst: dst.copy_(src)
    runs["sample"] = lambda: ctx.sample_latlon(lat, lon, [radius], value.data_ptr(), found.data_ptr(),
                                               irt.MODE_USER_GEOM, float("nan"), s)
    for fn in runs.values():  # warm-up
        fn()
    torch.cuda.synchronize()
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
    med = {k: sorted(x)[len(x) // 2] for k, x in ms.items()}
    for name in runs:
        t = sorted(ms[name])
        res["runs"][name] = {"ms": ms[name], "median_ms": med[name], "min_ms": t[0], "max_ms": t[-1],
                             "over_sample": med[name] / med["sample"]}
        print(f"{name:18s} median {med[name]:8.4f} ms  (min {t[0]:.4f} max {t[-1]:.4f})  {med[name] / med['sample']:7.3f} x sample")
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
