#!/usr/bin/env python3
"""profiles/hist_rate.py -- the time of irt_histogram on the C3 scene (R2B07 x 90, irt_create_synth),
on the smooth default field and on one with noise = 1 (neighbouring layers and records then fall into
different bins: the LDS-contention question), timed with HIP events on torch's current stream:

  count300      300 bins, counted, no bands
  thick300      300 bins, weighted by thickness, no bands
  bands64x64    64 bands x 64 bins, counted
  *_merge       the same three with IRT_HIST_MERGE=1: the kernel that merges a lane's run of items
                falling into one accumulator before it touches LDS (the product adds every item)
  torch_histc   the path a caller has today for count300: torch.histc over a device tensor of the
                values masked by numLayers (the tensor and the mask resident before the clock starts;
                not bit-comparable -- histc bins in its own arithmetic --, timed only)

Before timing: on a scene small enough for the host (--check-bisections, default R2B04 x 90) every case
against irt_histogram_cells, integer for integer; on C3 every case against the conservation identity
(bins + tails + outside == the sum of the weights, from the host's copy of the records) and count300
against irt_histogram_cells as well.  Five rounds, the runs interleaved in each, --reps calls inside
one event pair (a call is up to three memsets and the kernel); per run the median per call and the
range.  Two yardsticks, neither the code under test: the bytes the kernel must read (per record the
meta word and the 64-B blocks numLayers reaches) at the 6.29 TB/s copy rate, and torch_histc.  Writes
everything as JSON (--out)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "icon-ray-tracing_amd", "python"))
import irt  # noqa: E402

COPY_RATE = 6.29e12  # B/s: the device's measured copy rate


def cases(info_range, lo, hi):
    edges = np.linspace(lo - 10.0, hi + 10.0, 65).astype(np.float32)
    return {"count300": (info_range, 300, "count", None), "thick300": (info_range, 300, "thickness", None),
            "bands64x64": (info_range, 64, "count", edges)}


def run_case(ctx, torch, case):
    vr, bins, w, edges = case
    out = ctx.histogram(vr, bins, w, edges)
    torch.cuda.synchronize()
    return {k: t.cpu().numpy().view(np.uint64) for k, t in out.items()}


def same(a, b):
    return all(np.array_equal(np.asarray(a[k]).reshape(-1), np.asarray(b[k]).reshape(-1)) for k in irt.HISTOGRAM_OUTPUTS)


def weight_sum(cells, weighting):
    nl = cells["numLayers"]
    if weighting == "count":
        return int(nl.sum(dtype=np.int64))
    total = 0
    for a in range(0, cells.size, 1 << 18):  # in slabs: the items of C3 are 122 M
        c = cells[a:a + (1 << 18)]
        valid = np.arange(31)[None, :] < c["numLayers"][:, None]
        d = (c["height"][:, 1:32] - c["height"][:, :31])[valid]
        ok = (d > 0) & (d <= np.float32(1048576.0))
        total += int((np.where(ok, d, np.float32(0)) * np.float32(64.0)).astype(np.uint64).sum(dtype=np.uint64))
    return total


def measure(torch, name, bisections, noise, args, check_cells):
    cells = irt.synth_grid(2, bisections, 90, noise=noise)
    ctx = irt.Context.synth(2, bisections, 90, 0, noise=noise)
    info = ctx.info
    vr = (float(info.dataRange.lower), float(info.dataRange.upper))
    cs = cases(vr, float(info.sphericalBounds.lower.x), float(info.sphericalBounds.upper.x))
    res = {"records": int(info.numCells), "noise": noise, "value_range": vr, "checks": {}, "runs": {}}
    for merge in ("0", "1"):
        os.environ["IRT_HIST_MERGE"] = merge
        for key, case in cs.items():
            got = run_case(ctx, torch, case)
            total = int(got["bins"].sum(dtype=np.uint64)) + int(got["tails"].sum(dtype=np.uint64)) + int(got["outside"][0])
            ok = total == weight_sum(cells, case[2])
            if check_cells or key == "count300":
                ok = ok and same(got, irt.histogram_cells(cells, case[0], case[1], case[2], case[3]))
            res["checks"][key + ("" if merge == "0" else "_merge")] = bool(ok)
    assert all(res["checks"].values()), f"{name}: irt_histogram differs from the definition: {res['checks']}"
    if check_cells:  # the small scene: checked, not timed
        ctx.close()
        return res
    nl = cells["numLayers"].astype(np.int64)
    must = int(np.where(nl > 0, 64 * ((nl >> 3) + 1), 0).sum() + 4 * nl.size)
    res["bytes_must_read"] = must
    res["floor_ms"] = 1e3 * must / COPY_RATE
    d_val = torch.from_numpy(np.ascontiguousarray(cells["value"])).to("cuda:0")
    d_mask = torch.from_numpy(np.arange(32)[None, :] < cells["numLayers"][:, None]).to("cuda:0")
    del cells
    kept = {}

    def torch_histc():
        kept["h"] = torch.histc(d_val[d_mask], bins=300, min=vr[0], max=vr[1])

    def call(key, merge):
        def fn():
            os.environ["IRT_HIST_MERGE"] = merge
            kept[key] = ctx.histogram(*cs[key])
        return fn

    runs = {}
    for key in cs:
        runs[key] = call(key, "0")
        runs[key + "_merge"] = call(key, "1")
    runs["torch_histc"] = torch_histc
    for fn in runs.values():  # warm-up
        fn()
    torch.cuda.synchronize()
    res["torch_histc_items"] = int(kept["h"].sum().item())
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
    os.environ["IRT_HIST_MERGE"] = "0"
    for run in runs:
        t = sorted(ms[run])
        med = t[len(t) // 2]
        res["runs"][run] = {"ms": ms[run], "median_ms": med, "min_ms": t[0], "max_ms": t[-1],
                            "over_floor": med / res["floor_ms"]}
        print(f"{name:7s} {run:20s} median {med:8.4f} ms  (min {t[0]:.4f} max {t[-1]:.4f})  x{med / res['floor_ms']:.2f} floor")
    th = res["runs"]["torch_histc"]["median_ms"]
    for run in runs:
        res["runs"][run]["over_torch_histc"] = res["runs"][run]["median_ms"] / th
    ctx.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10, help="calls inside one event pair")
    ap.add_argument("--bisections", type=int, default=7)
    ap.add_argument("--check-bisections", type=int, default=4)
    args = ap.parse_args()
    import torch
    res = {"scene": f"R2B0{args.bisections} x 90", "rounds": args.rounds, "reps": args.reps, "copy_rate": COPY_RATE,
           "small": {}, "cases": {}}
    for name, noise in (("smooth", 0.0), ("noise1", 1.0)):
        res["small"][name] = measure(torch, name, args.check_bisections, noise, args, True)
        res["cases"][name] = measure(torch, name, args.bisections, noise, args, False)
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
