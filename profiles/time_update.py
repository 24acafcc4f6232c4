#!/usr/bin/env python3
"""Time a value update (irt_update_values* + irt_update_values_end) against re-creating the
context, the only way to advance a time series without it.

One process, one warm context of the scene (default C3: Context.synth(2, 7, 90)):
  (a) irt_update_values_device of all records from a torch tensor + irt_update_values_end
  (b) irt_update_values of all records from a (pageable) numpy array + irt_update_values_end
  (c) irt_create_synth of the same scene (+ irt_set_transfunc, which the update's commit includes)
each the median of --reps runs of a host clock around work that ends synchronised; (a) also split
into the scatter (HIP events on its stream) and the commit.  The kernels' own times come from a
`rocprofv3 --kernel-trace --stats` run of `--what device` (profiles/time_update.sh).

Prints one JSON line; fails without a GPU.  The algorithmic bytes per record kept here:
  k_value_scatter  128 B read + 128 B written (the value halves of the record's block)
  k_shell_rebuild  256 B block + 4 B meta + 8 B rectangle read; its stores are the min/max CAS
                   loops into the 8-MB shell
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "icon-ray-tracing_amd", "python"))

import numpy as np  # noqa: E402

STREAM_TBS = 6.29  # MI355X streaming rate the micro-architecture guide measures, TB/s
SCATTER_BYTES, REBUILD_BYTES = 256, 268


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", type=int, nargs=3, default=(2, 7, 90), metavar=("ROOT", "BISECTIONS", "LEVELS"))
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--what", choices=("all", "device", "host", "create"), default="all")
    ap.add_argument("--out", default=None, help="also append the JSON line to this file")
    a = ap.parse_args()
    import torch

    import irt
    if not torch.cuda.is_available():
        raise SystemExit("time_update.py: no GPU")
    t0 = time.perf_counter()
    ctx = irt.Context.synth(*a.scene)
    create0 = time.perf_counter() - t0
    n = int(ctx.info.numCells)
    lut, vr = irt.default_transfunc((ctx.info.dataRange.lower, ctx.info.dataRange.upper))
    ctx.set_transfunc(lut, vr)
    res = {"scene": list(a.scene), "records": n, "reps": a.reps, "first_create_s": round(create0, 4)}
    g = torch.Generator(device="cuda").manual_seed(1)
    dev = [torch.rand((n, 32), generator=g, device="cuda", dtype=torch.float32) for _ in range(2)]
    torch.cuda.synchronize()
    stream = torch.cuda.current_stream().cuda_stream

    def med(xs):
        return round(statistics.median(xs) * 1e3, 4)

    if a.what in ("all", "device"):
        tot, sc, end = [], [], []
        for k in range(a.reps + 2):  # two warm-up steps
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record()
            ctx.update_values_device(dev[k & 1].data_ptr(), n, 0, stream)
            e1.record()
            t1 = time.perf_counter()
            ctx.end_update()
            t2 = time.perf_counter()
            torch.cuda.synchronize()
            if k >= 2:
                tot.append(t2 - t0), sc.append(e0.elapsed_time(e1) * 1e-3), end.append(t2 - t1)
        res["a_device_ms"], res["a_scatter_ms"], res["a_commit_ms"] = med(tot), med(sc), med(end)
        res["a_scatter_fraction_of_stream"] = round(n * SCATTER_BYTES / (statistics.median(sc) * STREAM_TBS * 1e12), 4)
    if a.what in ("all", "host"):
        host = [d.cpu().numpy() for d in dev]
        tot = []
        for k in range(a.reps + 2):
            t0 = time.perf_counter()
            ctx.update_values(host[k & 1])
            ctx.end_update()
            t1 = time.perf_counter()
            if k >= 2:
                tot.append(t1 - t0)
        res["b_host_ms"] = med(tot)
    if a.what in ("all", "create"):
        tot = []
        for k in range(a.reps):
            t0 = time.perf_counter()
            c2 = irt.Context.synth(*a.scene)
            c2.set_transfunc(lut, vr)
            t1 = time.perf_counter()
            c2.close()
            tot.append(t1 - t0)
        res["c_create_ms"] = med(tot)
    if a.what == "all":
        res["create_over_device_update"] = round(res["c_create_ms"] / res["a_device_ms"], 2)
        res["create_over_host_update"] = round(res["c_create_ms"] / res["b_host_ms"], 2)
        res["update_faster_than_create"] = res["a_device_ms"] < res["c_create_ms"] and res["b_host_ms"] < res["c_create_ms"]
    ctx.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")
    if a.what == "all" and not res["update_faster_than_create"]:
        raise SystemExit("time_update.py: an update is not faster than re-creation")


if __name__ == "__main__":
    main()
