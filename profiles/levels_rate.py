#!/usr/bin/env python3
"""profiles/levels_rate.py -- the rate of irt_render_levels on the C3 scene (R2B07 x 90,
irt_create_synth) at 1024^2 with the framing camera, timed with HIP events on torch's current
stream, against the existing path on the same work: irt_sample_points over the frame's live hit
points, computed and uploaded outside the timed region.

  1 level                    mid-shell
  8 levels                   evenly spaced inside the shell, near hits only
  8 levels, IRT_LEVELS_BACK  ... and the far sides

The hit points of the comparison are those of the pixel centres' rays (jitter 0.5 in both axes),
made with torch in float32 by the expressions of intersectSphere: the same number of points to
locate, in slot order and, within a slot, in pixel order (64 consecutive pixels of a row per wave
instead of the levels kernel's 8 x 8 packet).  The levels call does strictly more per point (the
ray, the hit, the classification, the compositing and the pixel) and reads no xyz stream.

Five rounds, the runs interleaved in each, --reps calls inside one event pair; per run the median
per call and the range.  Prints M located points/s, the 128-B lines per point implied by the
random-line ceiling of DESIGN.md section 5.4 (48 G lines/s) and the ratio of the two rates, and
writes the same as JSON (--out)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "icon-ray-tracing_amd", "python"))
import irt  # noqa: E402

CEILING_LINES = 48e9


def hit_points(lp, W, H, radii, back, dev):
    """The live slots' points of the pixel centres' rays, in slot order: (n, 3) float32."""
    import torch
    c = torch.from_numpy(lp.camera12()).to(dev)
    org, d00, du, dv = c[0:3], c[3:6], c[6:9], c[9:12]
    ys, xs = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float32),
                            torch.arange(W, device=dev, dtype=torch.float32), indexing="ij")
    a, b = (xs + 0.5) + 0.5, (ys + 0.5) + 0.5
    d = d00 + a[..., None] * du + b[..., None] * dv
    d = d / d.norm(dim=-1, keepdim=True)
    d = torch.where(d.abs() < 1e-5, torch.full_like(d, 1e-5), d).reshape(-1, 3)
    A = (d * d).sum(-1)
    B = 2.0 * (d * org).sum(-1)
    near = sorted(range(len(radii)), key=lambda i: (-float(radii[i]), i))
    out = []
    for s in range(2 * len(radii)):
        far = s >= len(radii)
        r = float(radii[near[2 * len(radii) - 1 - s] if far else near[s]])
        C = (org * org).sum() - r * r
        disc = B * B - 4.0 * A * C
        sq = disc.clamp(min=0).sqrt()
        q = torch.where(B < 0, -0.5 * (B - sq), -0.5 * (B + sq))
        t1, t2 = q / A, C / q
        tn, tf = torch.minimum(t1, t2), torch.maximum(t1, t2)
        hit = disc >= 0
        live = hit & (tf > 0) & (torch.tensor(back, device=dev) | ~(tn > 0)) if far else hit & (tn > 0)
        t = tf if far else tn
        out.append((org + d * t[:, None])[live])
    return torch.cat(out).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=8, help="calls inside one event pair")
    ap.add_argument("--bisections", type=int, default=7)
    ap.add_argument("--size", type=int, default=1024)
    args = ap.parse_args()
    import torch
    dev = "cuda:0"
    W = H = args.size
    ctx = irt.Context.synth(2, args.bisections, 90, 0)
    info = ctx.info
    setup = irt.setup_frame(None, W, H, camera=irt.FRAMING_CAMERA, info=info)
    ctx.set_transfunc(setup.lut, setup.value_range)
    lp = setup.lp
    lo, hi = float(info.sphericalBounds.lower.x), float(info.sphericalBounds.upper.x)
    one = np.array([0.5 * (lo + hi)], np.float32)
    eight = (lo + (hi - lo) * (np.arange(8) + 0.5) / 8).astype(np.float32)
    fb = torch.zeros(W * H, dtype=torch.int32, device=dev)
    accum = torch.zeros(W * H * 4, dtype=torch.float32, device=dev)
    val = torch.empty(W * H, dtype=torch.float32, device=dev)
    lev = torch.empty(W * H, dtype=torch.int32, device=dev)
    s = torch.cuda.current_stream(0).cuda_stream
    cases = {"1_level": (one, False), "8_levels": (eight, False), "8_levels_back": (eight, True)}
    runs, counts = {}, {}
    for name, (radii, back) in cases.items():
        pts = hit_points(lp, W, H, radii, back, dev)
        out = torch.empty(len(pts), dtype=torch.float32, device=dev)
        counts[name] = len(pts)
        runs[name + "/levels"] = (lambda radii=radii, back=back: ctx.render_levels(
            lp, W, H, radii, fb.data_ptr(), accum.data_ptr(), val.data_ptr(), lev.data_ptr(), back, float("nan"), s))
        runs[name + "/points"] = (lambda pts=pts, out=out: ctx.sample_points(
            pts.data_ptr(), len(pts), out.data_ptr(), 0, 0, float("nan"), s))
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
    res = {"scene": f"R2B0{args.bisections} x 90", "records": int(info.numCells), "frame": [W, H],
           "rounds": args.rounds, "reps": args.reps, "ceiling_lines_per_s": CEILING_LINES, "runs": {}}
    for name in cases:
        row = {"points": counts[name]}
        for which in ("levels", "points"):
            t = sorted(ms[f"{name}/{which}"])
            med = t[len(t) // 2]
            rate = counts[name] / (med * 1e-3)
            row[which] = {"ms": ms[f"{name}/{which}"], "median_ms": med, "min_ms": t[0], "max_ms": t[-1],
                          "mpoints_per_s": rate / 1e6, "lines_per_point_at_ceiling": CEILING_LINES / rate}
            print(f"{name:14s} {which:7s} {counts[name]:9d} points  median {med:7.3f} ms  (min {t[0]:.3f} max {t[-1]:.3f})"
                  f"  {rate / 1e6:8.1f} M points/s  {CEILING_LINES / rate:6.2f} lines/point at the ceiling")
        row["levels_over_points_rate"] = row["levels"]["mpoints_per_s"] / row["points"]["mpoints_per_s"]
        print(f"{name:14s} levels / points rate: {row['levels_over_points_rate']:.3f}")
        res["runs"][name] = row
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
