#!/usr/bin/env python3
"""profiles/overlay_rate.py -- the rate of irt_render_overlay on the C3 framing view (R2B07 x 90,
irt_create_synth) at 1024^2, timed with HIP events on torch's current stream, in its two kernel
forms -- the per-lane walk (the product) and the wave-uniform walk (IRT_OVERLAY_UNIFORM=1) -- and with the
library's choice of bins (binsPerEdge 0: a mean list near 16) and with 256 bins per edge, against two
yardsticks measured in the same run:

  levels   irt_render_levels with one level on the same frame: a sibling that generates the same
           rays and writes the same pixel bytes, and also locates a point in the scene
  copy     the copy-rate floor of the bytes an overlay call must move per pixel: d_accum_in (16 B
           read), d_cover (16 B read, 16 B written), d_fb and d_segment (4 B written each) -- 56 B,
           as device-to-device copies of 28 B per pixel (a copy reads and writes each byte once)

Cases: a 10 degree graticule at 1 degree arcs; a synthetic coast of 2^17 segments (64 seeded random
walks of 2,048 steps of about 1.5e-3 rad); both together.  Lines are 1.5 pixels wide (overlay_width).
Before timing, d_segment of every case and form is checked against irt_overlay_cover on a strided
subset of the frame's pixels, their unit vectors restated with numpy in float32 for the jittered rays of
that frame (the LCG's two draws per pixel included).

Five rounds, the runs interleaved in each, --reps calls inside one event pair; per run the median
per call and the range.  Writes the same as JSON (--out)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "icon-ray-tracing_amd", "python"))
import irt  # noqa: E402

F = np.float32


def coast(walks=64, steps=2048, step=1.5e-3, seed=5):
    """(lat, lon, first) of `walks` random walks, float32."""
    rng = np.random.default_rng(seed)
    p = rng.normal(size=(walks, 3))
    p /= np.linalg.norm(p, axis=1, keepdims=True)
    head = rng.uniform(0, 2 * np.pi, walks)
    out = np.zeros((steps + 1, walks, 3))
    out[0] = p
    for k in range(steps):
        head += rng.normal(0.0, 0.3, walks)
        ref = np.where(np.abs(p[:, 2:3]) < 0.9, [[0.0, 0.0, 1.0]], [[1.0, 0.0, 0.0]])
        e1 = np.cross(ref, p)
        e1 /= np.linalg.norm(e1, axis=1, keepdims=True)
        e2 = np.cross(p, e1)
        p = p + step * (np.cos(head)[:, None] * e1 + np.sin(head)[:, None] * e2)
        p /= np.linalg.norm(p, axis=1, keepdims=True)
        out[k + 1] = p
    out = out.transpose(1, 0, 2).reshape(-1, 3)
    lat, lon = np.arcsin(out[:, 2]), np.arctan2(out[:, 1], out[:, 0])
    first = np.arange(walks + 1, dtype=np.int32) * (steps + 1)
    return lat.astype(F), lon.astype(F), first


def lcg_jitter(accum_id, W, H):
    """gen_ray's two draws per pixel (irt_common.h lcg_seed / lcg_next / lcg_float) in numpy uint32:
    (jv, ju), each (H, W) float32."""
    ys, xs = np.mgrid[0:H, 0:W].astype(np.uint32)
    v0 = (np.uint32(accum_id) * np.uint32(W) * np.uint32(H) + xs).astype(np.uint32)
    v1 = ys.astype(np.uint32)
    s = np.zeros_like(v0)
    with np.errstate(over="ignore"):
        for _ in range(4):  # lcg_seed: four TEA-like rounds
            s = (s + np.uint32(0x9e3779b9)).astype(np.uint32)
            v0 = (v0 + ((((v1 << np.uint32(4)) + np.uint32(0xa341316c)) ^ (v1 + s) ^ ((v1 >> np.uint32(5)) + np.uint32(0xc8013ea4))))).astype(np.uint32)
            v1 = (v1 + ((((v0 << np.uint32(4)) + np.uint32(0xad90777d)) ^ (v0 + s) ^ ((v0 >> np.uint32(5)) + np.uint32(0x7e95761e))))).astype(np.uint32)
        st = v0
        st = (np.uint32(1664525) * st + np.uint32(1013904223)).astype(np.uint32)
        jv = (st & np.uint32(0x00FFFFFF)).astype(F) / F(0x01000000)
        st = (np.uint32(1664525) * st + np.uint32(1013904223)).astype(np.uint32)
        ju = (st & np.uint32(0x00FFFFFF)).astype(F) / F(0x01000000)
    return jv, ju


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=8, help="calls inside one event pair")
    ap.add_argument("--bisections", type=int, default=7)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--stride", type=int, default=37, help="the checked subset: every stride-th pixel")
    args = ap.parse_args()
    import torch
    dev = "cuda:0"
    W = H = args.size
    ctx = irt.Context.synth(2, args.bisections, 90, 0)
    info = ctx.info
    setup = irt.setup_frame(None, W, H, camera=irt.FRAMING_CAMERA, info=info)
    ctx.set_transfunc(setup.lut, setup.value_range)
    lp = setup.lp
    R = float(info.sphericalBounds.lower.x)
    w = irt.overlay_width(lp, H, R, 1.5)
    styles = [((1.0, 1.0, 1.0, 1.0), w), ((0.1, 0.1, 0.1, 0.7), 2 * w)]
    deg = np.pi / 180
    grat = irt.graticule(10 * deg, 10 * deg, 1 * deg, 1)
    lat, lon, first = coast()
    shore = irt.overlay_segments(lat, lon, first, 0.2, 0)
    sets = {"graticule": grat, "coast": shore, "both": np.concatenate([shore, grat])}
    fb = torch.zeros(W * H, dtype=torch.int32, device=dev)
    accum = torch.zeros(W * H * 4, dtype=torch.float32, device=dev)
    cover = torch.zeros(W * H * 4, dtype=torch.float32, device=dev)
    segm = torch.empty(W * H, dtype=torch.int32, device=dev)
    s = torch.cuda.current_stream(0).cuda_stream
    ctx.render(lp, W, H, fb.data_ptr(), accum.data_ptr(), s)  # a frame's accum for the composite
    torch.cuda.synchronize()

    # the checked pixels' unit vectors, restated in float32 (the test suite pins every pixel of small frames)
    cam = lp.camera12()
    org, d00, du, dv = cam[0:3], cam[3:6], cam[6:9], cam[9:12]
    jv, ju = lcg_jitter(lp.accumID, W, H)
    ys, xs = np.mgrid[0:H, 0:W]
    a, b = (xs.astype(F) + F(0.5)) + ju, (ys.astype(F) + F(0.5)) + jv
    d = np.stack([(d00[k] + a * du[k]) + b * dv[k] for k in range(3)], -1).astype(F)
    d = d / np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])[..., None]
    d = np.where(np.abs(d) < F(1e-5), F(1e-5), d).reshape(-1, 3)[::args.stride]
    A = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    B = ((d[:, 0] * org[0] + d[:, 1] * org[1]) + d[:, 2] * org[2]) * F(2)
    Cc = ((org[0] * org[0] + org[1] * org[1]) + org[2] * org[2]) - F(R) * F(R)
    disc = B * B - F(4) * A * Cc
    hit = disc >= 0
    sq = np.sqrt(np.where(hit, disc, 0)).astype(F)
    q = np.where(B < 0, F(-0.5) * (B - sq), F(-0.5) * (B + sq)).astype(F)
    with np.errstate(divide="ignore", invalid="ignore"):
        t1, t2 = q / A, Cc / q
    tn, tf = np.minimum(t1, t2), np.maximum(t1, t2)
    live = hit & ((tn > 0) | (tf > 0))
    t = np.where(tn > 0, tn, tf).astype(F)
    P = (org[None] + d * t[:, None]).astype(F)
    with np.errstate(divide="ignore", invalid="ignore"):
        u = (P / np.sqrt((P[:, 0] * P[:, 0] + P[:, 1] * P[:, 1]) + P[:, 2] * P[:, 2])[:, None]).astype(F)

    ovs, checked = {}, {}
    for name, seg in sets.items():
        want = np.full(len(u), -1, np.int32)
        tables = {N: irt.overlay_bins(seg, 2 * w, N) for N in (64, 256)}
        want[live] = irt.overlay_cover(seg, styles, u[live], tables[64], 64)
        checked[name] = {"pixels": int(len(u)), "on_a_line": int((want >= 0).sum())}
        for N, (start, _) in tables.items():  # how long the lists are
            ln = np.diff(start.astype(np.int64))
            checked[name][f"entries_N{N}"] = int(start[-1])
            checked[name][f"mean_list_per_bin_N{N}"] = float(ln.mean())
            checked[name][f"mean_list_per_used_bin_N{N}"] = float(ln[ln > 0].mean())
        for bins in (0, 256):
            ovs[name, bins] = ctx.overlay(seg, styles, bins)
            if bins == 0:  # the library's choice, and how long its lists are
                N, entries = ovs[name, bins].bins()
                ln = np.diff(irt.overlay_bins(seg, 2 * w, N)[0].astype(np.int64))
                assert int(ln.sum()) == entries
                checked[name].update({"auto_bins_per_edge": N, "entries_auto": entries, "mean_list_per_bin_auto": float(ln.mean()),
                                      "mean_list_per_used_bin_auto": float(ln[ln > 0].mean()), "longest_list_auto": int(ln.max())})
            for uniform in ("0", "1"):
                os.environ["IRT_OVERLAY_UNIFORM"] = uniform
                segm.fill_(-9)
                ctx.render_overlay(ovs[name, bins], lp, W, H, R, cover.data_ptr(), fb.data_ptr(), accum.data_ptr(),
                                   segm.data_ptr(), False, s)
                torch.cuda.synchronize()
                got = segm.cpu().numpy()[::args.stride]
                bad = int((got != want).sum())
                if bad:
                    raise SystemExit(f"{name} (bins {bins}, uniform={uniform}): d_segment differs from irt_overlay_cover "
                                     f"at {bad} of {len(u)} pixels")
        print(f"{name}: {seg.size} segments, d_segment equals irt_overlay_cover at {len(u)} pixels "
              f"({checked[name]['on_a_line']} on a line), both forms, both bin counts; the library chose N = "
              f"{checked[name]['auto_bins_per_edge']} ({checked[name]['mean_list_per_used_bin_auto']:.1f} entries per used bin); list entries per used bin "
              f"{checked[name]['mean_list_per_used_bin_N64']:.1f} at N = 64, {checked[name]['mean_list_per_used_bin_N256']:.1f} at N = 256")

    lo, hi = float(info.sphericalBounds.lower.x), float(info.sphericalBounds.upper.x)
    one = np.array([0.5 * (lo + hi)], F)
    lfb, lacc = torch.zeros_like(fb), torch.zeros_like(accum)
    src, dst = torch.empty(W * H * 28, dtype=torch.uint8, device=dev), torch.empty(W * H * 28, dtype=torch.uint8, device=dev)

    def overlay_run(name, bins, uniform):
        def fn():
            os.environ["IRT_OVERLAY_UNIFORM"] = uniform
            ctx.render_overlay(ovs[name, bins], lp, W, H, R, cover.data_ptr(), fb.data_ptr(), accum.data_ptr(),
                               segm.data_ptr(), False, s)
        return fn

    runs = {}
    for name in sets:
        for bins in (0, 256):
            runs[f"{name}/N{bins or 'auto'}/lanes"] = overlay_run(name, bins, "0")
            runs[f"{name}/N{bins or 'auto'}/uniform"] = overlay_run(name, bins, "1")
    runs["levels"] = lambda: ctx.render_levels(lp, W, H, one, lfb.data_ptr(), lacc.data_ptr(), 0, 0, False, float("nan"), s)
    runs["copy"] = lambda: dst.copy_(src)
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
    os.environ.pop("IRT_OVERLAY_UNIFORM", None)
    med = {k: sorted(v)[len(v) // 2] for k, v in ms.items()}
    res = {"scene": f"R2B0{args.bisections} x 90", "frame": [W, H], "rounds": args.rounds, "reps": args.reps,
           "half_width_rad": w, "bytes_per_pixel": 56, "checked": checked,
           "segments": {k: int(v.size) for k, v in sets.items()}, "runs": {}}
    for name in runs:
        t = sorted(ms[name])
        res["runs"][name] = {"ms": ms[name], "median_ms": med[name], "min_ms": t[0], "max_ms": t[-1],
                             "over_levels": med[name] / med["levels"], "over_copy": med[name] / med["copy"]}
        print(f"{name:26s} median {med[name]:7.4f} ms  (min {t[0]:.4f} max {t[-1]:.4f})  "
              f"{med[name] / med['levels']:6.3f} x levels  {med[name] / med['copy']:6.2f} x copy")
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    for ov in ovs.values():
        ov.close()
    ctx.close()


if __name__ == "__main__":
    main()
