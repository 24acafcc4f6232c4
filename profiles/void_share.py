#!/usr/bin/env python3
"""The share of a chained launch's workgroup lifetime spent in void packets: 8x8 packets all of
whose rays, for every jitter, hit the world box and miss the shell's outer sphere (colour zero).

    python profiles/void_share.py [--config c3] [--batch 8] [--launches 3] [--warmup 5]

Workgroup start/end stamps as profiles/wg_trace.py takes them (one-wave workgroups: one packet
each).  The packets are classified here in float64 with no margin (centre direction and largest
corner angle against the sphere's angular radius), so the figure does not depend on the library's
own classifier and can be taken on a build without one.  One JSON line per launch.

A launch that runs the void-packet work-item list (Context.last_workgroups differs from the plain
grid's count) has rows of Lp live and Vr void items instead: its workgroups are decoded through
irt.void_lists -- workgroup x of row y is live item x, or void item x - Lp of row y; an empty item
renders nothing -- and the void workgroups are the library's own classification.  Each void packet then
has one workgroup per launch, in whichever row carries it, so the figure "frames after the first" is
the void items' lifetime in rows 1 .. B - 1, and the padding's lifetime is reported beside it.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "icon-ray-tracing_amd", "python"), ROOT]

import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
import irt  # noqa: E402


def void_packets_f64(cam12, W, H, radius):
    """bool[tilesY*tilesX*64] in launch order (whole frame): block = 16 tile + sub, packet = 4
    block + wave (irt_raygen.h pixel_of); True: every direction of the packet's active pixels,
    jitter included, misses the sphere of `radius` about the origin."""
    c = np.asarray(cam12, dtype=np.float64)
    org, d00, du, dv = c[0:3], c[3:6], c[6:9], c[9:12]
    tx, ty = (W + 63) // 64, (H + 63) // 64
    p = np.arange(tx * ty * 64)
    blk, wave = p >> 2, p & 3
    k, sub = blk >> 4, blk & 15
    x0 = (k % tx) * 64 + ((sub & 3) << 4) + ((wave & 1) << 3)
    y0 = (k // tx) * 64 + ((sub >> 2) << 4) + ((wave >> 1) << 3)
    x1 = np.minimum(x0 + 8, W)  # one past the last active pixel
    y1 = np.minimum(y0 + 8, H)
    active = (x0 < W) & (y0 < H)

    def unit(a, b):
        d = d00[None, :] + a[:, None] * du[None, :] + b[:, None] * dv[None, :]
        return d / np.linalg.norm(d, axis=1, keepdims=True)

    alo, ahi, blo, bhi = x0 + .5, x1 + .5, y0 + .5, y1 + .5
    cen = unit((alo + ahi) / 2, (blo + bhi) / 2)
    ext = np.zeros(len(p))
    for a, b in ((alo, blo), (ahi, blo), (alo, bhi), (ahi, bhi)):
        ext = np.maximum(ext, np.arccos(np.clip((cen * unit(a, b)).sum(1), -1, 1)))
    dist = np.linalg.norm(org)
    if dist <= radius:
        return np.zeros(len(p), dtype=bool)
    to_centre = np.arccos(np.clip((cen * (-org / dist)[None, :]).sum(1), -1, 1))
    return active & (to_centre - ext > np.arcsin(radius / dist))


def report_list_launches(args, ctx, lp, W, H, B, bufs, last, void64):
    """The launches ran rows of work items (see the head): `last` workgroups each."""
    live, rows = irt.void_lists(lp, ctx.info, W, H, B)
    Lp, Vr = live.size, rows.shape[1]
    assert last == B * (Lp + Vr), (last, B, Lp, Vr)
    item = np.concatenate([np.broadcast_to(live, (B, Lp)), rows], axis=1).reshape(-1)  # workgroup y (Lp + Vr) + x
    is_void_part = np.tile(np.arange(Lp + Vr) >= Lp, B)
    empty = item == 0xFFFFFFFF
    wg_void = is_void_part & ~empty
    frame = np.repeat(np.arange(B), Lp + Vr)
    nvoid = int(np.unique(item[wg_void]).size)
    for k in range(args.launches):
        tr = bufs[k].cpu().numpy().view(np.uint32).reshape(-1, 4)[:last]
        dur = ((tr[:, 1].astype(np.int64) - tr[:, 0].astype(np.int64)) & 0xFFFFFFFF) / 100.0  # us
        span = ((tr[:, 1].astype(np.int64) - tr[:, 0].astype(np.int64).min()) & 0xFFFFFFFF).max() / 100.0
        out = {"config": args.config, "launch": k, "frames_per_launch": B, "workgroups": int(last),
               "plain_grid_workgroups": int(irt.num_tiles(W, H) * 64 * B), "live_items_per_row": int(Lp),
               "void_items_per_row": int(Vr), "empty_items": int(empty.sum()),
               "void_packets_per_frame": nvoid, "void_packets_f64": int(void64.sum()),
               "packets_per_frame": int(irt.num_tiles(W, H) * 64),
               "void_lifetime_share": round(float(dur[wg_void].sum() / dur.sum()), 4),
               "void_lifetime_share_frames_after_first": round(float(dur[wg_void & (frame > 0)].sum() / dur.sum()), 4),
               "empty_item_lifetime_share": round(float(dur[empty].sum() / dur.sum()), 4),
               "wg_us_mean_void": round(float(dur[wg_void].mean()), 3),
               "wg_us_mean_empty": round(float(dur[empty].mean()), 3) if empty.any() else None,
               "wg_us_mean_other": round(float(dur[~is_void_part & ~empty].mean()), 3),
               "span_us": float(span)}
        print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c3")
    ap.add_argument("--launches", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=8)
    args = ap.parse_args()
    rn, bis, L, W, H, tf, orbit_cfg, desc = bench.CONFIGS[args.config]
    assert not orbit_cfg, "progressive configs only"
    dev = torch.device("cuda:0")
    ctx = irt.Context.synth(rn, bis, L, 0, terrain=bench.TERRAIN.get(args.config, 0.0))
    setup = irt.setup_frame(None, W, H, camera=bench.FRAMING, info=ctx.info)
    ctx.set_transfunc(bench.make_lut(tf, setup.lut), setup.value_range)
    ctx.set_statistics(False)
    lp = setup.lp
    fb = torch.zeros(W * H, dtype=torch.int32, device=dev)
    accum = torch.zeros(W * H * 4, dtype=torch.float32, device=dev)
    stream = torch.cuda.current_stream(0).cuda_stream
    ctx.clear(fb.data_ptr(), accum.data_ptr(), W * H, stream)
    B = args.batch

    def step(s):
        lp.accumID = s * B
        ctx.render_accumulate(lp, W, H, B, fb.data_ptr(), accum.data_ptr(), stream)

    for s in range(args.warmup):
        step(s)
    nt = irt.num_tiles(W, H)
    nwg = ctx.launch_workgroups(nt, B)
    assert nwg == nt * 64 * B, "one-wave workgroups, no split items"
    bufs = [torch.zeros(nwg * 4, dtype=torch.int32, device=dev) for _ in range(args.launches)]
    torch.cuda.synchronize()
    for k in range(args.launches):
        ctx.set_wg_trace(bufs[k].data_ptr())
        step(args.warmup + k)
    ctx.set_wg_trace(0)
    torch.cuda.synchronize()
    last = ctx.last_workgroups() if hasattr(irt.lib(), "irt_debug_last_workgroups") else nwg
    void = void_packets_f64(lp.camera12(), W, H, ctx.info.sphericalBounds.upper.x)
    if last != nwg:
        report_list_launches(args, ctx, lp, W, H, B, bufs, last, void)
        ctx.close()
        return
    # workgroup bx of a frame renders wave (bx >> 3) & 3 of block ((bx >> 5) << 3) | (bx & 7) (k_render)
    bx = np.arange(nt * 64)
    pkt = ((((bx >> 5) << 3) | (bx & 7)) << 2) | ((bx >> 3) & 3)
    wg_void = np.tile(void[pkt], B)
    frame = np.repeat(np.arange(B), nt * 64)
    for k in range(args.launches):
        tr = bufs[k].cpu().numpy().view(np.uint32).reshape(-1, 4)
        dur = ((tr[:, 1].astype(np.int64) - tr[:, 0].astype(np.int64)) & 0xFFFFFFFF) / 100.0  # us
        span = ((tr[:, 1].astype(np.int64) - tr[:, 0].astype(np.int64).min()) & 0xFFFFFFFF).max() / 100.0
        out = {"config": args.config, "launch": k, "frames_per_launch": B, "workgroups": int(nwg),
               "void_packets_per_frame": int(void.sum()), "packets_per_frame": int(nt * 64),
               "void_packet_share": round(float(void.mean()), 4),
               "void_lifetime_share": round(float(dur[wg_void].sum() / dur.sum()), 4),
               "void_lifetime_share_frames_after_first": round(float(dur[wg_void & (frame > 0)].sum() / dur.sum()), 4),
               "wg_us_mean_void_first_frame": round(float(dur[wg_void & (frame == 0)].mean()), 3) if void.any() else None,
               "wg_us_mean_void_later_frames": round(float(dur[wg_void & (frame > 0)].mean()), 3) if void.any() else None,
               "wg_us_mean_other": round(float(dur[~wg_void].mean()), 3),
               "span_us": float(span)}
        print(json.dumps(out), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
