"""The packet classifier (host/irt_void.cpp through irt.void_packets and irt.interior_packets) swept
over classifier_cameras' battery: every named camera on every scene it is defined for at four frame
sizes, 24 seeded random cameras at 96x72.

Soundness against the FLOAT32 evaluation the kernel and the reference run (classifier_cameras'
restatement, pinned here to oracle_box_test and oracle_intersect_sphere): every ray of every
flagged void packet passes boxTest with both discriminants negative; every ray of every flagged
interior packet passes the checks of test_interior_cpu._check_packets.  The rays: every active
pixel, the four jitter corners, the centre, 64 seeded jitters, and for named cameras the LCG's own
jitters of accumIDs 0, 1 and 1000.

Not vacuous: measured against the float64 census with no margin, never against the classifier.
Flagged is a subset of the census; an admitted named camera whose census holds 8 packets of a class
gets at least one flagged; three quarters of the admitted cameras have 8 census packets of each
class at 96x72 (a condition on the battery).

Each case prints one line: flagged / census counts per class and the smallest slack seen, in units
of eps = 2^-19: min over void rays of -disc / (4 A P^2), min over interior rays of the inner
sphere's disc / (4 A P^2).  DESIGN 5.1 carries the table.

What the sweep notices, tried on mutated copies of host/irt_void.cpp:
- eps = 0, and the 72 R limit at 720 R: the 72.5 R camera classifies (11 cases fail).  No ray goes
  wrong at eps = 0: delta's 4e-5 rad and the 1 % on the cone's half-angle are worth about an eps
  themselves below 72 R, and the float error stays under its bound of 0.58 eps.
- section 4(c)'s m_k rule applied where hi_k < r: 40 cases fail, all on the window scene, with rays
  that are not in the front-and-back case.
- the clamp's 4e-5 dropped from delta: not noticed by any camera of the fovy rule (the clamp turns a
  ray by up to 2e-5 rad, only where a component of its direction passes through zero, and a flagged
  packet's cone keeps its rectangle 0.2 pixels clear of the limb even at the finest piece).  The
  probe limb_clamp (classifier_cameras.PROBES: 3e-6 rad per pixel, the outer limb 5.5e-6 rad beyond
  the column where x vanishes) notices it at all four sizes: the packets beside that column are
  flagged void, and their rays within 1e-5 of it, the jitter corners among them, are lifted onto
  the globe and hit in float32 (-2.4 eps).
- rho <= 4 for rho <= 1/4: not noticed by the battery, whose smallest interior slack is 12 eps (the
  cone around a packet keeps it 1.7 pixels off the inner limb).  No ray goes wrong under it either:
  rho is a factor of safety over the float error's bound.  What it promises is that every interior
  ray's float32 disc / (4 A P^2) keeps 4 eps less the float error, and that is asserted (>= 3 eps).
  The probe limb_rho (the inner limb from 71 R at 3e-6 rad per pixel) brings the slack seen down to
  4.7 eps under the certificate as it is and to 2.8 eps under the mutant, which fails there at all
  four sizes (as does eps = 0, a second way).

The probes hold one class each by construction, so they are not counted among the battery's
cameras in the three-quarters condition; each must hold 8 census packets of its class at 96x72
and get one flagged.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import classifier_cameras as CC
import irt
import oracle as O
from classifier_cameras import F, _box32, _packet_rects, _rays32, _recip_ok, _sphere32, _void32

LCG_IDS = (0, 1, 1000)
CASES = [(n, s, W, H) for n in CC.NAMED for s in CC.scenes_of(n) for W, H in CC.SIZES]
CASES += [(n, "flat", 96, 72) for n in CC.RANDOM]
CASES += [(n, "flat", W, H) for n in CC.PROBES for W, H in CC.SIZES]


def _pin(org, lo, hi, r_in, r_out, rays, hits):
    """The restatement against the oracle's functions: the return values and the exact floats."""
    L = O.olib()
    box = O.b3(lo.tolist(), hi.tolist())
    for d, t0, st1, st4, st2, st3 in rays[:200]:
        a, b = C.c_float(), C.c_float()
        assert L.oracle_box_test(O.v3(org), O.v3(d), 0.0, 1e10, box, C.byref(a), C.byref(b)) == 1 and F(a.value) == t0
        got = L.oracle_intersect_sphere(O.v3(org), O.v3(d), r_out, C.byref(a), C.byref(b))
        assert got == hits and (not hits or (F(a.value) == st1 and F(b.value) == st4))
        got = L.oracle_intersect_sphere(O.v3(org), O.v3(d), r_in, C.byref(a), C.byref(b))
        assert got == hits and (not hits or (F(a.value) == st2 and F(b.value) == st3))


def _one_per_packet(ps):
    """Index of the first pixel of each packet in packet_pixels' order."""
    return np.nonzero(np.concatenate([[True], ps[1:] != ps[:-1]]))[0]


@functools.lru_cache(maxsize=None)
def _case(name, scene, W, H):
    """Every check of one (camera, scene, size); returns its record for the table."""
    inf = CC.info(scene)
    lp = CC.launch_params(name, scene, W, H)
    void = irt.void_packets(lp, inf, W, H)
    interior = irt.interior_packets(lp, inf, W, H)
    x0, y0, _, _ = _packet_rects(W, H)
    active = (x0 < W) & (y0 < H)
    assert not (void & interior).any(), "a packet both void and interior"
    assert not (void | interior)[~active].any(), "a packet without an active pixel is flagged"
    cam = lp.camera12()
    org = cam[0:3]
    lo, hi = CC.box32(inf)
    r_in, r_out = CC.radii(scene)
    P2 = float(np.dot(org.astype(np.float64), org.astype(np.float64)))
    lcg = () if name in CC.RANDOM else LCG_IDS
    rec = dict(void=int(void.sum()), interior=int(interior.sum()), slack_void=np.inf, slack_interior=np.inf)

    xs, ys, ps = CC.packet_pixels(W, H, void)
    if len(xs):
        ju, jv = CC.jitters_for(W, H, xs, ys, lcg)
        _, d = _rays32(cam, xs[:, None], ys[:, None], ju, jv)
        ok, disc, A = _void32(org, d, lo, hi, r_in, r_out)
        assert ok.all(), ("void packets with a ray that hits in float32, or leaves the box", np.unique(ps[~ok.all(1)]))
        rec["slack_void"] = float((-disc.astype(np.float64) / (4.0 * A * P2)).min() / CC.EPS)
        k = _one_per_packet(ps)
        _, t0, _ = _box32(org, d[k, 0], lo, hi)
        _pin(org, lo, hi, r_in, r_out, [(d[i, 0], t, None, None, None, None) for i, t in zip(k, t0)], 0)

    xs, ys, ps = CC.packet_pixels(W, H, interior)
    if len(xs):
        ju, jv = CC.jitters_for(W, H, xs, ys, lcg)
        ln, d = _rays32(cam, xs[:, None], ys[:, None], ju, jv)
        hit, t0, _ = _box32(org, d, lo, hi)
        bad = lambda m: np.unique(ps[m.any(1)])  # noqa: E731
        assert hit.all(), ("boxTest", bad(~hit))
        dO, A, qO, st1, st4 = _sphere32(org, d, r_out)
        dI, _, qI, st2, st3 = _sphere32(org, d, r_in)
        assert (dO >= 0).all() and (dI >= 0).all(), ("a sphere is missed", bad((dO < 0) | (dI < 0)))
        assert (t0 < st2).all() and not (st4 < t0).any(), ("not the front-and-back case", bad(~(t0 < st2) | (st4 < t0)))
        assert _recip_ok(ln).all() and _recip_ok(A).all() and _recip_ok(qO).all() and _recip_ok(qI).all()
        assert (np.abs(A - F(1)) < 1e-4).all()
        rec["slack_interior"] = float((dI.astype(np.float64) / (4.0 * A * P2)).min() / CC.EPS)
        # section 4(b): the exact disc / (4 D^2) of every tested ray is at least g >= 4 eps P^2 and the
        # float one is off by less than eps P^2, so it keeps 3 eps P^2 (what rho <= 1/4 promises)
        assert rec["slack_interior"] >= 3.0, ("an interior ray with less than the certified discriminant", rec["slack_interior"])
        k = _one_per_packet(ps)
        _pin(org, lo, hi, r_in, r_out, [(d[i, 0], t0[i, 0], st1[i, 0], st4[i, 0], st2[i, 0], st3[i, 0]) for i in k], 1)

    # a tile list and a strided launch: the whole frame's flags at their own index
    total = irt.num_tiles(W, H)
    tiles = list(range(total))[::-2]
    for fn, whole in ((irt.void_packets, void), (irt.interior_packets, interior)):
        whole = whole.reshape(-1, 64)
        assert np.array_equal(fn(lp, inf, W, H, tiles=tiles).reshape(-1, 64), whole[tiles])
        if total > 1:
            assert np.array_equal(fn(lp, inf, W, H, tile_begin=1, tile_stride=2).reshape(-1, 64), whole[1::2])

    cv, ci = CC.census_void(lp, inf, W, H), CC.census_interior(lp, inf, W, H)
    rec.update(census_void=int(cv.sum()), census_interior=int(ci.sum()))
    assert not (void & ~cv).any(), "a void packet outside the float64 census"
    assert not (interior & ~ci).any(), "an interior packet outside the float64 census"
    return rec


def _line(name, scene, W, H, r):
    s = lambda v: "     -" if not np.isfinite(v) else f"{v:6.1f}"  # noqa: E731
    return (f"| {name} | {scene} | {W}x{H} | {r['void']} / {r['census_void']} | {r['interior']} / {r['census_interior']} | "
            f"{s(r['slack_void']).strip()} | {s(r['slack_interior']).strip()} |")


@pytest.mark.parametrize("name,scene,W,H", CASES, ids=[f"{n}-{s}-{W}x{H}" for n, s, W, H in CASES])
def test_flagged_packets_hold_in_float32(name, scene, W, H):
    r = _case(name, scene, W, H)
    print(_line(name, scene, W, H, r))
    if CC.refuses(name):
        assert r["void"] == 0 and r["interior"] == 0, "a camera beyond the certificate's limits classified"
    elif name in CC.NAMED:
        for cls in ("void", "interior"):
            assert r[cls] >= 1 or r["census_" + cls] < 8, f"no {cls} packet where the census holds {r['census_' + cls]}"
    elif name in CC.PROBES and (W, H) == (96, 72):  # a probe holds its one class, and there is something to find
        cls = CC.PROBES[name][2]
        assert r["census_" + cls] >= 8 and r[cls] >= 1, (cls, r)


def test_the_battery_has_something_to_find():
    """At 96x72, from the census alone: three quarters of the admitted cameras hold at least 8
    packets of each class (each camera on the first scene it is defined for)."""
    admitted = [n for n in list(CC.NAMED) + list(CC.RANDOM) if not CC.refuses(n)]
    both = []
    for n in admitted:
        r = _case(n, CC.scenes_of(n)[0], 96, 72)
        both.append(r["census_void"] >= 8 and r["census_interior"] >= 8)
    print(f"{sum(both)} of {len(admitted)} admitted cameras hold 8 census packets of each class at 96x72; "
          f"without: {[n for n, b in zip(admitted, both) if not b]}")
    assert 4 * sum(both) >= 3 * len(admitted)


def test_the_limits_lie_between_the_paired_cameras():
    R = CC.radii("flat")[1]
    for inside, outside in (("P1.0011", "P1.0009"), ("P71.5", "P72.5")):
        a, b = (np.linalg.norm(CC.camera(n, "flat")[0]) / R for n in (inside, outside))
        lim = 1.001 if a < 2 else (0.01 / CC.EPS) ** 0.5
        assert min(a, b) < lim < max(a, b) and not CC.refuses(inside) and CC.refuses(outside)
        assert _case(inside, "flat", 96, 72)["void"] > 0 and _case(inside, "flat", 96, 72)["interior"] > 0


def test_refusals():
    """The AE raygen, grid mode and a NaN camera word classify nothing, in both classes, for a camera
    that otherwise classifies both."""
    W, H = 96, 72
    inf = CC.info("flat")
    fresh = lambda **kw: irt.setup_frame(CC.cells("flat"), W, H, camera=CC.camera("P3", "flat"), info=inf, **kw).lp  # noqa: E731
    assert irt.void_packets(fresh(), inf, W, H).any() and irt.interior_packets(fresh(), inf, W, H).any()
    lps = []
    lps.append(fresh(raygen=irt.RAYGEN_AE))
    lp = fresh()
    lp.accelMode = 1
    lps.append(lp)
    for field in ("org", "dir_00", "dir_du", "dir_dv"):
        for axis in "xyz":
            lp = fresh()
            setattr(getattr(lp, field), axis, float("nan"))
            lps.append(lp)
    for lp in lps:
        assert not irt.void_packets(lp, inf, W, H).any() and not irt.interior_packets(lp, inf, W, H).any()
