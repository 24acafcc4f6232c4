"""Scenes, value ranges, band edges and expected histograms shared by tests/test_histogram_cpu.py
(irt_histogram_cells against a NumPy restatement, and the census of these inputs by the helper alone)
and tests/test_gpu_histogram.py (irt_histogram on the device against the helper, integer for
integer).  Everything is computed once per process and read-only."""
import functools

import numpy as np

import irt
import sample_scenes as S

F = np.float32
SCENE_NAMES = S.SCENE_NAMES                   # flat, terrain, filtered
COUNTS = (1, 63, 64, 65, 255, 256, 257)       # records of the hand-made set
BINS = (1, 2, 7, 300, 4096)
WEIGHTINGS = ("count", "thickness")
BAND_SETS = ("none", "three", "sixtyfour")    # the last with at most 64 bins (4096 counters in all)
RANGES = ("data", "inner")
HAND_RANGE = (F(0.25), F(0.75))               # the hand-made set's value range


def _frozen(a):
    a.setflags(write=False)
    return a


def special_values():
    """What the bin rule has to get right, as float32: exactly lower and upper, -0.0, the bin edges
    lower + k * (upper - lower) / numBins for several k of every bin count, one float below lower and
    above upper, NaN and both infinities."""
    lo, hi = HAND_RANGE
    v = [lo, hi, F(-0.0), np.nextafter(lo, F(-np.inf)), np.nextafter(hi, F(np.inf)), F(np.nan), F(np.inf),
         F(-np.inf)]
    for nb in BINS:
        for k in sorted({1, nb // 2, nb - 1}):
            if 0 < k < nb:
                v.append(F(lo + F(k) * (hi - lo) / F(nb)))
        v.append(F(lo + F(nb - 0.5) * (hi - lo) / F(nb)))  # the middle of the last bin
    return np.array(v, F)


@functools.lru_cache(maxsize=None)
def hand_made(n):
    """The first n of 640 records with the geometry of irt.synth_grid(2, 1, 40) and, by hand: record 0
    with 31 layers holding every special value; record 1 without layers; record 2 with one layer;
    record 3 of zero thickness (every height the same); from record 4 on every third layer a special
    value.  COUNTS are sizes around the kernel's 4 records per wave and 16 per workgroup and pass."""
    cells = np.array(irt.synth_grid(2, 1, 40), copy=True)
    assert cells.size >= max(COUNTS)
    sp = special_values()
    full = cells[int(np.flatnonzero(cells["numLayers"] == 31)[0])]
    cells["height"][0], cells["numLayers"][0] = full["height"], 31
    cells["value"][0] = F(0.5)
    cells["value"][0][:sp.size] = sp
    if n > 1:
        cells["numLayers"][1] = 0
    if n > 2:
        cells["numLayers"][2] = 1
        cells["value"][2][0] = HAND_RANGE[1]
    if n > 3:
        cells["height"][3] = cells["height"][3][0]
    for r in range(4, cells.size):
        for l in range(int(cells["numLayers"][r])):
            if (r + l) % 3 == 0:
                cells["value"][r][l] = sp[(r * 31 + l) % sp.size]
    return _frozen(np.ascontiguousarray(cells[:n]))


@functools.lru_cache(maxsize=None)
def scene(name):
    """The three scenes of tests/sample_scenes.py, "hand<n>" (hand_made(n)), and "large":
    irt.synth_grid(2, 4, 90), 61,440 records -- fewer than one pass of the kernel's full grid covers
    on a 256-CU device (up to 8 workgroups per CU, 64 records per workgroup and pass: 131,072), so
    tests/test_gpu_histogram.py also runs it with the grid capped at 7 workgroups (138 passes)."""
    if name.startswith("hand"):
        return hand_made(int(name[4:]))
    if name == "large":
        return _frozen(irt.synth_grid(2, 4, 90))
    return S.scene(name)


def layers(cells):
    """(h0, h1, v) of every item (record i, layer l < numLayers[i]), in record order."""
    nl = cells["numLayers"]
    valid = np.arange(31)[None, :] < nl[:, None]
    return cells["height"][:, :31][valid], cells["height"][:, 1:32][valid], cells["value"][:, :31][valid]


def mids(cells):
    h0, h1, _ = layers(cells)
    return ((h0 + h1) * F(0.5)).astype(F)


@functools.lru_cache(maxsize=None)
def value_range(name, key):
    """"data": the scene's dataRange (irt_compute_volume_info); "inner": its middle half, so that both
    value tails fill.  The hand-made sets use HAND_RANGE for both."""
    if name.startswith("hand"):
        return HAND_RANGE
    r = irt.volume_info(scene(name)).dataRange
    lo, hi = F(r.lower), F(r.upper)
    if key == "data":
        return lo, hi
    return F(lo + F(0.25) * (hi - lo)), F(lo + F(0.75) * (hi - lo))


@functools.lru_cache(maxsize=None)
def band_edges(name, key):
    """"none": no edges.  "three": e0 below every layer; e1 exactly one layer's mid-height m (that
    layer is in band 1 by `<=`, and out of band 0 by `<`); e2 strictly between two neighbouring mid-heights
    and e3 the next float, so band 2 is empty; the layers from e3 up -- the top of the shell -- are in
    no band.  "sixtyfour": 64 even bands from below the shell to above it."""
    if key == "none":
        return None
    m = np.unique(mids(scene(name)))
    m = m[np.isfinite(m)]
    lo, hi = (F(m[0]), F(m[-1])) if m.size else (F(6.3e6), F(6.5e6))
    if key == "sixtyfour":
        return _frozen(np.linspace(float(lo) - 10.0, float(hi) + 10.0, 65).astype(F))
    if m.size < 4:  # (a scene of one or two layers: the same shape on made-up radii)
        return _frozen(np.array([lo - F(100), lo, F(hi + F(50)), np.nextafter(F(hi + F(50)), F(np.inf))], F))
    e1 = m[m.size // 3]
    j = 2 * m.size // 3
    while j + 1 < m.size - 1 and not m[j + 1] - m[j] >= F(1.0):
        j += 1
    e2 = F(0.5 * (float(m[j]) + float(m[j + 1])))
    assert e1 < m[j] < e2 < m[j + 1]
    return _frozen(np.array([lo - F(100), e1, e2, np.nextafter(e2, F(np.inf))], F))


def cases(name):
    """Every (range, bins, band set, weighting) of a scene: all bin counts without bands; with three
    bands 1365 in place of 4096, with 64 bands 64 in place of 300 and 4096 (4096 counters are the most)."""
    ranges = ("data",) if name.startswith("hand") else RANGES
    out = []
    for rk in ranges:
        for w in WEIGHTINGS:
            for bk in BAND_SETS:
                for nb in {"none": BINS, "three": (1, 2, 7, 300, 1365), "sixtyfour": (1, 2, 7, 64)}[bk]:
                    out.append((rk, nb, bk, w))
    return out


@functools.lru_cache(maxsize=None)
def expected(name, rk, bins, bk, weighting):
    """irt_histogram_cells of the case: {bins (bands, bins), tails (bands, 3), outside (1)}, uint64."""
    r = irt.histogram_cells(scene(name), value_range(name, rk), bins, weighting, band_edges(name, bk))
    return {k: _frozen(a) for k, a in r.items()}


def numpy_histogram(cells, vrange, bins, weighting, edges):
    """The definition restated in NumPy, float32 expression by expression."""
    h0, h1, v = layers(cells)
    lo, hi = F(vrange[0]), F(vrange[1])
    with np.errstate(all="ignore"):
        if weighting == "count":
            w = np.ones(v.size, np.uint64)
        else:
            d = (h1 - h0).astype(F)
            ok = (d > F(0)) & (d <= F(1048576.0))
            w = (np.where(ok, d, F(0)) * F(64.0)).astype(F).astype(np.uint64)
        bands = 1 if edges is None else len(edges) - 1
        band = np.zeros(v.size, np.int64)
        if edges is not None:
            m = ((h0 + h1).astype(F) * F(0.5)).astype(F)
            band[:] = -1
            for b in range(bands):
                band[(F(edges[b]) <= m) & (m < F(edges[b + 1]))] = b
        t = ((v - lo).astype(F) / F(hi - lo)).astype(F)
        bad = ~np.isfinite(v) | np.isnan(t)
        under = ~bad & (t < F(0))
        over = ~bad & ~under & (t > F(1))
        inside = ~bad & ~under & ~over
        k = np.minimum((np.where(inside, t, F(0)) * F(bins)).astype(F).astype(np.int64), bins - 1)
    keep = w > 0
    assert float(w.sum(dtype=np.float64)) < 2.0 ** 53  # bincount sums in float64: exact below 2^53
    wf = w.astype(np.float64)

    def count(sel, idx, size):
        sel = sel & keep & (band >= 0)
        return np.bincount(idx[sel], weights=wf[sel], minlength=size).astype(np.uint64)

    out_bins = count(inside, band * bins + k, bands * bins).reshape(bands, bins)
    tails = (count(under, 3 * band, 3 * bands) + count(over, 3 * band + 1, 3 * bands) +
             count(bad, 3 * band + 2, 3 * bands)).reshape(bands, 3)
    outside = np.array([w[keep & (band < 0)].sum(dtype=np.uint64)], np.uint64)
    return {"bins": out_bins, "tails": tails, "outside": outside, "weight_sum": int(w.sum(dtype=np.uint64))}


def differs(got, want):
    """None when bins, tails and outside are the same integers, else a description of the first difference."""
    for k in irt.HISTOGRAM_OUTPUTS:
        a, b = np.asarray(got[k]).astype(np.uint64).reshape(-1), np.asarray(want[k]).astype(np.uint64).reshape(-1)
        if a.shape != b.shape:
            return f"{k}: {a.size} against {b.size} counters"
        bad = np.flatnonzero(a != b)
        if bad.size:
            return f"{k}: {bad.size} of {a.size} counters differ, first [{bad[0]}]: {a[bad[0]]} against {b[bad[0]]}"
    return None
