"""irt -- Python binding of the MI355X ICON renderer's C ABI (include/icon_rt_hip.h).

Thin ctypes layer over ``icon-ray-tracing_amd/libicon_rt_hip.so`` (built in-tree by
``make -C icon-ray-tracing_amd``).  It mirrors the host flow of the reference app
``icon_rt`` (szellmann/icon-ray-tracing, icon_rt/hostCode.cu:703-968): load ``.ic``
records, lat/lon filter, volume facts, default transfer function, camera, then frame
launches on the GPU.  There is no CPU fallback: without the library or a HIP device the
calls raise ``IrtError``.
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass

import numpy as np

PKG_DIR = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# IRT_LIB_PATH: another build of the same library (profiles/ A/B runs only)
LIB_PATH = os.environ.get("IRT_LIB_PATH") or os.path.join(PKG_DIR, "libicon_rt_hip.so")

# icon_rt::ICONCell (icon_rt/ICONGrid.h:59-76), 284 bytes, the `.ic` record
CELL_DTYPE = np.dtype(
    [("lat", "<f4", (3,)), ("lon", "<f4", (3,)), ("numLayers", "<i4"),
     ("height", "<f4", (32,)), ("value", "<f4", (32,))], align=False)
assert CELL_DTYPE.itemsize == 284

RAYGEN_WITH_ACCEL = 0  # woodcockTrackingWithAccel (deviceCode.cu:281-341)
RAYGEN_AE = 1          # woodcockTrackingAE (deviceCode.cu:239-275)
ACCEL_SPHERE = 0       # SPHERE_ACCEL_MODE (Params.h:33): sdda over the shell grid
ACCEL_GRID = 1         # GRID_ACCEL_MODE (Params.h:34): dda3 over the 256^3 grid
MODE_USER_GEOM = 0     # Volume::mode (Params.h:29-31): sample() on the cells (default)
MODE_TRIANGLES = 1     # closest bottom triangle toward the centre (deviceCode.cu:61-76)
MODE_CUBQL = 2         # wedges + intersectWedgeEXT (deviceCode.cu:90-115)
MAX_LEVELS = 16        # IRT_MAX_LEVELS: the most radii of one render_levels call
LEVELS_BACK = 1        # IRT_LEVELS_BACK: also the far-side hits of spheres the camera is outside of
COLUMN_WSUM, COLUMN_MAX, COLUMN_MIN = 0, 1, 2  # IRT_COLUMN_*: the product render_column shows
# The raygen's render variants (irt_kernels.h OPT_* bits), all bit-identical: the product
# library compiles 73405728 (the default: one-wave workgroups since round 4, 5 waves/SIMD; since
# round 5 with the miss mode, the LDS-DMA prologue tables and the DPP prefix, and 73667872 its
# form without the miss mode, which hole-free scenes run),
# 5376 (256-thread workgroups; the persistent launch's base) and 36864 (per-wave statistics);
# libicon_rt_hip_all.so (`make VARIANTS=all`) adds the A/B variants: 4096 no waves-per-SIMD
# floor, 5120 at 4 waves/SIMD, 70656 the one-lane-per-ray Woodcock loop, 136192 per-lane
# candidate scans, 529408 per-region shader-clock timing (profiles/probe.py),
# 2102272 / 2102528 less LDS per workgroup, 6296576 / 6296832 one-wave workgroups (6558976 the latter without
# the miss mode: round 4's and early round 5's defaults), 529664 the timing variant
# at 5 waves/SIMD, 2102784 the lean-LDS build at 6 waves/SIMD, 33559808 the certified fast
# lat/lon for the sdda cells (OPT_FASTSPH).
ALL_LIB_PATH = os.path.join(PKG_DIR, "libicon_rt_hip_all.so")


def compiled_variants() -> tuple:
    """The render variants the loaded library compiled (irt_debug_variants)."""
    L = lib()
    n = L.irt_debug_variants(None, 0)
    out = (C.c_int * n)()
    L.irt_debug_variants(out, n)
    return tuple(out)


E_INVALID, E_HIP, E_DATA, E_IO, E_CHAIN = -1, -2, -3, -4, -5  # IRT_E_* (icon_rt_hip.h)


class IrtError(RuntimeError):
    def __init__(self, msg, code=None):
        super().__init__(msg)
        self.code = code


class Vec3(C.Structure):
    _fields_ = [("x", C.c_float), ("y", C.c_float), ("z", C.c_float)]

    def tolist(self):
        return [self.x, self.y, self.z]


class Vec4(C.Structure):
    _fields_ = [("x", C.c_float), ("y", C.c_float), ("z", C.c_float), ("w", C.c_float)]


class Box1(C.Structure):
    _fields_ = [("lower", C.c_float), ("upper", C.c_float)]


class Box3(C.Structure):
    _fields_ = [("lower", Vec3), ("upper", Vec3)]


class LaunchParams(C.Structure):
    """Per-frame part of icon_rt::LaunchParams (icon_rt/Params.h:92-119)."""
    _fields_ = [("org", Vec3), ("dir_00", Vec3), ("dir_du", Vec3), ("dir_dv", Vec3),
                ("accumID", C.c_int32), ("ambientColor", Vec3), ("ambientRadiance", C.c_float),
                ("unitDistance", C.c_float), ("raygen", C.c_int32), ("accelMode", C.c_int32),
                ("mode", C.c_int32)]

    def camera12(self) -> np.ndarray:
        return np.array(self.org.tolist() + self.dir_00.tolist() + self.dir_du.tolist()
                        + self.dir_dv.tolist(), dtype=np.float32)


class VolumeInfo(C.Structure):
    _fields_ = [("numCells", C.c_uint64), ("bounds", Box3), ("sphericalBounds", Box3),
                ("dataRange", Box1), ("unitDistance", C.c_float), ("shellDims", C.c_int32 * 3),
                ("locatorFaceRes", C.c_int32), ("locatorEntries", C.c_uint64),
                ("deviceBytes", C.c_uint64)]


class RenderStats(C.Structure):
    _fields_ = [("raysLaunched", C.c_uint64), ("raysInBox", C.c_uint64),
                ("locateCalls", C.c_uint64), ("samplesFound", C.c_uint64),
                ("candidatesTested", C.c_uint64), ("kernelMs", C.c_float)]

    def asdict(self):
        return {f: getattr(self, f) for f, _ in self._fields_}


_lib = None


class ColumnOut(C.Structure):
    """irt_column_out: where each output of a column reduction goes (0: not written)."""
    _fields_ = [(n, C.c_void_p) for n in ("wsum", "vmax", "vmin", "kmax", "kmin", "count")]


COLUMN_OUTPUTS = {"wsum": np.float32, "vmax": np.float32, "vmin": np.float32,
                  "kmax": np.int32, "kmin": np.int32, "count": np.int32}


class SectionOut(C.Structure):
    """irt_section_out: where each output of a section goes (0: not written)."""
    _fields_ = [("value", C.c_void_p), ("found", C.c_void_p), ("rgba", C.c_void_p), ("column", ColumnOut)]


SECTION_OUTPUTS = {"value": np.float32, "found": np.uint8, "rgba": np.uint32}  # per point; COLUMN_OUTPUTS per column


class HistogramOut(C.Structure):
    """irt_histogram_out: where bins, tails and outside go (0: not written); uint64 each."""
    _fields_ = [(n, C.c_void_p) for n in ("bins", "tails", "outside")]


HISTOGRAM_OUTPUTS = ("bins", "tails", "outside")
HIST_COUNT, HIST_THICKNESS = 0, 1  # IRT_HIST_*
HIST_WEIGHTINGS = {"count": HIST_COUNT, "thickness": HIST_THICKNESS}
HIST_MAX_BINS, HIST_MAX_BANDS = 4096, 64


class OverlayStyle(C.Structure):
    """irt_overlay_style: a straight-alpha colour and a half-width in radians on the sphere."""
    _fields_ = [("rgba", Vec4), ("halfWidth", C.c_float)]


# irt_overlay_segment: 64 B
SEGMENT_DTYPE = np.dtype([("a", "<f4", (3,)), ("b", "<f4", (3,)), ("n", "<f4", (3,)), ("t", "<f4", (3,)),
                          ("sinHalf", "<f4"), ("style", "<i4"), ("pad", "<u4", (2,))])
OVERLAY_MAX_STYLES = 8      # IRT_OVERLAY_MAX_STYLES
OVERLAY_OVER = 1            # IRT_OVERLAY_OVER: the lines on top of the frame
OVERLAY_MAX_HALF_WIDTH = 0.05
OVERLAY_MAX_ARC = 0.2
OVERLAY_MAX_BINS = 256
CONTOUR_WRAP = 1            # IRT_CONTOUR_WRAP: the grid closes in longitude
CONTOUR_MAX_THRESHOLDS = 16  # IRT_CONTOUR_MAX_THRESHOLDS


def lib() -> C.CDLL:
    """Load the in-tree product library (fails loudly if it was not built)."""
    global _lib
    if _lib is None:
        # One HIP runtime per process: PyTorch-ROCm bundles its own libamdhip64 (soname
        # libamdhip64.so.7, like /opt/rocm's).  Loading torch first makes the dynamic
        # linker bind our library to that same runtime, so torch tensors' device pointers,
        # streams and RCCL are shared with the kernels.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        if not os.path.exists(LIB_PATH):
            raise IrtError(f"{LIB_PATH} not built; run `make -C icon-ray-tracing_amd` "
                           "(or __graft_entry__.build())")
        L = C.CDLL(LIB_PATH)
        P, I, F, S = C.c_void_p, C.c_int, C.c_float, C.c_size_t
        L.irt_last_error.restype = C.c_char_p
        sig = {
            "irt_create": [P, S, I, C.POINTER(P)],
            "irt_create_begin": [S, I, C.POINTER(P)],
            "irt_create_append": [P, P, S],
            "irt_create_end": [P],
            "irt_create_from_file": [C.c_char_p, C.c_long, I, C.POINTER(P)],
            "irt_create_synth": [I, I, I, F, F, C.c_uint32, I, C.POINTER(P)],
            "irt_create_synth_terrain": [I, I, I, F, F, C.c_uint32, F, I, C.POINTER(P)],
            "irt_debug_context_array": [P, I, P, S, C.POINTER(S)],
            "irt_debug_scene_array": [P, I, P, S, C.POINTER(S)],
            "irt_destroy": [P],
            "irt_get_volume_info": [P, C.POINTER(VolumeInfo)],
            "irt_set_transfunc": [P, P, I, Box1, F],
            "irt_update_values": [P, S, S, P],
            "irt_update_values_device": [P, S, S, P, P],
            "irt_update_values_end": [P],
            "irt_sample_points": [P, I, P, S, P, P, F, P],
            "irt_sample_latlon": [P, I, P, I, P, I, P, I, P, P, F, P],
            "irt_latlon_points": [P, I, P, I, P, I, P],
            "irt_render_levels": [P, C.POINTER(LaunchParams), I, I, P, I, I, P, P, P, P, F, P],
            "irt_levels_order": [P, I, P, P],
            "irt_column_reduce": [P, P, I, S, P, F, ColumnOut],
            "irt_column_latlon": [P, I, P, I, P, I, P, P, I, ColumnOut, F, P],
            "irt_render_column": [P, C.POINTER(LaunchParams), I, I, F, P, P, I, I, P, P, P, F, P],
            "irt_section": [P, I, P, P, I, P, P, I, Vec3, F, SectionOut, F, P],
            "irt_section_points": [P, P, I, P, I, P],
            "irt_great_circle": [F, F, F, F, I, P, P, C.POINTER(C.c_double)],
            "irt_histogram": [P, Box1, I, I, P, I, HistogramOut, P],
            "irt_histogram_cells": [P, S, Box1, I, I, P, I, HistogramOut],
            "irt_overlay_segments": [P, P, P, I, F, I, P, S, C.POINTER(S)],
            "irt_graticule": [F, F, F, I, P, S, C.POINTER(S)],
            "irt_overlay_bins": [P, S, F, I, P, P, S, C.POINTER(S)],
            "irt_overlay_cover": [P, S, P, I, P, P, I, P, S, P],
            "irt_overlay_create": [P, P, S, P, I, I, C.POINTER(P)],
            "irt_overlay_destroy": [P, P],
            "irt_overlay_get_bins": [P, P, C.POINTER(I), C.POINTER(S)],
            "irt_overlay_width": [C.POINTER(LaunchParams), F, F, C.POINTER(F)],
            "irt_render_overlay": [P, P, C.POINTER(LaunchParams), I, I, F, I, P, P, P, P, P],
            "irt_contour_cells": [P, P, P, I, P, I, P, P, I, I, P, S, C.POINTER(S), P],
            "irt_contour_grid": [P, P, P, P, I, P, I, P, P, I, I, P, S, C.POINTER(S), P, P],
            "irt_contour_latlon": [P, I, P, I, P, I, F, P, P, I, I, P, S, C.POINTER(S), P, P],
            "irt_debug_sample_admits": [F, F, F],
            "irt_clear_frame": [P, P, P, S, P],
            "irt_render": [P, C.POINTER(LaunchParams), I, I, P, P, P],
            "irt_render_tiles": [P, C.POINTER(LaunchParams), I, I, I, I, P, P,
                                 C.POINTER(C.c_int), P],
            "irt_render_accumulate": [P, C.POINTER(LaunchParams), I, I, I, P, P, P],
            "irt_render_sequence": [P, C.POINTER(LaunchParams), I, I, I, P, P, P],
            "irt_render_tiles_accumulate": [P, C.POINTER(LaunchParams), I, I, I, I, I, P, P,
                                            C.POINTER(C.c_int), P],
            "irt_unpack_tiles": [P, P, I, I, I, I, P, P],
            "irt_deal_tiles": [C.POINTER(LaunchParams), C.POINTER(VolumeInfo), I, I, I, F, P, S,
                               C.POINTER(C.c_int)],
            "irt_render_tile_list": [P, C.POINTER(LaunchParams), I, I, P, I, I, P, P, P],
            "irt_unpack_tile_table": [P, P, I, I, P, I, I, P, P],
            "irt_get_render_stats": [P, C.POINTER(RenderStats)],
            "irt_get_render_stats_total": [P, C.POINTER(RenderStats), C.POINTER(C.c_longlong)],
            "irt_reset_render_stats_total": [P],
            "irt_set_timing_interval": [P, C.c_int],
            "irt_get_shell": [P, P, P],
            "irt_get_grid": [P, P, P],
            "irt_build_wedge_accel": [P, P, S],
            "irt_num_tiles": [I, I],
            "irt_load_ic": [C.c_char_p, C.c_long, P, S, C.POINTER(S)],
            "irt_save_ic": [C.c_char_p, P, S],
            "irt_convert_icon": [C.POINTER(ConvertOpts), P, S, C.POINTER(S)],
            "irt_convert_icon_umesh": [C.POINTER(ConvertOpts), C.c_char_p, C.POINTER(S), C.POINTER(S)],
            "irt_filter_cells": [P, S, Box1, Box1, C.POINTER(S)],
            "irt_compute_volume_info": [P, S, C.POINTER(VolumeInfo)],
            "irt_default_transfunc": [Box1, P, C.POINTER(Box1)],
            "irt_resample_lut": [P, I, P, I],
            "irt_camera_view_all": [Box3, F, I, I, C.POINTER(LaunchParams)],
            "irt_camera_look_at": [Vec3, Vec3, Vec3, F, I, I, C.POINTER(LaunchParams)],
            "irt_synth_grid": [I, I, I, F, F, C.c_uint32, P, S, C.POINTER(S)],
            "irt_synth_grid_terrain": [I, I, I, F, F, C.c_uint32, F, P, S, C.POINTER(S)],
            # host-only inspection (include/icon_rt_hip_debug.h)
            "irt_debug_asinf": [F],
            "irt_debug_atan2f": [F, F],
            "irt_debug_f2i": [F],
            "irt_debug_logf_entry": [C.c_uint32],
            "irt_debug_srgb_thresholds": [P],
            "irt_debug_scene_build": [P, S, C.POINTER(P)],
            "irt_debug_scene_info": [P, C.POINTER(VolumeInfo)],
            "irt_debug_scene_locate": [P, Vec3, C.POINTER(C.c_float), C.POINTER(C.c_uint32)],
            "irt_debug_scene_locate_binned": [P, Vec3, C.POINTER(C.c_float),
                                              C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)],
            "irt_debug_scene_candidates": [P, Vec3, P, I],
            "irt_debug_scene_planes": [P, C.c_uint32, P],
            "irt_debug_scene_values": [P, C.c_uint32, F, P],
            "irt_debug_logf_mismatches": [],
            "irt_debug_host_woodcock_log": [P],
            "irt_debug_device_woodcock_log": [I, P],
            "irt_debug_scene_free": [P],
        }
        for name, args in sig.items():
            fn = getattr(L, name)
            fn.argtypes = args
            if name not in ("irt_last_error",):
                fn.restype = C.c_int
        L.irt_debug_asinf.restype = F
        L.irt_debug_atan2f.restype = F
        L.irt_debug_logf_entry.restype = F
        L.irt_destroy.restype = None
        L.irt_debug_scene_free.restype = None
        L.irt_debug_srgb_thresholds.restype = None
        _lib = L
    return _lib


def _check(rc: int, what: str):
    if rc != 0:
        msg = lib().irt_last_error().decode(errors="replace")
        raise IrtError(f"{what} failed ({rc}): {msg}", rc)


def _ptr(a: np.ndarray) -> C.c_void_p:
    return C.c_void_p(a.ctypes.data)


def levels_radii(radii) -> np.ndarray:
    """render_levels' radii as the library takes them: 1 to MAX_LEVELS float32, each finite and
    positive (checked here as irt_render_levels checks them, so that a bad list names itself)."""
    r = np.ascontiguousarray(radii, dtype=np.float32).reshape(-1)
    if not 1 <= r.size <= MAX_LEVELS:
        raise IrtError(f"render_levels: {r.size} levels are outside [1, {MAX_LEVELS}]", E_INVALID)
    bad = np.flatnonzero(~(np.isfinite(r) & (r > 0)))
    if bad.size:
        raise IrtError(f"render_levels: radius[{bad[0]}] = {r[bad[0]]} is not finite and positive", E_INVALID)
    return r


def levels_order(radii):
    """irt_levels_order: (sorted, index) -- the radii in render_levels' near order (descending,
    ties by ascending index) and each one's index into `radii`."""
    r = np.ascontiguousarray(radii, dtype=np.float32).reshape(-1)
    out, idx = np.zeros(r.size, np.float32), np.zeros(r.size, np.int32)
    _check(lib().irt_levels_order(_ptr(r), r.size, _ptr(out), _ptr(idx)), "irt_levels_order")
    return out, idx


def _weights(weight, levels: int):
    """A column call's weights: None, or `levels` float32."""
    if weight is None:
        return None
    w = np.ascontiguousarray(weight, dtype=np.float32).reshape(-1)
    if w.size != levels:
        raise IrtError(f"{w.size} weights for {levels} levels", E_INVALID)
    return w


def column_reduce(value, found, weight=None, miss: float = float("nan")) -> dict:
    """irt_column_reduce: the column reduction of value / found (levels, ...) -- sample_latlon's
    layout -- over the first axis, on the host: a dict of wsum, vmax, vmin (float32), kmax, kmin,
    count (int32), each of shape value.shape[1:].  weight: None (every weight 1) or one float per
    level.  No GPU."""
    value = np.ascontiguousarray(value, dtype=np.float32)
    found = np.ascontiguousarray(found, dtype=np.uint8)
    if value.ndim < 1 or value.shape != found.shape:
        raise IrtError(f"column_reduce: value {value.shape} and found {found.shape} differ", E_INVALID)
    levels, shape = value.shape[0], value.shape[1:]
    w = _weights(weight, levels)
    out = {k: np.zeros(shape, t) for k, t in COLUMN_OUTPUTS.items()}
    _check(lib().irt_column_reduce(_ptr(value), _ptr(found), levels, int(np.prod(shape, dtype=np.int64)),
                                   _ptr(w) if w is not None else None, float(miss),
                                   ColumnOut(**{k: a.ctypes.data for k, a in out.items()})), "irt_column_reduce")
    return out


def _hist_args(weighting, band_edges):
    """A histogram call's weighting (a name or an IRT_HIST_* number) and band edges (None: one band;
    else at least two float32 edges) as the library takes them: (weighting, edges or None, bands)."""
    w = HIST_WEIGHTINGS.get(weighting, weighting)
    if not isinstance(w, (int, np.integer)):
        raise IrtError(f"histogram: weighting {weighting!r} is none of {sorted(HIST_WEIGHTINGS)}", E_INVALID)
    if band_edges is None:
        return int(w), None, 1
    e = np.ascontiguousarray(band_edges, dtype=np.float32).reshape(-1)
    if e.size < 2:
        raise IrtError(f"histogram: {e.size} band edges (at least 2)", E_INVALID)
    return int(w), e, e.size - 1


def histogram_cells(cells, value_range, bins: int, weighting="count", band_edges=None) -> dict:
    """irt_histogram_cells, the histogram's definition on the host (no GPU): the (record, layer) items
    of `cells` binned by value over value_range = (lower, upper) into `bins` bins, per altitude band
    when band_edges (ascending radii, metres from the centre) is given; weighting "count" (1 per
    item) or "thickness" (the layer's thickness in 1/64 m).  Returns uint64 arrays: bins (bands,
    bins), tails (bands, 3: under, over, not finite) and outside (1: items in no band)."""
    cells = np.ascontiguousarray(cells, dtype=CELL_DTYPE)
    w, e, bands = _hist_args(weighting, band_edges)
    out = {"bins": np.zeros((bands, max(int(bins), 0)), np.uint64), "tails": np.zeros((bands, 3), np.uint64),
           "outside": np.zeros(1, np.uint64)}
    _check(lib().irt_histogram_cells(_ptr(cells), cells.size, box1(*value_range), int(bins), w,
                                     _ptr(e) if e is not None else None, bands,
                                     HistogramOut(**{k: a.ctypes.data for k, a in out.items()})), "irt_histogram_cells")
    return out


def _segments(seg) -> np.ndarray:
    seg = np.ascontiguousarray(seg, dtype=SEGMENT_DTYPE).reshape(-1)
    assert SEGMENT_DTYPE.itemsize == 64
    return seg


def overlay_styles(styles):
    """Styles as the library takes them: a sequence of ((r, g, b, a), half_width) -- straight alpha, the
    half-width in radians on the sphere -- as an array of OverlayStyle."""
    styles = list(styles)
    arr = (OverlayStyle * max(len(styles), 1))()
    for k, (rgba, w) in enumerate(styles):
        arr[k] = OverlayStyle(Vec4(*(float(x) for x in rgba)), float(w))
    return arr, len(styles)


def overlay_segments(lat, lon, first=None, max_arc: float = 0.0174533, style: int = 0) -> np.ndarray:
    """irt_overlay_segments: polylines (lat, lon float32 radians; points first[l] .. first[l+1]-1 are
    line l, None: one line) as great-circle segments no longer than max_arc, a SEGMENT_DTYPE array.
    No GPU."""
    lat = np.ascontiguousarray(lat, dtype=np.float32).reshape(-1)
    lon = np.ascontiguousarray(lon, dtype=np.float32).reshape(-1)
    if lat.size != lon.size:
        raise IrtError(f"overlay_segments: {lat.size} lat for {lon.size} lon", E_INVALID)
    first = np.ascontiguousarray([0, lat.size] if first is None else first, dtype=np.int32).reshape(-1)
    if first.size < 1 or (first.size > 1 and int(first[-1]) > lat.size):
        raise IrtError(f"overlay_segments: first ends at {first[-1] if first.size else None} of {lat.size} points",
                       E_INVALID)
    n = C.c_size_t()
    args = (_ptr(lat), _ptr(lon), _ptr(first), first.size - 1, float(max_arc), int(style))
    _check(lib().irt_overlay_segments(*args, None, 0, C.byref(n)), "irt_overlay_segments")
    out = np.zeros(n.value, SEGMENT_DTYPE)
    _check(lib().irt_overlay_segments(*args, _ptr(out), out.size, C.byref(n)), "irt_overlay_segments")
    return out


def graticule(step_lat: float, step_lon: float, max_arc: float = 0.0174533, style: int = 0) -> np.ndarray:
    """irt_graticule: meridians every step_lon and parallels every step_lat (radians) as segments no
    longer than max_arc (parallels: chains of great-circle arcs).  No GPU."""
    n = C.c_size_t()
    args = (float(step_lat), float(step_lon), float(max_arc), int(style))
    _check(lib().irt_graticule(*args, None, 0, C.byref(n)), "irt_graticule")
    out = np.zeros(n.value, SEGMENT_DTYPE)
    _check(lib().irt_graticule(*args, _ptr(out), out.size, C.byref(n)), "irt_graticule")
    return out


def overlay_bins(segments, max_half_width: float, bins_per_edge: int):
    """irt_overlay_bins: (binStart (6 N^2 + 1), binSeg), uint32 -- the cube-map bin table as CSR, each
    bin's list ascending.  No GPU."""
    seg = _segments(segments)
    N = int(bins_per_edge)
    if not 1 <= N <= OVERLAY_MAX_BINS:
        raise IrtError(f"overlay_bins: binsPerEdge {N} is outside [1, {OVERLAY_MAX_BINS}]", E_INVALID)
    start = np.zeros(6 * N * N + 1, np.uint32)
    n = C.c_size_t()
    _check(lib().irt_overlay_bins(_ptr(seg), seg.size, float(max_half_width), N, _ptr(start), None, 0, C.byref(n)),
           "irt_overlay_bins")
    lists = np.zeros(n.value, np.uint32)
    _check(lib().irt_overlay_bins(_ptr(seg), seg.size, float(max_half_width), N, _ptr(start), _ptr(lists), lists.size,
                                  C.byref(n)), "irt_overlay_bins")
    return start, lists


def overlay_cover(segments, styles, u, bins=None, bins_per_edge: int = 0) -> np.ndarray:
    """irt_overlay_cover: the segment (lowest covering index, or -1) of every unit vector of u (..., 3)
    float32, int32 of shape u.shape[:-1].  bins: None scans every segment; (binStart, binSeg) of
    overlay_bins with its bins_per_edge scans each point's bin only.  No GPU."""
    seg = _segments(segments)
    st, ns = overlay_styles(styles)
    u = np.ascontiguousarray(u, dtype=np.float32)
    if u.ndim < 1 or u.shape[-1] != 3:
        raise IrtError(f"overlay_cover: u of shape {u.shape} (..., 3)", E_INVALID)
    out = np.full(u.shape[:-1], -2, np.int32)
    start, lists = bins if bins is not None else (None, None)
    _check(lib().irt_overlay_cover(_ptr(seg), seg.size, st, ns, _ptr(start) if start is not None else None,
                                   _ptr(lists) if lists is not None else None, int(bins_per_edge), _ptr(u),
                                   out.size, _ptr(out)), "irt_overlay_cover")
    return out


def overlay_width(lp: LaunchParams, height: int, surface_radius: float, pixels: float) -> float:
    """irt_overlay_width: the half-width in radians on the sphere of surface_radius of a line `pixels`
    pixels wide at the sub-camera point of lp's camera, for styles: a pixel's angle at the frame's centre
    is |dir_dv| over dir_00's component along dir_du x dir_dv, its footprint that angle times the camera's
    distance from the sphere, and the half-width half of `pixels` footprints over the radius -- clamped
    to the legal range (1e-7, OVERLAY_MAX_HALF_WIDTH].  `height` (the frame dir_dv was made for) must be
    positive and is otherwise not needed.  A convenience; no GPU."""
    if int(height) < 1:
        raise IrtError("overlay_width: height must be positive", E_INVALID)
    w = C.c_float()
    _check(lib().irt_overlay_width(C.byref(lp), float(surface_radius), float(pixels), C.byref(w)), "irt_overlay_width")
    return float(w.value)


def _contour_args(lat, lon, thresholds, styles):
    """A contour call's host arrays as the library takes them: lat, lon, thresholds float32, the
    per-threshold style indices int32 (None: all 0; one int: that style for every threshold)."""
    lat = np.ascontiguousarray(lat, dtype=np.float32).reshape(-1)
    lon = np.ascontiguousarray(lon, dtype=np.float32).reshape(-1)
    thr = np.ascontiguousarray(thresholds, dtype=np.float32).reshape(-1)
    if styles is None or np.ndim(styles) == 0:
        sty = np.full(thr.size, 0 if styles is None else int(styles), np.int32)
    else:
        sty = np.ascontiguousarray(styles, dtype=np.int32).reshape(-1)
    if sty.size != thr.size:
        raise IrtError(f"contour: {sty.size} styles for {thr.size} thresholds", E_INVALID)
    return lat, lon, thr, sty


class ContourError(IrtError):
    """A contour call the library refused; count / counts hold what it had set (capacity < count)."""
    def __init__(self, msg, code, count, counts):
        super().__init__(msg, code)
        self.count, self.counts = count, counts


def _contour_check(rc: int, what: str, n, per):
    if rc != 0:
        msg = lib().irt_last_error().decode(errors="replace")
        raise ContourError(f"{what} failed ({rc}): {msg}", rc, int(n.value), per.copy())


def contour_cells(value, found, lat, lon, thresholds, styles=None, wrap: bool = False, return_counts: bool = False):
    """irt_contour_cells, the isolines' definition on the host (no GPU): the isolines of value
    (len(lat), len(lon)) float32 -- found: the same shape, uint8, or None -- at `thresholds`, as a
    SEGMENT_DTYPE array ordered by threshold, then cell, then within the cell.  styles: the style
    index per threshold.  return_counts: also the segments per threshold (int64)."""
    lat, lon, thr, sty = _contour_args(lat, lon, thresholds, styles)
    value = np.ascontiguousarray(value, dtype=np.float32)
    if value.size != lat.size * lon.size:
        raise IrtError(f"contour_cells: value of shape {value.shape} for a {lat.size} x {lon.size} grid", E_INVALID)
    if found is not None:
        found = np.ascontiguousarray(found, dtype=np.uint8)
        if found.size != value.size:
            raise IrtError(f"contour_cells: found of shape {found.shape} for value {value.shape}", E_INVALID)
    n, per = C.c_size_t(), np.zeros(CONTOUR_MAX_THRESHOLDS, np.uintp)
    args = (_ptr(value), _ptr(found) if found is not None else None, _ptr(lat), lat.size, _ptr(lon), lon.size,
            _ptr(thr), _ptr(sty), thr.size, CONTOUR_WRAP if wrap else 0)
    _contour_check(lib().irt_contour_cells(*args, None, 0, C.byref(n), _ptr(per)), "irt_contour_cells", n, per)
    out = np.zeros(n.value, SEGMENT_DTYPE)
    _contour_check(lib().irt_contour_cells(*args, _ptr(out), out.size, C.byref(n), _ptr(per)), "irt_contour_cells",
                   n, per)
    return (out, per[:thr.size].astype(np.int64)) if return_counts else out


def vec3(v) -> Vec3:
    return Vec3(float(v[0]), float(v[1]), float(v[2]))


def box1(lo, hi) -> Box1:
    return Box1(float(lo), float(hi))


# ------------------------------------------------- value-by-value device hooks (tests only)
def debug_device_div(a: np.ndarray, b: np.ndarray, device: int = 0) -> tuple[np.ndarray, np.ndarray]:
    """irt_debug_device_div: (div_uniform, div_recip or the fallback division) of a / b."""
    a = np.ascontiguousarray(a, dtype=np.float32).ravel()
    b = np.ascontiguousarray(b, dtype=np.float32).ravel()
    u, r = np.zeros(a.size, np.float32), np.zeros(a.size, np.float32)
    L = lib()
    L.irt_debug_device_div.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    _check(L.irt_debug_device_div(device, _ptr(a), _ptr(b), a.size, _ptr(u), _ptr(r)), "irt_debug_device_div")
    return u, r


def debug_ray_tests(rays: np.ndarray, interior: np.ndarray, box6, radius_a: float, radius_b: float,
                    device: int = 0) -> tuple[np.ndarray, np.ndarray]:
    """irt_debug_ray_tests: (flags int32 (n,), out float32 (n, 14)) -- see include/icon_rt_hip_debug.h."""
    rays = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 6)
    interior = np.ascontiguousarray(interior, dtype=np.uint8).ravel()
    box6 = np.ascontiguousarray(box6, dtype=np.float32).ravel()
    flags = np.zeros(len(rays), np.int32)
    out = np.zeros((len(rays), 14), np.float32)
    L = lib()
    L.irt_debug_ray_tests.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_float, C.c_float,
                                      C.c_void_p, C.c_void_p]
    _check(L.irt_debug_ray_tests(device, _ptr(rays), _ptr(interior), len(rays), _ptr(box6), float(radius_a),
                                 float(radius_b), _ptr(flags), _ptr(out)), "irt_debug_ray_tests")
    return flags, out


def debug_gen_ray(lp: "LaunchParams", width: int, height: int, device: int = 0) -> tuple[np.ndarray, np.ndarray]:
    """irt_debug_gen_ray: (dir float32 (H, W, 3), LCG state uint32 (H, W)) of gen_ray per pixel."""
    d = np.zeros((height, width, 3), np.float32)
    st = np.zeros((height, width), np.uint32)
    L = lib()
    L.irt_debug_gen_ray.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    _check(L.irt_debug_gen_ray(device, C.byref(lp), width, height, _ptr(d), _ptr(st)), "irt_debug_gen_ray")
    return d, st


def debug_grid_coord(s: np.ndarray, lo: float, hi: float, dim: int, c: np.ndarray, d: int,
                     device: int = 0) -> tuple[np.ndarray, np.ndarray]:
    """irt_debug_grid_coord: (project_axis_inv of s, wrap_coord of c)."""
    s = np.ascontiguousarray(s, dtype=np.float32).ravel()
    c = np.ascontiguousarray(c, dtype=np.int32).ravel()
    cell, wrapped = np.zeros(s.size, np.int32), np.zeros(c.size, np.int32)
    L = lib()
    L.irt_debug_grid_coord.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_float, C.c_float, C.c_int, C.c_void_p,
                                       C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    _check(L.irt_debug_grid_coord(device, _ptr(s), s.size, float(lo), float(hi), dim, _ptr(cell), _ptr(c), c.size, d,
                                  _ptr(wrapped)), "irt_debug_grid_coord")
    return cell, wrapped


# ----------------------------------------------------------------------- host helpers
def default_kernel_id(ctx=None) -> int:
    """Template id of the raygen kernel (k_render<id>, as rocprofv3 names it) that `ctx`
    launches -- the default variant, its hole-free form (bit 262144) on scenes without holes
    or its located-mode void walk (bit 1073741824) on scenes with holes, with bit 128 (OPT_SLOT)
    where the launches use the slot table (irt_debug_slot_use) -- or, without a context,
    that of the default variant.

    A restatement of the library's launch plan kept for the profile lookups keyed on it; after a
    launch that carried void data it takes the list bit (| 64) from Context.last_plan(), so the
    lookup names the kernel the launch in fact ran (the flat kernel's work-item list form)."""
    L = lib()
    if ctx is not None:
        L.irt_debug_get_variant.argtypes = [C.c_void_p]
        v = int(L.irt_debug_get_variant(ctx._h)) & ~4096
        d = int(L.irt_debug_default_variant())
        L.irt_debug_slot_use.argtypes = [C.c_void_p, C.c_void_p]
        if v in ((d & ~4096), (d | 262144) & ~4096, (d | 1073741824) & ~4096) and L.irt_debug_slot_use(ctx._h, None) == 1:
            v |= 128  # VariantForms::slot: the default kernels' OPT_SLOT form
        elif ctx.void_use() > 0:
            v |= 16  # ... their OPT_VOID form: the last launch carried a void-packet bitmap
            v |= ctx.last_plan()[0] & 64  # ... or the work-item list (OPT_VLIST)
        return v
    return int(L.irt_debug_default_variant()) & ~4096  # OPT_MONO: one kernel per frame


PLAN_SLOTS, PLAN_VOID_BITS, PLAN_VOID_LIST, PLAN_QUEUE, PLAN_CHAIN = 1, 2, 4, 8, 16  # IRT_DEBUG_PLAN_*


def plan(variant: int, sampler: int = 0, accel: int = 0, flags: int = 0, tiles: int = 1, frames: int = 1,
         num_split: int = 0, void_live: int = 0, void_row: int = 0, queue_wg: int = 0) -> tuple:
    """irt_debug_plan (no device): (kernel id, threads, grid x, grid y, k_accumulate blocks) of a
    launch of `variant` with these arguments; flags: PLAN_* bits."""
    L = lib()
    L.irt_debug_plan.argtypes = [C.c_int] * 6 + [C.c_uint32] * 3 + [C.c_int, C.POINTER(C.c_int)]
    out = (C.c_int * 5)()
    _check(L.irt_debug_plan(variant, sampler, accel, flags, tiles, frames, num_split, void_live, void_row,
                            queue_wg, out), "irt_debug_plan")
    return tuple(out)


def variant_workgroups(variant: int, sched: bool, num_tiles: int, frames: int = 1) -> int:
    """irt_debug_variant_workgroups (no device): Context.launch_workgroups for a context of
    `variant` with measured-cost scheduling on or off."""
    L = lib()
    L.irt_debug_variant_workgroups.argtypes = [C.c_int] * 4
    L.irt_debug_variant_workgroups.restype = C.c_longlong
    n = L.irt_debug_variant_workgroups(variant, 1 if sched else 0, num_tiles, frames)
    if n < 0:
        raise IrtError("irt_debug_variant_workgroups failed")
    return n


def synth_grid(root_n: int, bisections: int, levels: int, top_height: float = 75e3,
               noise: float = 0.0, seed: int = 1234, terrain: float = 0.0) -> np.ndarray:
    """Synthetic RnBk ICON grid as `.ic` records (host/irt_synth.cpp); terrain > 0: over
    terrain up to `terrain` metres, as convert_icon writes it (irt_synth_grid_terrain)."""
    n = C.c_size_t()
    _check(lib().irt_synth_grid_terrain(root_n, bisections, levels, top_height, noise, seed, terrain,
                                        None, 0, C.byref(n)), "irt_synth_grid")
    cells = np.zeros(n.value, dtype=CELL_DTYPE)
    _check(lib().irt_synth_grid_terrain(root_n, bisections, levels, top_height, noise, seed, terrain,
                                        _ptr(cells), n.value, C.byref(n)), "irt_synth_grid")
    return cells


def load_ic(path: str, max_num_cells: int = -1) -> np.ndarray:
    n = C.c_size_t()
    _check(lib().irt_load_ic(path.encode(), max_num_cells, None, 0, C.byref(n)), "irt_load_ic")
    cells = np.zeros(n.value, dtype=CELL_DTYPE)
    _check(lib().irt_load_ic(path.encode(), max_num_cells, _ptr(cells), n.value, C.byref(n)),
           "irt_load_ic")
    return cells


class ConvertOpts(C.Structure):
    """irt_convert_opts: convert_icon's command line (convert_icon.cpp:121-161)."""
    _fields_ = [("hgridFile", C.c_char_p), ("hsurfFile", C.c_char_p),
                ("hhlFiles", C.POINTER(C.c_char_p)), ("numHhlFiles", C.c_int),
                ("dataFiles", C.POINTER(C.c_char_p)), ("numDataFiles", C.c_int),
                ("varName", C.c_char_p), ("maxLayers", C.c_int)]


def convert_icon(hgrid: str, hsurf: str, hhl: list, data: list, var: str = "pres",
                 max_layers: int = 5) -> np.ndarray:
    """tools/convert_icon (convert_icon.cpp:168-391): DWD ICON netCDF files -> .ic records."""
    hp = (C.c_char_p * max(len(hhl), 1))(*[f.encode() for f in hhl])
    dp = (C.c_char_p * max(len(data), 1))(*[f.encode() for f in data])
    o = ConvertOpts(hgrid.encode(), hsurf.encode(), hp, len(hhl), dp, len(data), var.encode(),
                    max_layers)
    n = C.c_size_t()
    _check(lib().irt_convert_icon(C.byref(o), None, 0, C.byref(n)), "irt_convert_icon")
    cells = np.zeros(n.value, dtype=CELL_DTYPE)
    _check(lib().irt_convert_icon(C.byref(o), _ptr(cells), n.value, C.byref(n)),
           "irt_convert_icon")
    return cells


def convert_icon_umesh(hgrid: str, hsurf: str, hhl: list, data: list, path: str,
                       var: str = "pres", max_layers: int = 5):
    """convert_icon's UMesh branch (convert_icon.cpp:393-452): writes `path` in umesh's
    binary layout; returns (vertices, wedges) written."""
    hp = (C.c_char_p * max(len(hhl), 1))(*[f.encode() for f in hhl])
    dp = (C.c_char_p * max(len(data), 1))(*[f.encode() for f in data])
    o = ConvertOpts(hgrid.encode(), hsurf.encode(), hp, len(hhl), dp, len(data), var.encode(),
                    max_layers)
    nv, nw = C.c_size_t(), C.c_size_t()
    _check(lib().irt_convert_icon_umesh(C.byref(o), path.encode(), C.byref(nv), C.byref(nw)),
           "irt_convert_icon_umesh")
    return nv.value, nw.value


def read_umesh(path: str) -> dict:
    """The arrays of a .umesh file as irt_convert_icon_umesh writes it (u64-counted)."""
    raw = open(path, "rb").read()
    pos = 0

    def u64():
        nonlocal pos
        v = int(np.frombuffer(raw, np.uint64, 1, pos)[0])
        pos += 8
        return v

    def arr(dtype, width):
        nonlocal pos
        n = u64()
        a = np.frombuffer(raw, dtype, n * width, pos).reshape(n, width) if width > 1 else \
            np.frombuffer(raw, dtype, n, pos)
        pos += a.nbytes
        return a

    out = {"magic": u64(), "vertices": arr(np.float32, 3), "scalars": arr(np.float32, 1)}
    for name, w in (("triangles", 3), ("quads", 4), ("tets", 4), ("pyrs", 5),
                    ("wedges", 6), ("hexes", 8)):
        out[name] = arr(np.int32, w)
    if pos != len(raw):
        raise ValueError(f"{path}: {len(raw) - pos} trailing bytes")
    return out


def save_ic(path: str, cells: np.ndarray):
    cells = np.ascontiguousarray(cells, dtype=CELL_DTYPE)
    _check(lib().irt_save_ic(path.encode(), _ptr(cells), cells.size), "irt_save_ic")


def filter_cells(cells: np.ndarray, lat_range=(-np.inf, np.inf), lon_range=(-np.inf, np.inf)):
    """--lat-range / --lon-range filter in degrees (hostCode.cu:736-758); returns a copy."""
    out = np.array(cells, dtype=CELL_DTYPE, copy=True)
    n = C.c_size_t()
    _check(lib().irt_filter_cells(_ptr(out), out.size, box1(*lat_range), box1(*lon_range),
                                  C.byref(n)), "irt_filter_cells")
    return out[: n.value].copy()


def _latlon_arrays(lat, lon, radius):
    return tuple(np.ascontiguousarray(a, dtype=np.float32).reshape(-1) for a in (lat, lon, radius))


def latlon_points(lat, lon, radius) -> np.ndarray:
    """irt_latlon_points: the points Context.sample_latlon samples, float32 of shape
    (len(radius), len(lat), len(lon), 3): toCartesian(radius[k], lat[j], lon[i]) with the host's
    cosf/sinf (lat/lon in radians, radius in metres from the Earth's centre).  No GPU."""
    lat, lon, radius = _latlon_arrays(lat, lon, radius)
    xyz = np.zeros((radius.size, lat.size, lon.size, 3), np.float32)
    _check(lib().irt_latlon_points(_ptr(lat), lat.size, _ptr(lon), lon.size, _ptr(radius),
                                   radius.size, _ptr(xyz)), "irt_latlon_points")
    return xyz


def _section_arrays(lat, lon, radius):
    lat, lon, radius = _latlon_arrays(lat, lon, radius)
    if lat.size != lon.size:
        raise IrtError(f"a section's columns are (lat, lon) pairs: {lat.size} lat for {lon.size} lon", E_INVALID)
    return lat, lon, radius


def section_points(lat, lon, radius) -> np.ndarray:
    """irt_section_points: the points Context.section samples, float32 of shape (len(radius),
    len(lat), 3): toCartesian(radius[k], lat[c], lon[c]) with the host's cosf/sinf, column c being
    the pair (lat[c], lon[c]) (radians; radius in metres from the Earth's centre).  No GPU."""
    lat, lon, radius = _section_arrays(lat, lon, radius)
    xyz = np.zeros((radius.size, lat.size, 3), np.float32)
    _check(lib().irt_section_points(_ptr(lat), _ptr(lon), lat.size, _ptr(radius), radius.size, _ptr(xyz)),
           "irt_section_points")
    return xyz


def great_circle(lat0: float, lon0: float, lat1: float, lon1: float, n: int):
    """irt_great_circle: (lat, lon, arc) -- n points (float32, radians) along the great circle from
    (lat0, lon0) to (lat1, lon1), the shorter way, equally spaced in angle, the end points being the
    inputs unchanged; arc = the angle between the end points in radians (the plot's x-axis runs
    from 0 to arc).  A polyline is joined leg by leg.  No GPU."""
    n = int(n)
    lat, lon = np.zeros(max(n, 0), np.float32), np.zeros(max(n, 0), np.float32)
    arc = C.c_double()
    _check(lib().irt_great_circle(float(lat0), float(lon0), float(lat1), float(lon1), n, _ptr(lat), _ptr(lon),
                                  C.byref(arc)), "irt_great_circle")
    return lat, lon, arc.value


def sample_admits(x: float, y: float, z: float) -> bool:
    """irt_debug_sample_admits: whether the sampling calls hand the point to a locator (its
    float squared length is finite and positive); every other point is a miss by definition."""
    return lib().irt_debug_sample_admits(C.c_float(x), C.c_float(y), C.c_float(z)) == 1


def volume_info(cells: np.ndarray) -> VolumeInfo:
    cells = np.ascontiguousarray(cells, dtype=CELL_DTYPE)
    info = VolumeInfo()
    _check(lib().irt_compute_volume_info(_ptr(cells), cells.size, C.byref(info)),
           "irt_compute_volume_info")
    return info


def default_transfunc(data_range) -> tuple[np.ndarray, tuple[float, float]]:
    """hostCode.cu:823-836 + Pipeline::setTransfunc resampling (pipeline.cu:469-473)."""
    lut = np.zeros((300, 4), dtype=np.float32)
    vr = Box1()
    _check(lib().irt_default_transfunc(box1(*data_range), _ptr(lut), C.byref(vr)),
           "irt_default_transfunc")
    return lut, (vr.lower, vr.upper)


def resample_lut(src: np.ndarray, n: int) -> np.ndarray:
    src = np.ascontiguousarray(src, dtype=np.float32).reshape(-1, 4)
    dst = np.zeros((n, 4), dtype=np.float32)
    _check(lib().irt_resample_lut(_ptr(src), src.shape[0], _ptr(dst), n), "irt_resample_lut")
    return dst


def camera_view_all(bounds: Box3, img_w: int, img_h: int, fovy_deg: float = 90.0) -> LaunchParams:
    lp = LaunchParams()
    _check(lib().irt_camera_view_all(bounds, fovy_deg, img_w, img_h, C.byref(lp)),
           "irt_camera_view_all")
    return lp


def camera_look_at(vp, vi, vu, fovy_deg: float, img_w: int, img_h: int) -> LaunchParams:
    lp = LaunchParams()
    _check(lib().irt_camera_look_at(vec3(vp), vec3(vi), vec3(vu), fovy_deg, img_w, img_h,
                                    C.byref(lp)), "irt_camera_look_at")
    return lp


def num_tiles(w: int, h: int) -> int:
    return lib().irt_num_tiles(w, h)


def deal_tiles(lp: LaunchParams, info: VolumeInfo, w: int, h: int, ranks: int,
               rank0_extra: float = 0.0) -> np.ndarray:
    """irt_deal_tiles: the cost-balanced deal of the frame's 64x64 tiles over `ranks` ranks,
    (ranks, max_tiles) int32, row r = rank r's tiles in render order, -1 padding; rank 0
    carries rank0_extra x a frame's cost besides its tiles."""
    m = C.c_int()
    _check(lib().irt_deal_tiles(C.byref(lp), C.byref(info), w, h, ranks, rank0_extra, None, 0,
                                C.byref(m)), "irt_deal_tiles")
    table = np.full((ranks, m.value), -1, np.int32)
    _check(lib().irt_deal_tiles(C.byref(lp), C.byref(info), w, h, ranks, rank0_extra,
                                _ptr(table), table.size, C.byref(m)), "irt_deal_tiles")
    return table


class VoidCache:
    """irt_debug_void_packets with a cache of its own, as a context's launches keep one."""

    def __init__(self):
        L = lib()
        L.irt_debug_void_cache_create.restype = C.c_void_p
        L.irt_debug_void_cache_free.argtypes = [C.c_void_p]
        L.irt_debug_void_cache_free.restype = None
        self._h = C.c_void_p(L.irt_debug_void_cache_create())
        self.computations = 0

    def packets(self, lp, info, w, h, tile_begin=0, tile_stride=1, tiles=None):
        out = void_packets(lp, info, w, h, tile_begin, tile_stride, tiles, cache=self)
        return out

    def __del__(self):
        if getattr(self, "_h", None):
            lib().irt_debug_void_cache_free(self._h)
            self._h = None


def void_packets(lp: LaunchParams, info: VolumeInfo, w: int, h: int, tile_begin: int = 0,
                 tile_stride: int = 1, tiles=None, cache: VoidCache = None) -> np.ndarray:
    """irt_debug_void_packets: bool per packet of the launch (4 * block + wave, 64 per launch tile):
    every ray of the packet, whatever the jitter, passes boxTest and misses the outer sphere."""
    L = lib()
    L.irt_debug_void_packets.argtypes = [C.c_void_p, C.POINTER(LaunchParams), C.POINTER(VolumeInfo), C.c_int,
                                         C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p,
                                         C.c_size_t, C.POINTER(C.c_uint32), C.POINTER(C.c_longlong)]
    total = num_tiles(w, h)
    t = None if tiles is None else np.ascontiguousarray(tiles, dtype=np.int32)
    nt = len(t) if t is not None else (max(0, (total - tile_begin + tile_stride - 1) // tile_stride)
                                       if tile_begin < total else 0)
    bits = np.zeros(max(2 * nt, 1), np.uint32)
    n, comp = C.c_uint32(), C.c_longlong()
    _check(L.irt_debug_void_packets(cache._h if cache else None, C.byref(lp), C.byref(info), w, h, tile_begin,
                                    tile_stride, _ptr(t) if t is not None else None, nt if t is not None else 0,
                                    _ptr(bits), bits.size, C.byref(n), C.byref(comp)), "irt_debug_void_packets")
    if cache:
        cache.computations = comp.value
    out = ((bits[:2 * nt, None] >> np.arange(32, dtype=np.uint32)[None, :]) & 1).astype(bool).reshape(-1)
    assert int(out.sum()) == n.value
    return out


def interior_packets(lp: LaunchParams, info: VolumeInfo, w: int, h: int, tile_begin: int = 0,
                     tile_stride: int = 1, tiles=None, cache: VoidCache = None) -> np.ndarray:
    """irt_debug_interior_packets: bool per packet of the launch, numbered as void_packets numbers them:
    every ray of the packet, whatever the jitter, passes boxTest, hits both spheres and takes the
    front-and-back ranges with the fast divisions' guards holding."""
    L = lib()
    L.irt_debug_interior_packets.argtypes = [C.c_void_p, C.POINTER(LaunchParams), C.POINTER(VolumeInfo), C.c_int,
                                             C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p,
                                             C.c_size_t, C.POINTER(C.c_uint32), C.POINTER(C.c_longlong)]
    total = num_tiles(w, h)
    t = None if tiles is None else np.ascontiguousarray(tiles, dtype=np.int32)
    nt = len(t) if t is not None else (max(0, (total - tile_begin + tile_stride - 1) // tile_stride)
                                       if tile_begin < total else 0)
    bits = np.zeros(max(2 * nt, 1), np.uint32)
    n, comp = C.c_uint32(), C.c_longlong()
    _check(L.irt_debug_interior_packets(cache._h if cache else None, C.byref(lp), C.byref(info), w, h, tile_begin,
                                        tile_stride, _ptr(t) if t is not None else None, nt if t is not None else 0,
                                        _ptr(bits), bits.size, C.byref(n), C.byref(comp)),
           "irt_debug_interior_packets")
    if cache:
        cache.computations = comp.value
    out = ((bits[:2 * nt, None] >> np.arange(32, dtype=np.uint32)[None, :]) & 1).astype(bool).reshape(-1)
    assert int(out.sum()) == n.value
    return out


def void_lists(lp: LaunchParams, info: VolumeInfo, w: int, h: int, frames: int, tile_begin: int = 0,
               tile_stride: int = 1, tiles=None, cache: VoidCache = None):
    """irt_debug_void_lists: the work items of a chained launch of `frames` frames that renders its void
    packets once -- (live, void): live (Lp,) uint32, the live part every grid row shares; void (frames, Vr)
    uint32, each row's void part; packets as 4 * block + wave, 0xFFFFFFFF an empty item.  None when
    the request has no void packet (the launch runs the plain grid)."""
    L = lib()
    L.irt_debug_void_lists.argtypes = [C.c_void_p, C.POINTER(LaunchParams), C.POINTER(VolumeInfo), C.c_int, C.c_int,
                                       C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_size_t,
                                       C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    t = None if tiles is None else np.ascontiguousarray(tiles, dtype=np.int32)
    live, row, n = C.c_uint32(), C.c_uint32(), C.c_uint32()

    def call(items):
        _check(L.irt_debug_void_lists(cache._h if cache else None, C.byref(lp), C.byref(info), w, h, tile_begin,
                                      tile_stride, _ptr(t) if t is not None else None, len(t) if t is not None else 0,
                                      frames, _ptr(items) if items is not None else None,
                                      items.size if items is not None else 0, C.byref(live), C.byref(row), C.byref(n)),
               "irt_debug_void_lists")

    call(None)
    if n.value == 0:
        return None
    items = np.zeros(live.value + frames * row.value, np.uint32)
    call(items)
    return items[:live.value].copy(), items[live.value:].reshape(frames, row.value).copy()


@dataclass
class FrameSetup:
    """What icon_rt's main() derives before the first launch (hostCode.cu:736-958)."""
    lp: LaunchParams
    lut: np.ndarray
    value_range: tuple[float, float]
    opacity_scale: float
    info: VolumeInfo


# The survey's framing camera: --camera 0 0 1.4e7 0 0 0 0 1 0 -fovy 60
FRAMING_CAMERA = ((0.0, 0.0, 1.4e7), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 60.0)


def setup_frame(cells: np.ndarray, width: int, height: int, camera=None,
                camera_div=None, raygen: int = RAYGEN_WITH_ACCEL, info: VolumeInfo = None) -> FrameSetup:
    """Mirror hostCode.cu main(): volume facts, default TF, unitDistance, camera.

    info: the volume facts when already known (Context.info: a streamed context never
          holds the whole cell array on the host); otherwise computed from `cells`.

    camera: None -> Camera::viewAll(volbounds) with fovy 90 (hostCode.cu:819-821);
            (vp, vi, vu, fovyDeg) -> Pipeline --camera/-fovy (pipeline.cu:444-454).
    camera_div: the image size dir_du/dir_dv are divided by; the reference hard-codes
            512 (hostCode.cu:815,944-945); default: the real (width, height).
    """
    if info is None:
        info = volume_info(cells)
    lut, vr = default_transfunc((info.dataRange.lower, info.dataRange.upper))
    dw, dh = camera_div if camera_div is not None else (width, height)
    if camera is None:
        lp = camera_view_all(info.bounds, dw, dh)
    else:
        vp, vi, vu, fovy = camera
        lp = camera_look_at(vp, vi, vu, fovy, dw, dh)
    lp.accumID = 0
    lp.ambientColor = Vec3(1.0, 1.0, 1.0)
    lp.ambientRadiance = 1.0
    lp.unitDistance = info.unitDistance
    lp.raygen = raygen
    return FrameSetup(lp=lp, lut=lut, value_range=vr, opacity_scale=1.0, info=info)


# scene arrays the render kernel reads (irt_debug_context_array / irt_debug_scene_array)
SCENE_ARRAYS = {"bin_hdr": 0, "fat": 1, "blocks": 2, "sph_r": 3, "sph_off": 4, "sph_rec": 5,
                "sph_bits": 6}
# ... and those only a context holds: the slot table (irt_common.h kSlot4; empty when the
# scene's cells do not share their radial edges, or with IRT_SLOTS=0) and GRID_ACCEL_MODE's
# empty-space bitmap (k_grid_bits; empty until the grid is built)
CONTEXT_ARRAYS = {"slots": 7, "grid_bits": 8}


def _array(fn, h, name):
    which = SCENE_ARRAYS[name] if name in SCENE_ARRAYS else CONTEXT_ARRAYS[name]
    n = C.c_size_t()
    _check(fn(h, which, None, 0, C.byref(n)), "scene array")
    out = np.zeros(max(n.value, 1), np.uint8)
    _check(fn(h, which, _ptr(out), n.value, C.byref(n)), "scene array")
    return out[:n.value]


def check_update_values(values) -> np.ndarray:
    """The argument check of Context.update_values: a float32 array of shape (n, 32),
    C-contiguous -- nothing is converted or copied on the way to the library."""
    if not isinstance(values, np.ndarray) or values.dtype != np.float32:
        raise TypeError("update_values: values must be a float32 numpy array")
    if values.ndim != 2 or values.shape[1] != 32:
        raise ValueError(f"update_values: values must have shape (n, 32), not {values.shape}")
    if not values.flags.c_contiguous:
        raise ValueError("update_values: values must be C-contiguous")
    return values


# ----------------------------------------------------------------------- GPU context
class Context:
    """One renderer context on one HIP device (irt_create ... irt_destroy).

    Context(cells) uploads a host array; Context.synth / Context.from_file /
    Context.streamed feed the cells to HBM chunk by chunk (irt_create_begin / _append /
    _end), so host memory stays at one chunk."""

    def __init__(self, cells: np.ndarray = None, device: int = 0, _handle=None):
        if _handle is None:
            cells = np.ascontiguousarray(cells, dtype=CELL_DTYPE)
            _handle = C.c_void_p()
            _check(lib().irt_create(_ptr(cells), cells.size, device, C.byref(_handle)),
                   "irt_create")
        self._h = _handle
        self.device = device
        self.info = VolumeInfo()
        _check(lib().irt_get_volume_info(self._h, C.byref(self.info)), "irt_get_volume_info")

    @classmethod
    def synth(cls, root_n: int, bisections: int, levels: int, device: int = 0,
              top_height: float = 75e3, noise: float = 0.0, seed: int = 1234,
              terrain: float = 0.0) -> "Context":
        """The grid of synth_grid(...), generated straight into HBM (irt_create_synth /
        irt_create_synth_terrain)."""
        h = C.c_void_p()
        _check(lib().irt_create_synth_terrain(root_n, bisections, levels, top_height, noise, seed,
                                              terrain, device, C.byref(h)), "irt_create_synth")
        return cls(device=device, _handle=h)

    @classmethod
    def from_file(cls, path: str, max_num_cells: int = -1, device: int = 0) -> "Context":
        """A `.ic` file streamed into HBM (irt_create_from_file, hostCode.cu:717-734)."""
        h = C.c_void_p()
        _check(lib().irt_create_from_file(path.encode(), max_num_cells, device, C.byref(h)),
               "irt_create_from_file")
        return cls(device=device, _handle=h)

    @classmethod
    def streamed(cls, chunks, num_cells: int, device: int = 0) -> "Context":
        """`num_cells` records from an iterable of record arrays, in order."""
        h = C.c_void_p()
        _check(lib().irt_create_begin(num_cells, device, C.byref(h)), "irt_create_begin")
        try:
            for ch in chunks:
                ch = np.ascontiguousarray(ch, dtype=CELL_DTYPE)
                _check(lib().irt_create_append(h, _ptr(ch), ch.size), "irt_create_append")
            _check(lib().irt_create_end(h), "irt_create_end")
        except Exception:
            lib().irt_destroy(h)
            raise
        return cls(device=device, _handle=h)

    def array(self, name: str) -> np.ndarray:
        """A scene array as the device built it (bytes; irt_debug_context_array)."""
        return _array(lib().irt_debug_context_array, self._h, name)

    def array_bytes(self, name: str) -> int:
        """The size of a scene array, without copying it."""
        which = SCENE_ARRAYS[name] if name in SCENE_ARRAYS else CONTEXT_ARRAYS[name]
        n = C.c_size_t()
        _check(lib().irt_debug_context_array(self._h, which, None, 0, C.byref(n)), "scene array")
        return n.value

    def close(self):
        if getattr(self, "_h", None):
            lib().irt_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def set_transfunc(self, lut: np.ndarray, value_range, opacity_scale: float = 1.0):
        lut = np.ascontiguousarray(lut, dtype=np.float32).reshape(-1, 4)
        _check(lib().irt_set_transfunc(self._h, _ptr(lut), lut.shape[0], box1(*value_range),
                                       float(opacity_scale)), "irt_set_transfunc")

    def update_values(self, values: np.ndarray, first: int = 0):
        """irt_update_values: values[k, j] becomes value[j] of record first + k (all 32 j);
        float32, shape (n, 32), C-contiguous.  Commit with end_update()."""
        values = check_update_values(values)
        _check(lib().irt_update_values(self._h, int(first), values.shape[0], _ptr(values)),
               "irt_update_values")

    def update_values_device(self, ptr: int, n: int, first: int = 0, stream: int = 0):
        """irt_update_values_device: the same from n x 32 float32 in device memory at `ptr`
        (a torch tensor's data_ptr()), enqueued on `stream`."""
        _check(lib().irt_update_values_device(self._h, int(first), int(n), C.c_void_p(ptr),
                                              C.c_void_p(stream)), "irt_update_values_device")

    def end_update(self):
        """irt_update_values_end: commits the updates (shell, data range, majorants, grid);
        self.info is read again, so info.dataRange is the new range."""
        _check(lib().irt_update_values_end(self._h), "irt_update_values_end")
        _check(lib().irt_get_volume_info(self._h, C.byref(self.info)), "irt_get_volume_info")

    def set_statistics(self, on: bool):
        """Per-launch event counts on (default) or off (irt_set_statistics); frames are
        identical either way, the counts read 0 while off."""
        L = lib()
        L.irt_set_statistics.argtypes = [C.c_void_p, C.c_int]
        _check(L.irt_set_statistics(self._h, 1 if on else 0), "irt_set_statistics")

    def set_queue(self, on: bool):
        """Persistent launches (every resident wave pulls 8x8 packets from a per-launch
        counter) on or off for this context; frames are identical either way."""
        L = lib()
        L.irt_debug_set_queue.argtypes = [C.c_void_p, C.c_int]
        _check(L.irt_debug_set_queue(self._h, 1 if on else 0), "irt_debug_set_queue")

    def set_wg_trace(self, ptr: int):
        """Measurement only: the next renders' workgroups write {start, end, HW_ID, XCC_ID}
        to the device buffer at `ptr` (4 u32 per workgroup; 0: off)."""
        L = lib()
        L.irt_debug_set_wg_trace.argtypes = [C.c_void_p, C.c_void_p]
        _check(L.irt_debug_set_wg_trace(self._h, C.c_void_p(ptr or None)), "irt_debug_set_wg_trace")

    def set_chain(self, on: bool):
        """Chained progressive frames (default on): a multi-frame launch lerps each frame
        straight into accum/fb instead of through the sample buffer + k_accumulate; frames are
        identical either way."""
        L = lib()
        L.irt_debug_set_chain.argtypes = [C.c_void_p, C.c_int]
        _check(L.irt_debug_set_chain(self._h, 1 if on else 0), "irt_debug_set_chain")

    def chain_errors(self) -> int:
        """Launches whose chained-frame waits timed out (0 in every correct run); retires
        every launch in flight (waits for the device)."""
        L = lib()
        L.irt_debug_chain_errors.argtypes = [C.c_void_p]
        n = L.irt_debug_chain_errors(self._h)
        if n < 0:
            raise IrtError("irt_debug_chain_errors failed")
        return n

    def set_chain_fault(self, spins: int, withhold_frame: int = -1):
        """Test hook: chained waits give up after `spins` polls (0: default) and frame
        `withhold_frame`'s waves never publish (-1: none) -- the IRT_E_CHAIN path."""
        L = lib()
        L.irt_debug_set_chain_fault.argtypes = [C.c_void_p, C.c_uint32, C.c_int]
        _check(L.irt_debug_set_chain_fault(self._h, spins, withhold_frame), "irt_debug_set_chain_fault")

    def sched_split(self):
        """(split work items of the last launch -- parts x split packets, padded with empty items to
        a multiple of 8 -- and log2 of the parts per packet): measured-cost scheduling."""
        L = lib()
        L.irt_debug_sched_split.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        n, lg = C.c_int(), C.c_int()
        _check(L.irt_debug_sched_split(self._h, C.byref(n), C.byref(lg)), "irt_debug_sched_split")
        return n.value, lg.value

    def void_use(self) -> int:
        """Packets the last launch rendered as void (a chained launch of progressive frames renders
        the packets that miss the globe in every frame once); 0: that path was not taken."""
        L = lib()
        if not hasattr(L, "irt_debug_void_use"):  # an older build loaded through IRT_LIB_PATH (A/B tools)
            return 0
        L.irt_debug_void_use.argtypes = [C.c_void_p]
        L.irt_debug_void_use.restype = C.c_longlong
        return L.irt_debug_void_use(self._h)

    def interior_use(self) -> int:
        """Packets the last launch flagged interior for its kernel (the host's count of the class it
        uploaded: such packets' rays are set up with no box test and no range guards); 0: no void
        data, or no such packet."""
        L = lib()
        if not hasattr(L, "irt_debug_interior_use"):  # an older build loaded through IRT_LIB_PATH (A/B tools)
            return 0
        L.irt_debug_interior_use.argtypes = [C.c_void_p]
        L.irt_debug_interior_use.restype = C.c_longlong
        return L.irt_debug_interior_use(self._h)

    def last_workgroups(self) -> int:
        """Workgroups the last launch dispatched for its raygen (grid x * grid y)."""
        L = lib()
        L.irt_debug_last_workgroups.argtypes = [C.c_void_p]
        L.irt_debug_last_workgroups.restype = C.c_longlong
        return L.irt_debug_last_workgroups(self._h)

    def last_plan(self) -> tuple:
        """irt_debug_last_plan: (kernel id, threads, grid x, grid y, k_accumulate blocks) of the
        last launch, as irt.plan gives them."""
        L = lib()
        L.irt_debug_last_plan.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
        out = (C.c_int * 5)()
        _check(L.irt_debug_last_plan(self._h, out), "irt_debug_last_plan")
        return tuple(out)

    def launch_workgroups(self, num_tiles: int, frames: int = 1) -> int:
        """Workgroups of one launch of num_tiles tiles x frames (the wg-trace buffer needs 4
        u32 per workgroup)."""
        L = lib()
        L.irt_debug_launch_workgroups.argtypes = [C.c_void_p, C.c_int, C.c_int]
        L.irt_debug_launch_workgroups.restype = C.c_longlong
        n = L.irt_debug_launch_workgroups(self._h, num_tiles, frames)
        if n < 0:
            raise IrtError("irt_debug_launch_workgroups failed")
        return n

    def queue(self) -> bool:
        L = lib()
        L.irt_debug_get_queue.argtypes = [C.c_void_p]
        return L.irt_debug_get_queue(self._h) == 1

    def clear(self, fb_ptr: int, accum_ptr: int, num_pixels: int, stream: int = 0):
        _check(lib().irt_clear_frame(self._h, C.c_void_p(fb_ptr), C.c_void_p(accum_ptr),
                                     num_pixels, C.c_void_p(stream)), "irt_clear_frame")

    def render(self, lp: LaunchParams, width: int, height: int, fb_ptr: int, accum_ptr: int,
               stream: int = 0):
        _check(lib().irt_render(self._h, C.byref(lp), width, height, C.c_void_p(fb_ptr),
                                C.c_void_p(accum_ptr), C.c_void_p(stream)), "irt_render")

    def render_tiles(self, lp: LaunchParams, width: int, height: int, tile_begin: int,
                     tile_stride: int, fb_ptr: int, accum_ptr: int, stream: int = 0) -> int:
        n = C.c_int()
        _check(lib().irt_render_tiles(self._h, C.byref(lp), width, height, tile_begin,
                                      tile_stride, C.c_void_p(fb_ptr), C.c_void_p(accum_ptr),
                                      C.byref(n), C.c_void_p(stream)), "irt_render_tiles")
        return n.value

    def render_sequence(self, lps, width: int, height: int, fb_ptr: int, accum_ptr: int,
                        stream: int = 0):
        """irt_render_sequence: lps[k] (camera and accumID per frame) in one launch."""
        arr = (LaunchParams * len(lps))(*lps)
        _check(lib().irt_render_sequence(self._h, arr, len(lps), width, height, C.c_void_p(fb_ptr),
                                         C.c_void_p(accum_ptr), C.c_void_p(stream)),
               "irt_render_sequence")

    def render_tile_list_sequence(self, lps, width: int, height: int, tiles, fb_tiles_ptr: int,
                                  accum_tiles_ptr: int, stream: int = 0):
        """irt_render_tile_list_sequence: lps[k] over the listed tiles, packed in list order."""
        arr = (LaunchParams * len(lps))(*lps)
        t = np.ascontiguousarray(tiles, dtype=np.int32)
        L = lib()
        L.irt_render_tile_list_sequence.argtypes = [C.c_void_p, C.POINTER(LaunchParams), C.c_int, C.c_int, C.c_int,
                                                    C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        _check(L.irt_render_tile_list_sequence(self._h, arr, len(lps), width, height, _ptr(t), t.size,
                                               C.c_void_p(fb_tiles_ptr), C.c_void_p(accum_tiles_ptr),
                                               C.c_void_p(stream)), "irt_render_tile_list_sequence")

    def render_accumulate(self, lp: LaunchParams, width: int, height: int, num_frames: int,
                          fb_ptr: int, accum_ptr: int, stream: int = 0):
        """Frames lp.accumID .. lp.accumID+num_frames-1 of the progressive accumulation in
        one launch (irt_render_accumulate)."""
        _check(lib().irt_render_accumulate(self._h, C.byref(lp), width, height, num_frames,
                                           C.c_void_p(fb_ptr), C.c_void_p(accum_ptr),
                                           C.c_void_p(stream)), "irt_render_accumulate")

    def render_tiles_accumulate(self, lp: LaunchParams, width: int, height: int, tile_begin: int,
                                tile_stride: int, num_frames: int, fb_ptr: int, accum_ptr: int,
                                stream: int = 0) -> int:
        n = C.c_int()
        _check(lib().irt_render_tiles_accumulate(self._h, C.byref(lp), width, height, tile_begin,
                                                 tile_stride, num_frames, C.c_void_p(fb_ptr),
                                                 C.c_void_p(accum_ptr), C.byref(n),
                                                 C.c_void_p(stream)), "irt_render_tiles_accumulate")
        return n.value

    def render_tile_list(self, lp: LaunchParams, width: int, height: int, tiles, num_frames: int,
                         fb_tiles_ptr: int, accum_tiles_ptr: int, stream: int = 0):
        """irt_render_tile_list: the listed tiles (row-major ids), packed in list order."""
        t = np.ascontiguousarray(tiles, dtype=np.int32)
        _check(lib().irt_render_tile_list(self._h, C.byref(lp), width, height, _ptr(t), t.size,
                                          num_frames, C.c_void_p(fb_tiles_ptr),
                                          C.c_void_p(accum_tiles_ptr), C.c_void_p(stream)),
               "irt_render_tile_list")

    def unpack_tile_table(self, gathered_ptr: int, table: np.ndarray, width: int, height: int,
                          fb_ptr: int, stream: int = 0):
        """irt_unpack_tile_table: rank-major packed tiles whose ids are table[rank, k]."""
        t = np.ascontiguousarray(table, dtype=np.int32)
        _check(lib().irt_unpack_tile_table(self._h, C.c_void_p(gathered_ptr), t.shape[0], t.shape[1],
                                           _ptr(t), width, height, C.c_void_p(fb_ptr),
                                           C.c_void_p(stream)), "irt_unpack_tile_table")

    def unpack_tiles(self, gathered_ptr: int, num_ranks: int, max_tiles: int, width: int,
                     height: int, fb_ptr: int, stream: int = 0):
        _check(lib().irt_unpack_tiles(self._h, C.c_void_p(gathered_ptr), num_ranks, max_tiles,
                                      width, height, C.c_void_p(fb_ptr), C.c_void_p(stream)),
               "irt_unpack_tiles")

    def stats(self) -> RenderStats:
        st = RenderStats()
        _check(lib().irt_get_render_stats(self._h, C.byref(st)), "irt_get_render_stats")
        return st

    def stats_total(self) -> tuple[RenderStats, int]:
        """Sums of the statistics of every launch since reset_stats_total()."""
        st = RenderStats()
        n = C.c_longlong()
        _check(lib().irt_get_render_stats_total(self._h, C.byref(st), C.byref(n)),
               "irt_get_render_stats_total")
        return st, n.value

    def reset_stats_total(self):
        _check(lib().irt_reset_render_stats_total(self._h), "irt_reset_render_stats_total")

    def set_timing_interval(self, every: int):
        """Kernel-timing events on every `every`-th launch only (default 8)."""
        _check(lib().irt_set_timing_interval(self._h, int(every)), "irt_set_timing_interval")

    def build_wedge_accel(self, cells: np.ndarray):
        """buildCuBQLAccel (hostCode.cu:557-649): enables LaunchParams.mode = MODE_CUBQL."""
        cells = np.ascontiguousarray(cells, dtype=CELL_DTYPE)
        _check(lib().irt_build_wedge_accel(self._h, _ptr(cells), cells.size),
               "irt_build_wedge_accel")

    def sample_points(self, xyz_ptr: int, n: int, value_ptr: int, found_ptr: int = 0,
                      mode: int = MODE_USER_GEOM, miss: float = float("nan"), stream: int = 0):
        """irt_sample_points: value[i] = the `mode` sampler's value at point i of n x 3 float32 in
        device memory at xyz_ptr, or `miss` where no cell holds it; found[i] = 1/0 (uint8;
        found_ptr 0: not written).  Device pointers, enqueued on `stream`."""
        _check(lib().irt_sample_points(self._h, int(mode), C.c_void_p(xyz_ptr), int(n),
                                       C.c_void_p(value_ptr), C.c_void_p(found_ptr), float(miss),
                                       C.c_void_p(stream)), "irt_sample_points")

    def sample_latlon(self, lat, lon, radius, value_ptr: int, found_ptr: int = 0,
                      mode: int = MODE_USER_GEOM, miss: float = float("nan"), stream: int = 0):
        """irt_sample_latlon: the same on the grid latlon_points(lat, lon, radius) (host arrays,
        radians and metres from the centre), value at [(k * len(lat) + j) * len(lon) + i] of the
        device arrays; no point array exists.  Returns the grid's shape (levels, lat, lon)."""
        lat, lon, radius = _latlon_arrays(lat, lon, radius)
        _check(lib().irt_sample_latlon(self._h, int(mode), _ptr(lat), lat.size, _ptr(lon), lon.size,
                                       _ptr(radius), radius.size, C.c_void_p(value_ptr),
                                       C.c_void_p(found_ptr), float(miss), C.c_void_p(stream)),
               "irt_sample_latlon")
        return radius.size, lat.size, lon.size

    def render_levels(self, lp: LaunchParams, width: int, height: int, radii, fb_ptr: int, accum_ptr: int,
                      value_ptr: int = 0, level_ptr: int = 0, back: bool = False,
                      miss: float = float("nan"), stream: int = 0):
        """irt_render_levels: the field on the spheres of `radii` (metres from the centre, any
        order, at most MAX_LEVELS) seen through lp's camera and the transfer function, composited
        front to back into fb / accum (device arrays of width * height, as render's); value_ptr
        (float32) and level_ptr (int32; an index into radii, or -1) take the first value found per
        pixel, 0: not written.  lp.mode chooses the sampler.  Enqueued on `stream`."""
        radii = levels_radii(radii)
        _check(lib().irt_render_levels(self._h, C.byref(lp), int(width), int(height), _ptr(radii), radii.size,
                                       LEVELS_BACK if back else 0, C.c_void_p(fb_ptr), C.c_void_p(accum_ptr),
                                       C.c_void_p(value_ptr), C.c_void_p(level_ptr), float(miss),
                                       C.c_void_p(stream)), "irt_render_levels")

    def column_latlon(self, lat, lon, radius, out: dict, weight=None, mode: int = MODE_USER_GEOM,
                      miss: float = float("nan"), stream: int = 0):
        """irt_column_latlon: the column reduction (column_reduce) over the levels `radius` of the grid
        sample_latlon samples, in one pass: `out` maps any of wsum, vmax, vmin (float32), kmax, kmin,
        count (int32) to a device pointer of len(lat) * len(lon) elements, column (j, i) at
        [j * len(lon) + i].  weight: None or one float per level.  Returns (lat, lon) sizes."""
        lat, lon, radius = _latlon_arrays(lat, lon, radius)
        w = _weights(weight, radius.size)
        unknown = set(out) - set(COLUMN_OUTPUTS)
        if unknown:
            raise IrtError(f"column_latlon: unknown outputs {sorted(unknown)}", E_INVALID)
        _check(lib().irt_column_latlon(self._h, int(mode), _ptr(lat), lat.size, _ptr(lon), lon.size, _ptr(radius),
                                       _ptr(w) if w is not None else None, radius.size,
                                       ColumnOut(**{k: int(v) or None for k, v in out.items()}), float(miss),
                                       C.c_void_p(stream)), "irt_column_latlon")
        return lat.size, lon.size

    def column(self, lat, lon, radius, weight=None, mode: int = MODE_USER_GEOM, miss: float = float("nan")) -> dict:
        """The column products on a lat x lon grid: a dict of torch tensors wsum, vmax, vmin
        (float32), kmax, kmin, count (int32) of shape (len(lat), len(lon)) on the context's device,
        computed on torch's current stream."""
        import torch
        dev = torch.device("cuda", self.device)
        shape = (np.size(lat), np.size(lon))
        with torch.cuda.device(dev):
            out = {k: torch.empty(shape, dtype=torch.float32 if t is np.float32 else torch.int32, device=dev)
                   for k, t in COLUMN_OUTPUTS.items()}
            self.column_latlon(lat, lon, radius, {k: t.data_ptr() for k, t in out.items()}, weight, mode, miss,
                               torch.cuda.current_stream(dev).cuda_stream)
        return out

    def render_column(self, lp: LaunchParams, width: int, height: int, surface_radius: float, radii, fb_ptr: int,
                      accum_ptr: int, value_ptr: int = 0, weight=None, product: int = COLUMN_WSUM,
                      miss: float = float("nan"), stream: int = 0):
        """irt_render_column: a column product (COLUMN_WSUM, COLUMN_MAX or COLUMN_MIN over the levels
        `radii`, any number of them) drawn on the sphere of surface_radius as lp's camera sees it,
        through the transfer function, into fb / accum (device arrays of width * height, as
        render_levels'); value_ptr (float32) takes the product per pixel, 0: not written.  lp.mode
        chooses the sampler.  Enqueued on `stream`."""
        radii = np.ascontiguousarray(radii, dtype=np.float32).reshape(-1)
        w = _weights(weight, radii.size)
        _check(lib().irt_render_column(self._h, C.byref(lp), int(width), int(height), float(surface_radius),
                                       _ptr(radii), _ptr(w) if w is not None else None, radii.size, int(product),
                                       C.c_void_p(fb_ptr), C.c_void_p(accum_ptr), C.c_void_p(value_ptr), float(miss),
                                       C.c_void_p(stream)), "irt_render_column")

    def section_raw(self, lat, lon, radius, out: dict, weight=None, ambient=(1.0, 1.0, 1.0), radiance: float = 1.0,
                    mode: int = MODE_USER_GEOM, miss: float = float("nan"), stream: int = 0):
        """irt_section: the field on the levels `radius` of the columns at the pairs (lat[c], lon[c])
        (host arrays, radians and metres from the centre), in one pass.  `out` maps any of value
        (float32), found (uint8), rgba (uint32; the curtain through the transfer function, ambient
        and radiance) -- device pointers of len(radius) * len(lat) elements, point (k, c) at
        [k * len(lat) + c] -- and of the column outputs wsum, vmax, vmin (float32), kmax, kmin,
        count (int32) -- len(lat) elements -- to a device pointer.  weight: None or one float per
        level.  Enqueued on `stream`.  Returns (levels, columns)."""
        lat, lon, radius = _section_arrays(lat, lon, radius)
        w = _weights(weight, radius.size)
        unknown = set(out) - set(SECTION_OUTPUTS) - set(COLUMN_OUTPUTS)
        if unknown:
            raise IrtError(f"section: unknown outputs {sorted(unknown)}", E_INVALID)
        o = SectionOut(column=ColumnOut(**{k: int(v) or None for k, v in out.items() if k in COLUMN_OUTPUTS}),
                       **{k: int(v) or None for k, v in out.items() if k in SECTION_OUTPUTS})
        _check(lib().irt_section(self._h, int(mode), _ptr(lat), _ptr(lon), lat.size, _ptr(radius),
                                 _ptr(w) if w is not None else None, radius.size, vec3(ambient), float(radiance), o,
                                 float(miss), C.c_void_p(stream)), "irt_section")
        return radius.size, lat.size

    def section(self, lat, lon, radius, weight=None, image: bool = False, columns: bool = False,
                ambient=(1.0, 1.0, 1.0), radiance: float = 1.0, mode: int = MODE_USER_GEOM,
                miss: float = float("nan")) -> dict:
        """The vertical cross-section along the pairs (lat[c], lon[c]) -- a great_circle track, a
        station list -- as a dict of torch tensors on the context's device, computed on torch's
        current stream: value (float32) and found (uint8) of shape (len(radius), len(lat)); with
        image=True also rgba (uint8, (len(radius), len(lat), 4): row k is level k, so flip it for a
        picture with the top level in the top row); with columns=True also wsum, vmax, vmin
        (float32), kmax, kmin, count (int32) of shape (len(lat),)."""
        import torch
        dev = torch.device("cuda", self.device)
        L, n = np.size(radius), np.size(lat)
        tt = {np.float32: torch.float32, np.uint8: torch.uint8, np.int32: torch.int32}
        with torch.cuda.device(dev):
            out = {"value": torch.empty((L, n), dtype=torch.float32, device=dev),
                   "found": torch.empty((L, n), dtype=torch.uint8, device=dev)}
            if image:
                out["rgba"] = torch.empty((L, n, 4), dtype=torch.uint8, device=dev)
            if columns:
                out.update({k: torch.empty((n,), dtype=tt[t], device=dev) for k, t in COLUMN_OUTPUTS.items()})
            self.section_raw(lat, lon, radius, {k: t.data_ptr() for k, t in out.items()}, weight, ambient, radiance,
                             mode, miss, torch.cuda.current_stream(dev).cuda_stream)
        return out

    def histogram_raw(self, value_range, bins: int, out: dict, weighting="count", band_edges=None, stream: int = 0):
        """irt_histogram: the histogram of the context's values (histogram_cells' definition) into the
        device pointers of `out` -- any of bins (bands * bins uint64), tails (bands * 3) and outside
        (1) --, overwritten, on `stream`.  Returns (bands, bins)."""
        w, e, bands = _hist_args(weighting, band_edges)
        unknown = set(out) - set(HISTOGRAM_OUTPUTS)
        if unknown:
            raise IrtError(f"histogram: unknown outputs {sorted(unknown)}", E_INVALID)
        o = HistogramOut(**{k: int(v) or None for k, v in out.items()})
        _check(lib().irt_histogram(self._h, box1(*value_range), int(bins), w, _ptr(e) if e is not None else None,
                                   bands, o, C.c_void_p(stream)), "irt_histogram")
        return bands, int(bins)

    def histogram(self, value_range=None, bins: int = 300, weighting="count", band_edges=None, stream: int = 0) -> dict:
        """The distribution of the field's values as the device holds them (every committed update
        included): a dict of int64 torch tensors on the context's device -- bins (bands, bins), tails
        (bands, 3: under, over, not finite), outside (1) -- holding the unsigned 64-bit counts of
        histogram_cells.  value_range None: the context's dataRange.  With bins = the transfer
        function's size, bin k is the LUT entry postClassify reads.  Enqueued on `stream`."""
        import torch
        dev = torch.device("cuda", self.device)
        if value_range is None:
            value_range = (self.info.dataRange.lower, self.info.dataRange.upper)
        _, _, bands = _hist_args(weighting, band_edges)
        with torch.cuda.device(dev):
            out = {"bins": torch.empty((bands, max(int(bins), 0)), dtype=torch.int64, device=dev),
                   "tails": torch.empty((bands, 3), dtype=torch.int64, device=dev),
                   "outside": torch.empty((1,), dtype=torch.int64, device=dev)}
            if stream == 0:  # the buffers were allocated on torch's current stream: stay behind it
                stream = torch.cuda.current_stream(dev).cuda_stream
            self.histogram_raw(value_range, bins, {k: t.data_ptr() for k, t in out.items()}, weighting, band_edges,
                               stream)
        return out

    def overlay(self, segments, styles, bins_per_edge: int = 0) -> "Overlay":
        """irt_overlay_create: the segments (overlay_segments, graticule; concatenate for several
        lines), their styles (overlay_styles' input) and the bin table on the device; bins_per_edge 0
        lets the library choose.  Returns an Overlay: close() it, or leave it to the context."""
        seg = _segments(segments)
        st, ns = overlay_styles(styles)
        h = C.c_void_p()
        _check(lib().irt_overlay_create(self._h, _ptr(seg), seg.size, st, ns, int(bins_per_edge), C.byref(h)),
               "irt_overlay_create")
        return Overlay(self, h, seg.size)

    def render_overlay(self, overlay: "Overlay", lp: LaunchParams, width: int, height: int, surface_radius: float,
                       cover_ptr: int, fb_ptr: int, accum_in_ptr: int = 0, segment_ptr: int = 0, over: bool = False,
                       stream: int = 0):
        """irt_render_overlay: the overlay's lines on the sphere of surface_radius as lp's camera sees
        it.  cover_ptr (float4 per pixel) holds the line layer, lerped with lp.accumID as a render
        call lerps accum; it must hold finite values before the first frame (clear it: the lerp forms
        0 * cover at accumID 0 too, and 0 * NaN is NaN for good); fb_ptr
        takes the composite of the layer with accum_in_ptr (a frame's accum, read only; 0: none),
        the lines under it or, over=True, on top; segment_ptr (int32; 0: not written) the segment
        under each pixel, -1 for none.  Enqueued on `stream`."""
        _check(lib().irt_render_overlay(self._h, overlay._h if overlay is not None else None, C.byref(lp), int(width),
                                        int(height), float(surface_radius), OVERLAY_OVER if over else 0,
                                        C.c_void_p(accum_in_ptr), C.c_void_p(cover_ptr), C.c_void_p(fb_ptr),
                                        C.c_void_p(segment_ptr), C.c_void_p(stream)), "irt_render_overlay")

    def contour_grid(self, value_ptr: int, found_ptr: int, lat, lon, thresholds, styles=None, out_ptr: int = 0,
                     capacity: int = 0, wrap: bool = False, stream: int = 0):
        """irt_contour_grid: the isolines of the device grid value_ptr (float32, len(lat) x len(lon))
        / found_ptr (uint8; 0: every point found) at `thresholds`, written to the device array out_ptr
        (64-byte aligned, `capacity` segments of SEGMENT_DTYPE) in the order of contour_cells, bit for
        bit.  out_ptr 0 only counts.  Synchronises `stream` to read the counts; the segments are then
        written in stream order.  Returns (count, counts per threshold int64); a refusal raises
        ContourError, whose count / counts hold what the library had set."""
        lat, lon, thr, sty = _contour_args(lat, lon, thresholds, styles)
        n, per = C.c_size_t(), np.zeros(CONTOUR_MAX_THRESHOLDS, np.uintp)
        _contour_check(lib().irt_contour_grid(self._h, C.c_void_p(value_ptr), C.c_void_p(found_ptr), _ptr(lat),
                                              lat.size, _ptr(lon), lon.size, _ptr(thr), _ptr(sty), thr.size,
                                              CONTOUR_WRAP if wrap else 0, C.c_void_p(out_ptr), int(capacity),
                                              C.byref(n), _ptr(per), C.c_void_p(stream)), "irt_contour_grid", n, per)
        return int(n.value), per[:thr.size].astype(np.int64)

    def contour_latlon(self, lat, lon, radius: float, thresholds, styles=None, out_ptr: int = 0, capacity: int = 0,
                       wrap: bool = False, mode: int = MODE_USER_GEOM, stream: int = 0):
        """irt_contour_latlon: sample_latlon of the one level `radius` into a grid the context owns,
        then contour_grid on it, on the same stream.  Returns (count, counts per threshold)."""
        lat, lon, thr, sty = _contour_args(lat, lon, thresholds, styles)
        n, per = C.c_size_t(), np.zeros(CONTOUR_MAX_THRESHOLDS, np.uintp)
        _contour_check(lib().irt_contour_latlon(self._h, int(mode), _ptr(lat), lat.size, _ptr(lon), lon.size,
                                                float(radius), _ptr(thr), _ptr(sty), thr.size,
                                                CONTOUR_WRAP if wrap else 0, C.c_void_p(out_ptr), int(capacity),
                                                C.byref(n), _ptr(per), C.c_void_p(stream)), "irt_contour_latlon",
                       n, per)
        return int(n.value), per[:thr.size].astype(np.int64)

    def contour_segments(self, lat, lon, thresholds, styles=None, value=None, found=None, radius=None,
                         wrap: bool = False, mode: int = MODE_USER_GEOM) -> np.ndarray:
        """The isolines as a host SEGMENT_DTYPE array, computed on the device on torch's current
        stream: of the torch tensors value / found (float32 / uint8, on the context's device) through
        contour_grid, or, with radius, of the field at that level through contour_latlon."""
        import torch
        dev = torch.device("cuda", self.device)
        if (value is None) == (radius is None):
            raise IrtError("contour_segments: give either value or radius", E_INVALID)
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev).cuda_stream
            if radius is None:
                if value.device != dev or value.dtype != torch.float32 or not value.is_contiguous():
                    raise IrtError(f"contour_segments: value must be contiguous float32 on {dev}", E_INVALID)
                if value.numel() != np.size(lat) * np.size(lon):
                    raise IrtError(f"contour_segments: value of {value.numel()} elements for a "
                                   f"{np.size(lat)} x {np.size(lon)} grid", E_INVALID)
                if found is not None and (found.device != dev or found.dtype != torch.uint8
                                          or not found.is_contiguous() or found.numel() != value.numel()):
                    raise IrtError(f"contour_segments: found must be contiguous uint8 on {dev}, as large as value",
                                   E_INVALID)
                call = lambda out, cap: self.contour_grid(  # noqa: E731
                    value.data_ptr(), found.data_ptr() if found is not None else 0, lat, lon, thresholds, styles,
                    out, cap, wrap, stream)
            else:
                call = lambda out, cap: self.contour_latlon(  # noqa: E731
                    lat, lon, radius, thresholds, styles, out, cap, wrap, mode, stream)
            n, _ = call(0, 0)
            # (torch's allocations are 512-byte aligned: the 64-byte lines the kernel writes)
            out = torch.empty((max(n, 1), SEGMENT_DTYPE.itemsize), dtype=torch.uint8, device=dev)
            if n:
                call(out.data_ptr(), n)
            host = out[:n].cpu().numpy()
        return host.reshape(-1).view(SEGMENT_DTYPE).copy()

    def contour_overlay(self, lat, lon, thresholds, styles, bins: int = 0, style_index=None, value=None,
                        found=None, radius=None, wrap: bool = False, mode: int = MODE_USER_GEOM) -> "Overlay":
        """A convenience: contour_segments (the device passes), copied back, as an overlay of this
        context drawn in `styles` (overlay_styles' input); style_index: the style per threshold (None:
        threshold k in style k modulo len(styles)); bins: the overlay's bins per edge (0: the
        library's choice).  The returned Overlay's `segments` holds the host copy."""
        styles = list(styles)
        if style_index is None:
            style_index = np.arange(np.size(thresholds)) % max(len(styles), 1)
        seg = self.contour_segments(lat, lon, thresholds, style_index, value, found, radius, wrap, mode)
        ov = self.overlay(seg, styles, bins)
        ov.segments = seg
        return ov

    def resample(self, points, mode: int = MODE_USER_GEOM, miss: float = float("nan")):
        """The field at `points` (..., 3): a float32 torch tensor on the context's device (sampled
        in place, on torch's current stream) or a numpy array (which goes up and comes back).
        Returns (value float32, found bool) of shape points.shape[:-1], of the same kind."""
        import torch
        dev = torch.device("cuda", self.device)
        host = not isinstance(points, torch.Tensor)
        pts = torch.from_numpy(np.array(points, dtype=np.float32, order="C")).to(dev) if host else points
        if pts.device != dev or pts.dtype != torch.float32 or pts.shape[-1] != 3:
            raise IrtError(f"resample: points must be float32 (..., 3) on {dev}, got {pts.dtype} "
                           f"{tuple(pts.shape)} on {pts.device}")
        with torch.cuda.device(dev):
            pts = pts.contiguous()
            value = torch.empty(pts.shape[:-1], dtype=torch.float32, device=dev)
            found = torch.empty(pts.shape[:-1], dtype=torch.uint8, device=dev)
            self.sample_points(pts.data_ptr(), value.numel(), value.data_ptr(), found.data_ptr(), mode,
                               miss, torch.cuda.current_stream(dev).cuda_stream)
            if host:
                return value.cpu().numpy(), found.cpu().numpy().astype(bool)
        return value, found.bool()

    def locate_sampler(self, points: np.ndarray, mode: int) -> tuple[np.ndarray, np.ndarray]:
        """irt_debug_locate_sampler: the device point location of the MODE_CUBQL or
        MODE_TRIANGLES sampler at points (n, 3); returns (found int32, value float32, 0 on a
        miss).  Needs build_wedge_accel first."""
        pts = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
        found = np.zeros(len(pts), np.int32)
        value = np.zeros(len(pts), np.float32)
        L = lib()
        L.irt_debug_locate_sampler.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p,
                                               C.c_void_p]
        _check(L.irt_debug_locate_sampler(self._h, int(mode), _ptr(pts), len(pts), _ptr(found),
                                          _ptr(value)), "irt_debug_locate_sampler")
        return found, value

    def debug_classify(self, values: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
        """irt_debug_classify: the kernels' post_classify (n, 4) and classify_alpha (n,) of `values`
        under the current transfer function."""
        v = np.ascontiguousarray(values, dtype=np.float32).ravel()
        out = np.zeros((v.size, 4), np.float32)
        alpha = np.zeros(v.size, np.float32)
        L = lib()
        L.irt_debug_classify.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        _check(L.irt_debug_classify(self._h, _ptr(v), v.size, _ptr(out), _ptr(alpha)), "irt_debug_classify")
        return out, alpha

    def grid(self) -> tuple[np.ndarray, np.ndarray]:
        """GRID_ACCEL_MODE grid: (valueRanges (256^3, 2), maxOpacities (256^3,))."""
        n = 256 ** 3
        vr = np.zeros((n, 2), np.float32)
        mo = np.zeros(n, np.float32)
        _check(lib().irt_get_grid(self._h, _ptr(vr), _ptr(mo)), "irt_get_grid")
        return vr, mo

    def shell(self) -> tuple[np.ndarray, np.ndarray]:
        n = int(np.prod(list(self.info.shellDims)))
        vr = np.zeros((n, 2), dtype=np.float32)
        mo = np.zeros(n, dtype=np.float32)
        _check(lib().irt_get_shell(self._h, _ptr(vr), _ptr(mo)), "irt_get_shell")
        return vr, mo


class Overlay:
    """A device overlay of one Context (irt_overlay_create ... irt_overlay_destroy)."""

    def __init__(self, ctx: Context, handle, num_segments: int):
        self._ctx, self._h, self.num_segments = ctx, handle, int(num_segments)

    def bins(self) -> tuple:
        """irt_overlay_get_bins: (bins per edge, list entries) of the overlay's bin table."""
        n, e = C.c_int(), C.c_size_t()
        _check(lib().irt_overlay_get_bins(self._ctx._h, self._h, C.byref(n), C.byref(e)), "irt_overlay_get_bins")
        return n.value, e.value

    def close(self):
        """irt_overlay_destroy (waits for the sampling calls issued so far); a context that was
        closed first has freed it already."""
        if self._h is not None and getattr(self._ctx, "_h", None):
            _check(lib().irt_overlay_destroy(self._ctx._h, self._h), "irt_overlay_destroy")
        self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


class DebugScene:
    """Host-side locator (include/icon_rt_hip_debug.h), for CPU checks."""

    def __init__(self, cells: np.ndarray):
        cells = np.ascontiguousarray(cells, dtype=CELL_DTYPE)
        h = C.c_void_p()
        _check(lib().irt_debug_scene_build(_ptr(cells), cells.size, C.byref(h)),
               "irt_debug_scene_build")
        self._h = h
        self.info = VolumeInfo()
        lib().irt_debug_scene_info(self._h, C.byref(self.info))

    def locate(self, p):
        v = C.c_float()
        r = C.c_uint32()
        hit = lib().irt_debug_scene_locate(self._h, vec3(p), C.byref(v), C.byref(r))
        return (True, v.value, r.value) if hit == 1 else (False, 0.0, None)

    def locate_binned(self, p):
        """locate() through the binned locator of the render kernel; also returns the
        number of candidate entries examined."""
        v = C.c_float()
        r = C.c_uint32()
        t = C.c_uint32()
        hit = lib().irt_debug_scene_locate_binned(self._h, vec3(p), C.byref(v), C.byref(r),
                                                  C.byref(t))
        return (True, v.value, r.value, t.value) if hit == 1 else (False, 0.0, None, t.value)

    def candidates(self, p):
        n = lib().irt_debug_scene_candidates(self._h, vec3(p), None, 0)
        out = np.zeros(max(n, 1), dtype=np.uint32)
        lib().irt_debug_scene_candidates(self._h, vec3(p), _ptr(out), n)
        return out[:n]

    def values(self, rec: int, r: float):
        """(literal findHeight value, render-record value) of record `rec` at radius r."""
        out = np.zeros(2, dtype=np.float32)
        _check(lib().irt_debug_scene_values(self._h, rec, C.c_float(r), _ptr(out)),
               "irt_debug_scene_values")
        return out

    def array(self, name: str) -> np.ndarray:
        """A scene array as the host restatement built it (bytes)."""
        return _array(lib().irt_debug_scene_array, self._h, name)

    def planes(self, rec: int) -> np.ndarray:
        out = np.zeros(12, dtype=np.float32)
        _check(lib().irt_debug_scene_planes(self._h, rec, _ptr(out)), "irt_debug_scene_planes")
        return out.reshape(3, 4)

    def close(self):
        if getattr(self, "_h", None):
            lib().irt_debug_scene_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
