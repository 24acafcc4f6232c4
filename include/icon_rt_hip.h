/*
 * icon_rt_hip.h -- C ABI of the MI355X-native ICON volume renderer.
 *
 * Drop-in boundary for the hot path of szellmann/icon-ray-tracing `icon_rt`:
 * the reference renders one frame with
 *     SET_LAUNCH_PARAMS(parms); pl.launch();            (icon_rt/hostCode.cu:961-963)
 * which runs the raygen `woodcockTrackingWithAccel` (icon_rt/deviceCode.cu:281-341)
 * once per pixel -- on the CPU through parallel::for_each (common/pipeline.cu:1066-1071),
 * on NVIDIA through owlLaunch2D (common/pipeline.cu:1064).  This library replaces that
 * launch (and the accelerator builds that feed it) with hand-written HIP kernels for
 * gfx950.  Plain C types, plain pointers and sizes; no C++ or torch types.
 *
 * Conventions
 *  - Every function returns IRT_OK (0) or a negative IRT_E_* code; irt_last_error()
 *    returns a thread-local message for the last failure.  (The reference prints and
 *    continues or abort()s; pipeline.cu:992-995, hostCode.cu:19-34.)
 *  - Input arrays are copied; the context never retains caller pointers beyond a call
 *    (the reference's LaunchParams borrow pointers owned by Buffer/Frame/Transfunc).
 *  - Framebuffer pointers passed to irt_render* are DEVICE pointers on the context's
 *    device (HBM-resident, as the reference's fbPointer/accumBuffer in RTCORE builds).
 *  - `stream` is a hipStream_t passed as void*; NULL is HIP's null (legacy default) stream,
 *    so work launched there is ordered with every blocking stream of the process (torch's
 *    default stream included).
 *  - A context is single-caller.  Multi-GPU = one process (one context) per GPU.
 *  - Launches of one context execute in call order, whatever streams they are given: a call
 *    on another stream than the previous call's makes its stream wait for the previous launch
 *    first (the reference has one launch stream per pipeline, pipeline.cu:1064).
 */
#ifndef ICON_RT_HIP_H
#define ICON_RT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define IRT_OK 0
#define IRT_E_INVALID (-1)   /* bad argument */
#define IRT_E_HIP (-2)       /* HIP runtime error (no device, OOM, launch failure) */
#define IRT_E_DATA (-3)      /* unusable cell data (numLayers out of [0,31], non-finite) */
#define IRT_E_IO (-4)        /* file I/O */
#define IRT_E_CHAIN (-5)     /* a chained multi-frame launch's per-pixel hand-off timed out: that
                                launch's frames were lerped out of order (see
                                irt_render_accumulate) */

/* == icon_rt::ICONCell (icon_rt/ICONGrid.h:59-76); 284 bytes; the `.ic` record. */
typedef struct irt_icon_cell {
  float lat[3];        /* radians, per triangle corner, ccw */
  float lon[3];        /* radians */
  int32_t numLayers;   /* <= 31 (MAX_LAYERS 32, ICONGrid.h:57) */
  float height[32];    /* metres from the Earth centre, [0:numLayers] used */
  float value[32];     /* per layer, [0:numLayers) used */
} irt_icon_cell;

typedef struct irt_vec3f { float x, y, z; } irt_vec3f;
typedef struct irt_vec4f { float x, y, z, w; } irt_vec4f;
typedef struct irt_box1f { float lower, upper; } irt_box1f;
typedef struct irt_box3f { irt_vec3f lower, upper; } irt_box3f;

/* Raygen selector == Pipeline::setRayGen(...) choice (hostCode.cu:138-149, 863). */
#define IRT_RAYGEN_WITH_ACCEL 0 /* woodcockTrackingWithAccel, deviceCode.cu:281-341 */
#define IRT_RAYGEN_AE 1         /* woodcockTrackingAE, deviceCode.cu:239-275 */
#define IRT_ACCEL_SPHERE 0      /* SPHERE_ACCEL_MODE (Params.h:33): sdda, ShellAccel.h:82-229 */
#define IRT_ACCEL_GRID 1        /* GRID_ACCEL_MODE (Params.h:34): dda3, DDA.h:35-136 */
/* Sampler == Volume::mode (Params.h:29-31, 60; the -mode flag, hostCode.cu:125-127). */
#define IRT_MODE_USER_GEOM 0    /* sample() on the cells (ICONGrid.h:181-208): the CPU build's
                                   scan (deviceCode.cu:116-123), lowest index wins */
#define IRT_MODE_TRIANGLES 1    /* the OptiX triangle trace (deviceCode.cu:61-76): closest
                                   bottom triangle toward the Earth's centre (needs
                                   irt_build_wedge_accel); OptiX's own intersection test is
                                   not reproducible, see ray_triangle in csrc/irt_common.h */
#define IRT_MODE_CUBQL 2        /* wedges + intersectWedgeEXT (deviceCode.cu:90-115) */

/* Per-frame part of icon_rt::LaunchParams (icon_rt/Params.h:92-119).  The volume,
 * accelerator and transfer-function members live in the context (set by irt_create /
 * irt_set_transfunc); the framebuffer pointers are arguments of irt_render. */
typedef struct irt_launch_params {
  irt_vec3f org;            /* camera.org    (Params.h:101; hostCode.cu:942) */
  irt_vec3f dir_00;         /* camera.dir_00 (Params.h:102; hostCode.cu:943) */
  irt_vec3f dir_du;         /* camera.dir_du (Params.h:103; hostCode.cu:944) */
  irt_vec3f dir_dv;         /* camera.dir_dv (Params.h:104; hostCode.cu:945) */
  int32_t accumID;          /* Params.h:111; hostCode.cu:958 */
  irt_vec3f ambientColor;   /* Params.h:114; hostCode.cu:925 */
  float ambientRadiance;    /* Params.h:115; hostCode.cu:926 */
  float unitDistance;       /* Params.h:118; hostCode.cu:956 */
  int32_t raygen;           /* IRT_RAYGEN_* */
  int32_t accelMode;        /* volume.accelMode (Params.h:33-34; hostCode.cu:170-200, the
                               "Accel mode" UI option 853-857): IRT_ACCEL_SPHERE (sdda over
                               the shell grid, the default) or IRT_ACCEL_GRID (dda3 over the
                               256^3 Cartesian grid) */
  int32_t mode;             /* volume.mode: IRT_MODE_USER_GEOM (default), IRT_MODE_TRIANGLES
                               or IRT_MODE_CUBQL (both need irt_build_wedge_accel) */
} irt_launch_params;

/* Scene facts computed at irt_create exactly as hostCode.cu:792-808, 838-840. */
typedef struct irt_volume_info {
  uint64_t numCells;            /* Volume::numCells (Params.h:63) */
  irt_box3f bounds;             /* Volume::bounds = union of ICONCell::getBounds() */
  irt_box3f sphericalBounds;    /* ShellAccel::sphericalBounds (r, lat, lon) */
  irt_box1f dataRange;          /* min/max of value[0:numLayers) */
  float unitDistance;           /* 10^(floor(log10(sphericalBounds.lower.x))-3) */
  int32_t shellDims[3];         /* ShellAccel::dims = (1,1024,1024) (hostCode.cu:654) */
  /* locator facts (MI355X point-location structure replacing OptiX/cuBQL) */
  int32_t locatorFaceRes;       /* cube-map cells per face edge */
  uint64_t locatorEntries;      /* candidate-list entries */
  uint64_t deviceBytes;         /* HBM held by the context */
} irt_volume_info;

/* Statistics of the most recent irt_render* call on a context. */
typedef struct irt_render_stats {
  uint64_t raysLaunched;        /* pixels the raygen ran for */
  uint64_t raysInBox;           /* rays that passed boxTest (deviceCode.cu:294) */
  uint64_t locateCalls;         /* sampleVolume calls (deviceCode.cu:173) */
  uint64_t samplesFound;        /* sampleVolume calls that found a cell */
  uint64_t candidatesTested;    /* locator candidate-list entries examined */
  float kernelMs;               /* render kernel time, HIP events on the launch stream
                                   (most recent timed launch, irt_set_timing_interval) */
} irt_render_stats;

typedef struct irt_context irt_context;

/* ---------------------------------------------------------------- errors */
const char *irt_last_error(void);

/* ---------------------------------------------------------------- context
 * irt_create: validate and copy `cells` (already lat/lon-filtered, see irt_filter_cells),
 * compute the volume facts (hostCode.cu:792-808), build the cell locator that replaces the
 * OptiX/cuBQL accelerators (hostCode.cu:440-650), upload to HBM on `device`, and build the
 * spherical-shell accelerator on the GPU: initGrid + buildShell_ICON
 * (hostCode.cu:216-225, 299-336, 652-666).  Majorants stay zero until irt_set_transfunc.
 * Everything but the per-record glibc corner trig (toCartesian's cosf/sinf) is built on
 * the device.  irt_create = irt_create_begin + irt_create_append(all) + irt_create_end. */
int irt_create(const irt_icon_cell *cells, size_t numCells, int device, irt_context **out);

/* Streaming creation, for scenes larger than host memory should hold at once (the cells
 * go to HBM chunk by chunk, host memory stays at one chunk): `numCells` records arrive
 * through any number of irt_create_append calls, in record order; irt_create_end builds
 * the scene on the device.  The context is unusable (and irt_create_end fails) unless
 * exactly numCells records were appended. */
int irt_create_begin(size_t numCells, int device, irt_context **out);
int irt_create_append(irt_context *ctx, const irt_icon_cell *cells, size_t n);
int irt_create_end(irt_context *ctx);

/* The load of hostCode.cu:717-734 streamed straight into a context: records of the `.ic`
 * file (N = filesize / 284, truncated to maxNumCells when >= 0, `--num-cells`). */
int irt_create_from_file(const char *path, long maxNumCells, int device, irt_context **out);

/* A synthetic RnBk grid (irt_synth_grid) generated chunk by chunk straight into a context. */
int irt_create_synth(int rootN, int bisections, int levels, float topHeight, float noise,
                     uint32_t seed, int device, irt_context **out);
/* ... with terrain (irt_synth_grid_terrain). */
int irt_create_synth_terrain(int rootN, int bisections, int levels, float topHeight, float noise,
                             uint32_t seed, float terrainHeight, int device, irt_context **out);
void irt_destroy(irt_context *ctx);
int irt_get_volume_info(const irt_context *ctx, irt_volume_info *info);

/* == Pipeline::setTransfunc -> transfuncUpdateHandler -> computeMaxOpacities
 * (pipeline.cu:456-478; hostCode.cu:878-909, 362-397).  `rgbaLUT` is the final LUT
 * (the reference resamples to 300 entries first when size < 300; irt_resample_lut). */
int irt_set_transfunc(irt_context *ctx, const irt_vec4f *rgbaLUT, int size,
                      irt_box1f valueRange, float opacityScale);

/* ---------------------------------------------------------------- time series
 * The next output step of a time series: the same records with new value[] (the mesh, the
 * heights and numLayers stay).  Only the value halves of the per-record blocks, the shell's
 * value ranges and majorants, the GRID_ACCEL_MODE grid (if built), dataRange and the sparse
 * transfer-function decision depend on value[]; the locator, the sphere tables and the wedge
 * locator are kept.  No counterpart in the reference, whose viewer loads one `.ic`.
 *
 * New values for records [first, first + n): values[k*32 + j] replaces record first+k's
 * value[j] for all 32 j (as irt_create stores all 32).  Host pointer; copied; returns once
 * the copy has been issued.  Any number of calls, in any order, until irt_update_values_end;
 * calls that overlap apply in call order.
 *  - Ordering: an update waits for every launch of the context already issued (as
 *    irt_set_transfunc does); irt_render* calls after irt_update_values_end, on any stream, see
 *    the committed values.
 *  - Between the first irt_update_values* and irt_update_values_end, every irt_render* call,
 *    irt_get_shell, irt_get_grid and irt_set_transfunc returns IRT_E_INVALID (the accelerators
 *    are stale); irt_last_error() names the pending update.
 *  - first + n > numCells, a NULL pointer with n > 0, a context still being created or a NULL
 *    context: IRT_E_INVALID, nothing written.
 *  - The values are not validated (irt_create validates none either); NaNs behave as through
 *    irt_create: the shell's min/max never store them, the data range skips them.
 *  - Multi-GPU: every rank's context holds the whole scene, so every rank updates its own. */
int irt_update_values(irt_context *ctx, size_t first, size_t n, const float *values);
/* The same from a DEVICE pointer on the context's device, enqueued on `stream`
 * (e.g. a torch tensor's data_ptr()); d_values must stay valid until the work on `stream`
 * has run. */
int irt_update_values_device(irt_context *ctx, size_t first, size_t n, const float *d_values,
                             void *stream);
/* Commit: rebuild what depends on the values -- the shell's valueRanges from ALL records,
 * info.dataRange, the majorants for the current transfer function (if one is set), the
 * 256^3 grid and its majorants/bits (if built), the sparse-TF decision (as irt_set_transfunc
 * makes it).  After it the context is indistinguishable from one created from the same
 * records with the new values: of irt_volume_info only dataRange changes (where the new
 * minimum or maximum is a zero, with the sign irt_compute_volume_info's fold gives it); the
 * transfer function's valueRange is the caller's and stays.  Waits for the rebuild.  With
 * nothing pending: IRT_OK, nothing done. */
int irt_update_values_end(irt_context *ctx);

/* ---------------------------------------------------------------- resampling
 * The field's value at points, or on a regular lat x lon x level grid, through the raygen's own
 * point location: sampleVolume (deviceCode.cu:58-125) of the chosen sampler without a ray around
 * it.  No counterpart in the reference, whose only consumer of sampleVolume is the raygen.
 *  - mode: IRT_MODE_USER_GEOM, IRT_MODE_CUBQL or IRT_MODE_TRIANGLES; the last two need
 *    irt_build_wedge_accel (IRT_E_INVALID without it).
 *  - d_xyz, d_value, d_found: DEVICE pointers on the context's device, used on `stream`; they must
 *    stay valid until that work has run.  d_found may be NULL.
 *  - Points that are never located (a miss, found = 0): a point with a non-finite coordinate (a
 *    documented deviation: the reference's sample() has no defined answer for NaN), and a point
 *    whose float squared length x*x + y*y + z*z is not finite and positive (the reference's own
 *    answer on every scene whose heights are positive: len < height[0] or len > height[n]).
 *  - Ordering: a sampling call counts as a launch of the context for everything that waits for
 *    every launch already issued (irt_update_values*, irt_set_transfunc, irt_destroy); sampling
 *    calls after irt_update_values_end see the committed values; between the first
 *    irt_update_values* and irt_update_values_end they return IRT_E_INVALID as irt_render does.
 *    They touch neither the render statistics nor fb/accum, and neither report nor consume
 *    IRT_E_CHAIN.  Sampling calls of one context run in call order, whatever their streams.
 *  - IRT_E_INVALID, nothing written: a NULL or still-building context, a bad mode, NULL d_xyz or
 *    d_value with points to sample, a negative count, more than 2^36 points.  Zero points:
 *    IRT_OK, nothing launched.
 *  - No record index is returned (the raygen's locator yields none).
 *
 * value[i] = the sampler's value at point i (xyz[3i .. 3i+2]) or missValue where no cell holds
 * it; found[i] = 1/0. */
int irt_sample_points(irt_context *ctx, int mode, const float *d_xyz, size_t n, float *d_value,
                      uint8_t *d_found, float missValue, void *stream);
/* The regular grid: point (k, j, i) = toCartesian(radius[k], lat[j], lon[i]) (ICONGrid.h:44-54:
 * x = (r cos lat) cos lon, y = (r cos lat) sin lon, z = r sin lat, cosf/sinf from the host's
 * glibc once per row and per column, so every point has the bits of the reference's
 * toCartesian), its value at d_value[(k*numLat + j)*numLon + i].  lat/lon in radians, radius in
 * metres from the Earth's centre; HOST arrays, copied before the call returns.  Equal, bit for
 * bit, to irt_sample_points on irt_latlon_points' output. */
int irt_sample_latlon(irt_context *ctx, int mode, const float *lat, int numLat, const float *lon,
                      int numLon, const float *radius, int numLevels, float *d_value,
                      uint8_t *d_found, float missValue, void *stream);
/* Host helper, no GPU: the points irt_sample_latlon samples, xyz[3*((k*numLat + j)*numLon + i) ...]. */
int irt_latlon_points(const float *lat, int numLat, const float *lon, int numLon,
                      const float *radius, int numLevels, float *xyz);

/* ---------------------------------------------------------------- level surfaces
 * The field on spheres of given radii ("the variable at 5 km"), seen from the camera through the
 * transfer function: per pixel the raygen's own ray, its hits with the spheres, the field's value
 * at each hit through the point location of irt_sample_points, classified and composited front to
 * back.  Deterministic apart from the anti-aliasing jitter: one frame is the picture.  No
 * counterpart in the reference.
 *  - radius: HOST array of numLevels radii in metres from the Earth's centre, in any order,
 *    copied before the call returns.  d_fb / d_accum: device arrays of width*height as for
 *    irt_render; d_value / d_level: device arrays of width*height, either may be NULL.  Of lp the
 *    call uses the camera, accumID, ambientColor, ambientRadiance and mode (the sampler, as in
 *    irt_sample_points); it ignores raygen, accelMode and unitDistance.
 *  - The ray of pixel (x, y) is the raygen's (generateRay, deviceCode.cu:36-49, with Random
 *    rnd(accumID*W*H + x, y), 288-291), tmin = 0: a level frame lines up with an irt_render frame
 *    of the same lp pixel for pixel.
 *  - Hit slots.  near[] = the level indices by descending radius, ties by ascending index; far[] =
 *    near[] reversed.  Slot h < numLevels is the near hit tn of intersectSphere(ray,
 *    radius[near[h]]) (ShellAccel.h:34-53), live when the sphere is hit and tn > 0.  Slot
 *    numLevels + h is the far hit tf of radius[far[h]], live when the sphere is hit, tf > 0 and
 *    either IRT_LEVELS_BACK is set or that sphere's near slot is not live (the camera is inside
 *    it).  Slot order is the compositing order: front to back for any camera, no sort by t.
 *  - A live slot's point P = org + dir * t (each component o + d * t in float) is sampled exactly
 *    as a point of irt_sample_points.  A found value v gives s = postClassify(v)
 *    (deviceCode.cu:127-135) with the context's transfer function, a = clamp(s.w, 0, 1), c =
 *    (s.rgb * ambientColor) * ambientRadiance, and then, in float, w = (1 - A) * a; C += w * c
 *    (per component); A += w; C and A start at 0.
 *  - Every pixel of the frame is written (no box test: unlike irt_render no pixel is left
 *    untouched): (C, A) is lerped into accum with 1/(accumID+1) and fb =
 *    make_rgba(linear_to_srgb(accum)) (deviceCode.cu:333-340); a ray that finds nothing lerps
 *    (0, 0, 0, 0).
 *  - d_value[p] = the value found at the first slot, in slot order, that found one, or
 *    missValue; d_level[p] = that slot's index into the caller's radius, or -1.
 *  - Non-finite values are outside the contract, as they are for frames: they classify as the
 *    device's post_classify happens to.
 *  - Ordering: a sampling call, not a launch of the ring.  It counts for everything that waits
 *    for every launch already issued (irt_update_values*, irt_set_transfunc, irt_destroy), runs
 *    after earlier sampling calls whatever their streams, touches no render statistics and
 *    neither reports nor consumes IRT_E_CHAIN.  Against irt_render* calls that use the same
 *    d_fb / d_accum it is ordered ONLY by its stream: put both on one stream, or synchronise.
 *  - IRT_E_INVALID, nothing written: a NULL or still-building context; a pending
 *    irt_update_values*; no transfer function set; a bad lp->mode, or a wedge or triangle mode
 *    without irt_build_wedge_accel; numLevels outside [1, IRT_MAX_LEVELS]; a radius that is not
 *    finite and positive; unknown flag bits; width or height < 1, or 2^27 pixels or more; NULL
 *    lp, radius, d_fb or d_accum.
 * The tile forms, multi-GPU splitting and several frames per launch have no level form. */
#define IRT_MAX_LEVELS 16
#define IRT_LEVELS_BACK 1   /* also the far-side hits of spheres the camera is outside of */
int irt_render_levels(irt_context *ctx, const irt_launch_params *lp, int width, int height,
                      const float *radius, int numLevels, int flags,
                      uint32_t *d_fb, irt_vec4f *d_accum,
                      float *d_value, int32_t *d_level, float missValue, void *stream);
/* Host helper, no GPU: the near[] order irt_render_levels gives numLevels radii -- sorted[h] =
 * radius[index[h]], descending, ties by ascending index.  IRT_E_INVALID for numLevels outside
 * [1, IRT_MAX_LEVELS], a radius that is not finite and positive, or a NULL pointer. */
int irt_levels_order(const float *radius, int numLevels, float *sorted, int32_t *index);

/* ---------------------------------------------------------------- column products
 * A reduction over the vertical of the field sampled on a column's levels: the weighted sum
 * ("total column X"), the maximum and the minimum with the levels they sit at, and how many of the
 * levels hold data -- on a lat x lon grid (irt_column_latlon) and on the globe as the camera sees
 * it (irt_render_column).  One pass on the device: the numLevels values per column that
 * irt_sample_latlon would write never reach memory.  No counterpart in the reference.
 *
 * The reduction of one column walks the levels k = 0 .. numLevels-1 in ascending order and skips a
 * level that was not found.  At the first found level, with value v: mn = mx = v, kmin = kmax = k,
 * wsum = weight[k] * v.  At each later found level: if (v < mn) { mn = v; kmin = k; } if (v > mx)
 * { mx = v; kmax = k; } wsum = wsum + weight[k] * v.  count++ at every found level.  The
 * comparisons are strict: a tie keeps the lower k, a NaN never replaces a value.  Everything is
 * float, one multiply then one add, never an fma.  weight == NULL: every weight is 1.0f (1.0f * v is
 * v, so wsum is the plain sequential sum).  A column with count == 0 has wsum = vmax = vmin =
 * missValue and kmax = kmin = -1. */
typedef struct irt_column_out {      /* every pointer may be NULL: that output is not written */
  float   *wsum;    /* sum over found levels of weight[k] * value, in level order */
  float   *vmax, *vmin;
  int32_t *kmax, *kmin;   /* level index of the max / min, or -1 */
  int32_t *count;         /* found levels */
} irt_column_out;
/* Host helper, no GPU: the reduction above of numColumns columns whose level k is at value / found
 * [k * numColumns + c] (the layout irt_sample_latlon writes, with numColumns = numLat * numLon);
 * out's arrays hold numColumns elements.  IRT_E_INVALID for numLevels < 1, and for a NULL value or
 * found with columns to reduce. */
int irt_column_reduce(const float *value, const uint8_t *found, int numLevels, size_t numColumns,
                      const float *weight, float missValue, irt_column_out out);
/* The reduction on the grid of irt_sample_latlon: point (k, j, i) is exactly irt_sample_latlon's
 * point (k, j, i) for the same lat, lon and radius, and column (j, i) writes its results at
 * [j*numLon + i] of the DEVICE arrays in d_out.  Equal, bit for bit, to irt_column_reduce applied to
 * irt_sample_latlon's output for the same arguments, for every sampler.
 *  - lat, lon, radius, weight: HOST arrays, copied before the call returns; weight is NULL or
 *    numLevels floats.  The radii may come in any order and may repeat: k is the caller's index,
 *    and the sum runs in that order.
 *  - A sampling call in every respect of "resampling" above: mode, ordering, no statistics, no
 *    IRT_E_CHAIN.
 *  - IRT_E_INVALID, nothing written: what irt_sample_latlon refuses for these arguments, and a
 *    weight that is not finite.  A grid without points (a zero count), or a d_out whose pointers
 *    are all NULL: IRT_OK, nothing launched. */
int irt_column_latlon(irt_context *ctx, int mode, const float *lat, int numLat, const float *lon,
                      int numLon, const float *radius, const float *weight, int numLevels,
                      irt_column_out d_out, float missValue, void *stream);
/* The product on the globe: the shell is ~75 km thick on a 6,371 km globe, so a column product
 * mapped onto a sphere is the readable 2-D view of the volume.  Per pixel:
 *  - the ray and the single hit slot of irt_render_levels with the one level surfaceRadius and
 *    flags 0: the near hit when tn > 0, else the far hit when tf > 0 (the camera is inside);
 *  - with P = org + dir * t: len = sqrtf(P.x*P.x + P.y*P.y + P.z*P.z), summed left to right, and the
 *    column point of level k is (P.x*s, P.y*s, P.z*s) with s = radius[k] / len, sampled exactly as
 *    a point of irt_sample_points;
 *  - the reduction above; v = the chosen product (wsum, vmax or vmin);
 *  - a pixel with count > 0: s4 = postClassify(v), a = clamp(s4.w, 0, 1), C = a * ((s4.rgb *
 *    ambientColor) * ambientRadiance), A = a.  A pixel without a live hit, or with count == 0: C =
 *    A = 0 and v = missValue;
 *  - (C, A) is lerped into accum and fb written as irt_render_levels writes every pixel; d_value[p]
 *    = v (d_value may be NULL).
 * Of lp the call uses what irt_render_levels uses.  Ordering: as irt_render_levels (a sampling
 * call; against irt_render* on the same d_fb / d_accum ordered only by its stream).
 * IRT_E_INVALID, nothing written: what irt_render_levels refuses (numLevels < 1 in place of its
 * range: there is no upper limit here), a surfaceRadius that is not finite and positive, a product
 * that is none of the three, a weight that is not finite.
 * The tile forms, multi-GPU splitting and several frames per launch have no column form. */
#define IRT_COLUMN_WSUM 0
#define IRT_COLUMN_MAX 1
#define IRT_COLUMN_MIN 2
int irt_render_column(irt_context *ctx, const irt_launch_params *lp, int width, int height,
                      float surfaceRadius, const float *radius, const float *weight, int numLevels,
                      int product, uint32_t *d_fb, irt_vec4f *d_accum, float *d_value,
                      float missValue, void *stream);

/* ---------------------------------------------------------------- sections
 * The vertical cross-section ("curtain") along a track, and profiles and column products at station
 * lists and flight or satellite tracks: the field on numLevels levels of numColumns columns at
 * arbitrary (lat, lon) pairs, in one pass on the device.  The shell is a few pixels thick in a frame
 * of the globe, so a curtain is an image of its own: distance along the track on one axis, the
 * level on the other.  No counterpart in the reference.
 *  - lat, lon (numColumns each, radians), radius (numLevels, metres from the Earth's centre) and
 *    weight (numLevels, or NULL: every weight 1.0f) are HOST arrays, copied before the call
 *    returns.  Column c is the pair (lat[c], lon[c]); pairs come in any order and may repeat, and so
 *    may the radii.
 *  - Point (k, c) = toCartesian(radius[k], lat[c], lon[c]) (ICONGrid.h:44-54) with cosf/sinf from the
 *    host's glibc once per column: the bits irt_latlon_points gives a grid point of the same three
 *    numbers.  irt_section_points writes that point at xyz[3*(k*numColumns + c) ...].
 *  - value / found [k*numColumns + c] (the layout irt_column_reduce reads) equal, bit for bit,
 *    irt_sample_points on irt_section_points' output, for every sampler.
 *  - column (numColumns elements per array) equals irt_column_reduce(value, found, numLevels,
 *    numColumns, weight, missValue) bit for bit: the reduction of "column products" above.
 *  - rgba[k*numColumns + c], row k = level k: for a found value v, s = postClassify(v)
 *    (deviceCode.cu:127-135) with the context's transfer function, a = clamp(s.w, 0, 1), C = a *
 *    ((s.rgb * ambientColor) * ambientRadiance), and the pixel is make_rgba(linear_to_srgb(C), a)
 *    (deviceCode.cu:336-340) -- the bytes irt_render_column's pixel write stores for (C, a) at
 *    accumID 0 over a cleared accum; there is no accum buffer here and no lerp.  A point that was
 *    not found gives 0.  ambientColor and ambientRadiance are read only when rgba is asked for.
 *    Non-finite values are outside the contract, as they are for frames.
 *  - A sampling call in every respect of "resampling" above: mode, ordering, no launch-ring slot, no
 *    statistics, IRT_E_CHAIN neither reported nor consumed.
 *  - IRT_E_INVALID, nothing written: what irt_sample_latlon refuses for one axis of pairs (a NULL or
 *    still-building context, a bad mode, a pending irt_update_values*, NULL lat, lon or radius with
 *    points to sample, a negative count, more than 2^36 points; like it, no angle or radius is
 *    looked at); a weight that is not finite; rgba non-NULL with no transfer function set, or with a
 *    non-finite ambientColor or ambientRadiance.  Zero columns or zero levels, or a d_out whose
 *    pointers are all NULL: IRT_OK, nothing launched. */
typedef struct irt_section_out {   /* DEVICE pointers; every one may be NULL: not written */
  float    *value;   /* [k*numColumns + c] */
  uint8_t  *found;   /* [k*numColumns + c] */
  uint32_t *rgba;    /* [k*numColumns + c]: the curtain, row k = level k, RGBA8 as fb */
  irt_column_out column;   /* [c] */
} irt_section_out;
int irt_section(irt_context *ctx, int mode, const float *lat, const float *lon, int numColumns,
                const float *radius, const float *weight, int numLevels,
                irt_vec3f ambientColor, float ambientRadiance,
                irt_section_out d_out, float missValue, void *stream);
/* Host helper, no GPU: the points irt_section samples, xyz[3*(k*numColumns + c) ...].  Refuses what
 * irt_section refuses of these arguments, and a NULL xyz with points to write. */
int irt_section_points(const float *lat, const float *lon, int numColumns,
                       const float *radius, int numLevels, float *xyz);
/* Host helper, no GPU: numPoints points along the great circle from (lat0, lon0) to (lat1, lon1)
 * (radians), the shorter way, equally spaced in angle; computed in double, rounded to float at the
 * end.  With a, b the end points' unit vectors and w = atan2(|a x b|, a . b): point i is at t =
 * i/(numPoints-1), p = (sin((1-t) w) a + sin(t w) b) / sin w, lat = asin(clamp(p.z/|p|, -1, 1)), lon =
 * atan2(p.y, p.x).  Points 0 and numPoints-1 are the inputs unchanged; numPoints == 1 gives the start
 * point.  *arc = w when arc is non-NULL: the plot's x-axis in radians.  End points closer than
 * sin w < 1e-9 give every point between them equal to the start.  A latitude of exactly +-pi/2 as a
 * float lies 4.4e-8 rad past the pole: a track between two such poles is the meridian the formula
 * gives it (lon + pi), not one chosen by the caller's lon.  The caller joins the legs of a polyline
 * by calling it per leg.
 * IRT_E_INVALID: numPoints < 1, a non-finite input, a NULL lat or lon, antipodal end points (sin w <
 * 1e-9 with a . b < 0: no unique circle). */
int irt_great_circle(float lat0, float lon0, float lat1, float lon1, int numPoints,
                     float *lat, float *lon, double *arc);

/* ---------------------------------------------------------------- field statistics
 * The distribution of the field's values, by value and by altitude band (a CFAD, contoured
 * frequency by altitude diagram): what a caller chooses a transfer function or a value range from.
 * After irt_update_values_device a step's values exist only on the device; this is the one pass
 * over them.  The reference's transfer-function editor has the slot (common/alpha_editor.h:47-48,
 * AlphaEditor::setHistogram) and never fills it.
 *
 * The definition (csrc/irt_histogram.h, compiled by the host helper and by the kernel).  Everything is
 * float, every accumulator an unsigned 64-bit integer: the result does not depend on the order of the
 * additions.  The items are every (record i, layer l) with 0 <= l < numLayers[i] over all records of
 * the scene -- the values dataRange is folded from.  Per item, v = value[l], h0 = height[l], h1 =
 * height[l+1]:
 *  - Weight w.  IRT_HIST_COUNT: w = 1.  IRT_HIST_THICKNESS: d = h1 - h0; w = (uint64_t)(d * 64.0f),
 *    truncating, when d > 0 and d <= 1048576.0f, else w = 0: the unit is 1/64 m (heights near 6.4e6 m
 *    are multiples of 0.5 m, so nothing is lost).  ICON cells have nearly equal area, so thickness
 *    stands in for volume.  An item with w == 0 is dropped entirely.
 *  - Band b.  bandEdges == NULL: one band, every item in it.  Otherwise m = (h0 + h1) * 0.5f and the
 *    item is in band b iff bandEdges[b] <= m && m < bandEdges[b+1]; an item in no band adds w to
 *    outside[0] and goes nowhere else.
 *  - Bin.  t = (v - lower) / (upper - lower), postClassify's normalisation (deviceCode.cu:129).  v not
 *    finite, or t NaN: tails[3b + 2] += w.  Else t < 0: tails[3b + 0] += w.  Else t > 1: tails[3b + 1]
 *    += w.  Else k = min((int)(t * (float)numBins), numBins - 1) and bins[b * numBins + k] += w.
 *    With numBins == the transfer function's size, bin k is postClassify's LUT index clamp(idx, 0,
 *    size - 1): the bins line up with the LUT entries.
 * The sum of bins, tails and outside is the sum of w over the items. */
#define IRT_HIST_COUNT 0
#define IRT_HIST_THICKNESS 1
typedef struct irt_histogram_out {   /* every pointer may be NULL: not written */
  uint64_t *bins;     /* [numBands * numBins] */
  uint64_t *tails;    /* [numBands * 3]: under, over, not finite */
  uint64_t *outside;  /* [1] */
} irt_histogram_out;
/* The histogram of the context's records with the values of every committed update.  Equal to
 * irt_histogram_cells on those records, integer for integer, however the context was made.
 *  - d_out holds DEVICE pointers, used on `stream`; the call OVERWRITES them (it does not add to what
 *    they held).  bandEdges is a HOST array of numBands + 1 floats, copied before the call returns;
 *    when it is NULL, numBands must be 1.
 *  - Ordering: a sampling call in the sense of "resampling" above -- no launch-ring slot, no render
 *    statistics, IRT_E_CHAIN neither reported nor consumed; irt_update_values*, irt_set_transfunc and
 *    irt_destroy wait for it; it runs after earlier sampling calls whatever their streams; between the
 *    first irt_update_values* and irt_update_values_end it returns IRT_E_INVALID.  It takes no sampler
 *    mode and needs neither a transfer function nor irt_build_wedge_accel.
 *  - IRT_E_INVALID, nothing written: a NULL or still-building context, or a pending update; numBins
 *    outside [1, 4096]; numBands outside [1, 64]; numBins * numBands > 4096; a valueRange that is not
 *    finite or has upper <= lower; an unknown weighting; band edges that are not finite and strictly
 *    ascending; NULL bandEdges with numBands != 1.
 *  - A d_out of NULLs: IRT_OK, nothing launched.  A scene without records: IRT_OK, the outputs zeroed. */
int irt_histogram(irt_context *ctx, irt_box1f valueRange, int numBins, int weighting,
                  const float *bandEdges, int numBands, irt_histogram_out d_out, void *stream);
/* Host helper and the definition, no GPU: the histogram of n records; out holds HOST pointers and is
 * overwritten.  Refuses what irt_histogram refuses of these arguments, NULL cells with n > 0
 * (IRT_E_INVALID) and a numLayers outside [0, 31] (IRT_E_DATA, as irt_create). */
int irt_histogram_cells(const irt_icon_cell *cells, size_t n, irt_box1f valueRange, int numBins,
                        int weighting, const float *bandEdges, int numBands, irt_histogram_out out);

/* ---------------------------------------------------------------- overlay
 * Lines on the globe -- coastlines, borders, a graticule -- drawn with the raygen's own jittered
 * rays, so that they line up with a frame pixel for pixel and anti-alias with it over progressive
 * frames.  An overlay is scene-independent: it reads a frame's accum and writes fb, so it composes
 * with irt_render, irt_render_levels and irt_render_column.  No counterpart in the reference.
 *
 * The definition (csrc/irt_overlay.h, compiled by the host helpers and by the kernel; float, never an
 * fma, with dot(x, y) = (x0*y0 + x1*y1) + x2*y2).  A line is a list of segments: arcs of great circles
 * no longer than 0.2 rad, each drawn in one of up to IRT_OVERLAY_MAX_STYLES styles.  A style is a
 * straight-alpha colour and a half-width W in radians on the sphere, 0 < W <= 0.05; from it, in double
 * and rounded once to float, sinW = sin(W) and chord2 = (2 sin(W/2))^2.  A unit vector u is covered by
 * segment i iff
 *   body   = fabsf(dot(u,n)) <= sinW && fabsf(dot(u,t)) <= sinHalf && dot(u,a) + dot(u,b) > 0
 *   cap(e) = with d = u - e per component, dot(d,d) <= chord2
 *   covered = body || cap(a) || cap(b)
 * with sinW and chord2 of the segment's style (the caps use chord lengths because cos W of a thin line
 * rounds to 1.0f; the > 0 term keeps the antipodal arc out).  The segment of u is the LOWEST index that
 * covers it, or -1.
 * The bins: a cube map of N = binsPerEdge in [1, 256] bins per face edge, 6 N^2 bins.  The face of u
 * is 2 * axis + (u[axis] < 0), axis that of the largest |component| (a tie goes to the lowest axis);
 * (p, q) are the two other components, in axis order, each divided by |u[axis]|; i = min((int)((p +
 * 1.f) * 0.5f * N), N - 1) clamped at 0, j likewise from q; bin = (face * N + j) * N + i. */
#define IRT_OVERLAY_MAX_STYLES 8
#define IRT_OVERLAY_OVER 1       /* irt_render_overlay: the lines on top of the frame */
typedef struct irt_overlay_segment {   /* 64 B, one cache line */
  float a[3], b[3];   /* the end points, unit vectors */
  float n[3];         /* the unit normal of their great circle: a x b normalised */
  float t[3];         /* the unit tangent at the arc's midpoint: b - a normalised */
  float sinHalf;      /* the sine of half the arc */
  int32_t style;
  uint32_t pad[2];    /* zero */
} irt_overlay_segment;
typedef struct irt_overlay_style {
  irt_vec4f rgba;     /* straight alpha */
  float halfWidth;    /* radians on the sphere, in (0, 0.05] */
} irt_overlay_style;
typedef struct irt_overlay irt_overlay;

/* Host helpers, no GPU.  Each refuses (IRT_E_INVALID, nothing written) NULL pointers with work to do,
 * a style index outside its table, widths and arcs outside the ranges above, and 2^24 segments or more.
 *
 * irt_overlay_segments: polylines as segments.  lat, lon are float radians; points first[l] ..
 * first[l+1]-1 are line l.  Unit vectors are computed in double on the axes of irt_latlon_points (x =
 * cos lat cos lon, y = cos lat sin lon, z = sin lat), so a line at (lat, lon) lies over the field
 * irt_sample_latlon reports there.  Consecutive points whose float unit vectors are equal are merged;
 * every remaining leg is cut by slerp, in double, into ceil(arc / maxArc) equal pieces (0 < maxArc <=
 * 0.2 rad), and every field of a piece is rounded to float at the end.  Also refused: a non-finite
 * input, and consecutive antipodal points (irt_great_circle's rule).  *count = the segments needed;
 * out == NULL only counts, capacity < *count is IRT_E_INVALID. */
int irt_overlay_segments(const float *lat, const float *lon, const int32_t *first, int numLines,
                         float maxArc, int style, irt_overlay_segment *out, size_t capacity,
                         size_t *count);
/* The graticule, built through irt_overlay_segments: the meridians lon = m stepLon, m = 0 ..
 * floor(2 pi / stepLon) - 1, great-circle arcs pole to pole; the parallels lat = k stepLat for every
 * integer k with |lat| < pi/2, closed chains of great-circle arcs of at most maxArc in longitude.  Such
 * a chord of a parallel at latitude phi leaves the true parallel by (maxArc^2 / 8) sin phi cos phi at
 * its middle: at 1 degree arcs at most 1.9e-5 rad, 121 m on the Earth, at 45 degrees (under 100 m
 * poleward of 63 and equatorward of 27 degrees).  Steps in (0, pi] x (0, 2 pi] radians. */
int irt_graticule(float stepLat, float stepLon, float maxArc, int style, irt_overlay_segment *out,
                  size_t capacity, size_t *count);
/* The bin table as CSR: binStart[6 N^2 + 1], and binSeg[binStart[b] .. binStart[b+1]) the segments of
 * bin b, ASCENDING.  A segment goes to every bin whose bounding cap (its centre direction and the
 * largest corner angle) comes within the sum of the radii plus 1e-5 rad of the segment's cap (the
 * arc's midpoint, half the arc + maxHalfWidth), all in double: more bins than a segment covers points
 * in, never fewer.  *count = the entries; binSeg == NULL fills binStart alone. */
int irt_overlay_bins(const irt_overlay_segment *seg, size_t n, float maxHalfWidth, int binsPerEdge,
                     uint32_t *binStart, uint32_t *binSeg, size_t capacity, size_t *count);
/* The definition applied to numPoints unit vectors u[3 p ..]: segment[p] = the segment of point p.
 * binStart == NULL scans every segment; else only the list of the point's bin, to its first hit. */
int irt_overlay_cover(const irt_overlay_segment *seg, size_t n, const irt_overlay_style *styles,
                      int numStyles, const uint32_t *binStart, const uint32_t *binSeg,
                      int binsPerEdge, const float *u, size_t numPoints, int32_t *segment);

/* A convenience: the half-width in radians on the sphere of surfaceRadius of a line `pixels` pixels wide
 * at the sub-camera point of lp's camera.  In double, left to right: n = dir_du x dir_dv; focal =
 * |dir_00 . n| / |n|; a pixel's angle at the frame's centre = |dir_dv| / focal; its footprint = that
 * angle times | |org| - surfaceRadius |; *halfWidth = 0.5 * pixels * footprint / surfaceRadius, clamped to
 * [1e-7, 0.05] and rounded to float.  IRT_E_INVALID: a NULL pointer, a surfaceRadius or pixels that is not
 * finite and positive. */
int irt_overlay_width(const irt_launch_params *lp, float surfaceRadius, float pixels, float *halfWidth);

/* The device object: the segments, the styles and the bin table in memory the context owns (the
 * segment array 64-byte aligned there).  binsPerEdge 0 picks N so that the mean list stays near 16
 * entries, capped at 256.  n == 0 is legal: the render call then only composites.  A context may hold
 * several overlays; irt_overlay_destroy waits for the sampling calls issued so far, and irt_destroy
 * frees the overlays that are left. */
int irt_overlay_create(irt_context *ctx, const irt_overlay_segment *seg, size_t n,
                       const irt_overlay_style *styles, int numStyles, int binsPerEdge,
                       irt_overlay **overlay);
int irt_overlay_destroy(irt_context *ctx, irt_overlay *overlay);
/* The bin table an overlay was created with: its bins per edge (the library's choice where 0 was asked
 * for) and the number of list entries; either pointer may be NULL. */
int irt_overlay_get_bins(const irt_context *ctx, const irt_overlay *overlay, int *binsPerEdge,
                         size_t *numEntries);
/* Draws the overlay into a frame of width x height pixels.  Per pixel p:
 *  - the ray and the single hit slot of irt_render_column on the sphere of surfaceRadius: the near hit
 *    when tn > 0, else the far hit when tf > 0; P = org + dir * t, len = sqrtf((P.x*P.x + P.y*P.y) +
 *    P.z*P.z), u = P / len per component;
 *  - s = the segment of u (through the bins), -1 for a pixel without a hit; d_segment[p] = s (d_segment
 *    may be NULL): which line is under the cursor;
 *  - the line sample L = (r*a, g*a, b*a, a) of s's style, or 0; d_cover[p] = w * L + (1 - w) *
 *    d_cover[p] with w = 1 / (accumID + 1), the lerp of every render call: progressive frames
 *    anti-alias the hard edge through the raygen's own jitter.  The product (1 - w) * d_cover[p] is
 *    formed at accumID 0 too, where w = 1: d_cover must hold finite values before the first frame
 *    (clear it, as irt_clear_frame clears accum) -- 0 * NaN and 0 * inf are NaN, and a NaN stays;
 *  - with V = d_accum_in[p] (premultiplied, as every render call leaves it; 0 when d_accum_in is NULL)
 *    and K = d_cover[p], one multiply and one add per component: out = V + (1 - V.w) * K (the lines
 *    under the volume, on the Earth's surface), or with IRT_OVERLAY_OVER out = K + (1 - K.w) * V;
 *  - d_fb[p] = make_rgba(linear_to_srgb(out.rgb), out.w), as every render call writes fb.
 * d_accum_in is never written, so a progressive irt_render loop goes on undisturbed and its next frame
 * rewrites fb from accum.  Every pixel of the frame is written.  Of lp the call uses the camera and
 * accumID.  A sampling call in every respect of "resampling" above (the cell mode's checks: neither a
 * transfer function nor irt_build_wedge_accel is needed): ordering, no launch-ring slot, no
 * statistics, no IRT_E_CHAIN, refused while an update is pending.
 * IRT_E_INVALID, nothing written: a NULL overlay, lp, d_cover or d_fb; an overlay of another context;
 * a surfaceRadius that is not finite and positive; unknown flag bits; a frame irt_render_levels
 * refuses.  Far-side lines seen through the globe, the tile forms, multi-GPU splitting and several
 * frames per launch have no overlay form. */
int irt_render_overlay(irt_context *ctx, const irt_overlay *overlay, const irt_launch_params *lp,
                       int width, int height, float surfaceRadius, int flags,
                       const irt_vec4f *d_accum_in, irt_vec4f *d_cover, uint32_t *d_fb,
                       int32_t *d_segment, void *stream);

/* ---------------------------------------------------------------- isolines
 * Isolines of a lat x lon value grid -- one level of irt_sample_latlon, one array of irt_column_out
 * -- as overlay segments: marching squares on the sphere, from DEVICE values to a compact DEVICE
 * array of irt_overlay_segment in a fixed order, ready for irt_overlay_create.  No counterpart in
 * the reference.
 *
 * The definition (csrc/irt_contour.h, compiled by the host helper and by the kernels).  All arithmetic
 * is double + - * / sqrt on float inputs, never an fma, evaluated left to right as written; the
 * saddle's centre value alone is float.
 *  - Inputs: value[j*numLon + i] and found[j*numLon + i] (found == NULL: every point is found);
 *    lat[numLat], lon[numLon] float radians, strictly ascending, each step (the float difference of
 *    neighbours) <= 0.1f rad, so that a cell's diagonal stays under the overlay's 0.2 rad arc limit;
 *    numLat, numLon >= 2 and numLat * numLon < 2^27.  IRT_CONTOUR_WRAP: the grid closes in
 *    longitude, numLon columns of cells instead of numLon - 1, the last between lon[numLon-1] and
 *    lon[0]; legal only if, in double, lon[numLon-1] - lon[0] < 2 pi and the closing step 2 pi - that
 *    span is <= 0.1f.  threshold[T], 1 <= T <= IRT_CONTOUR_MAX_THRESHOLDS, each finite, in any
 *    order, repeats allowed; style[T] in [0, IRT_OVERLAY_MAX_STYLES), copied into the segments.
 *  - Corner vectors: the host computes cos and sin of every lat and every lon once, in double, with
 *    glibc (the axes of irt_latlon_points and irt_overlay_segments); the device receives the four
 *    tables; a corner's unit vector is (cl*co, cl*si, sl).
 *  - A cell (j, i) has corners 0 = (j, i), 1 = (j, i+1), 2 = (j+1, i+1), 3 = (j+1, i), i+1 modulo
 *    numLon with wrap.  It emits nothing, for every threshold, if any corner is not found or not
 *    finite.  Its edges, each always evaluated in this direction, so that the two cells sharing an
 *    edge compute the same bits: e0 = 0 -> 1 (south), e1 = 1 -> 2 (east), e2 = 3 -> 2 (north),
 *    e3 = 0 -> 3 (west).
 *  - For threshold c: mask = sum over k of (v_k >= c) << k.  The crossing on an edge from corner A
 *    to corner B: t = ((double)c - va) / ((double)vb - va); p = A + t*(B - A) per component;
 *    P = p / sqrt((px*px + py*py) + pz*pz) per component.
 *  - Segments per mask, first edge -> second edge (the side with value >= c lies on the left, seen
 *    from outside with north up):  0, 15: none;  1: e0->e3;  2: e1->e0;  3: e1->e3;  4: e2->e1;
 *    6: e2->e0;  7: e2->e3;  8: e3->e2;  9: e0->e2;  11: e1->e2;  12: e3->e1;  13: e0->e1;
 *    14: e3->e0.  Saddles, with the centre value m = ((v0 + v1) + (v2 + v3)) * 0.25f in float:
 *    mask 5: m >= c ? (e0->e1, e2->e3) : (e0->e3, e2->e1);  mask 10: m >= c ? (e1->e2, e3->e0) :
 *    (e1->e0, e3->e2); in the order written.
 *  - The segment from crossing Pa to crossing Pb (double), each field rounded once to float:
 *    a = Pa, b = Pb; n = N / |N| with N = (Pa.y*Pb.z - Pa.z*Pb.y, Pa.z*Pb.x - Pa.x*Pb.z,
 *    Pa.x*Pb.y - Pa.y*Pb.x); t = D / |D| with D = Pb - Pa; sinHalf = 0.5 * |D| (half the chord of two
 *    unit vectors is the sine of half the arc); |v| = sqrt((vx*vx + vy*vy) + vz*vz); style =
 *    style[T index], pad = 0.  A segment whose a and b are equal as floats in all three components is
 *    DROPPED (a crossing at a shared corner; collapsed pole rows) and counts nowhere.
 *  - Output order: threshold index (the caller's order), then cell index j*numCellsLon + i, then the
 *    order within the cell.  The overlay's "lowest index wins" and d_segment picking depend on it.
 *
 * irt_contour_cells: the definition on the host, no GPU.  *count = the segments; countPerThreshold
 * (T entries, may be NULL) their number per threshold.  out == NULL only counts; capacity < *count is
 * IRT_E_INVALID with *count (and countPerThreshold) set.  IRT_E_INVALID, nothing written: an input
 * outside the conditions above, a NULL value, lat, lon, threshold, style or count, unknown flag bits,
 * 2^24 segments or more (the overlay's limit).
 *
 * irt_contour_grid: the same on the device, bit for bit and in the same order on every run.  d_value
 * and d_found (may be NULL) are DEVICE arrays read on `stream`; lat, lon, threshold and style are HOST
 * arrays, copied before the call returns; d_out is a DEVICE array of `capacity` segments, 64-byte
 * aligned (refused otherwise), each segment written as one whole 64-byte line.  Three passes without
 * a global atomic: count (one lane per cell, the kept segments of every threshold, per-workgroup
 * totals from wave ballots), an exclusive scan of the totals in (threshold, workgroup) order, and
 * emit (each lane's place from the scanned total and a wave prefix; the lane runs the definition
 * again).  The counts are returned on the host, so THE CALL SYNCHRONISES `stream` after the first two
 * passes; the emit pass is then queued on `stream`, and d_out is valid in stream order like any
 * sampling call's output.  d_out == NULL counts only (no third pass); capacity < *count is
 * IRT_E_INVALID with *count set and no byte of d_out written.  The scratch (4 bytes per cell, 4 bytes
 * per threshold and 256 cells, the tables) belongs to the context, grows on demand and is freed by
 * irt_destroy.  A sampling call in every respect of "resampling" above (the cell mode's checks):
 * ordering, no launch-ring slot, no statistics, no IRT_E_CHAIN, refused while an update is pending.
 * IRT_E_INVALID, nothing written: what irt_contour_cells refuses, a NULL or still-building context, a
 * NULL d_value, a d_out that is not 64-byte aligned.
 *
 * irt_contour_latlon: irt_sample_latlon(mode, lat, lon, {radius}) with missValue NaN into a grid the
 * context owns, then irt_contour_grid on it, on the same stream: equal, bit for bit, to the two calls
 * made by hand.  Also refused: a radius that is not finite and positive, and what irt_sample_latlon
 * refuses for `mode`.
 *
 * Not here: joining segments into polylines, labels, smoothing, building the overlay's bin table on
 * the device (irt_overlay_create builds it on the host from a host copy of the segments), tile and
 * multi-GPU forms. */
#define IRT_CONTOUR_WRAP 1
#define IRT_CONTOUR_MAX_THRESHOLDS 16
int irt_contour_cells(const float *value, const uint8_t *found, const float *lat, int numLat,
                      const float *lon, int numLon, const float *threshold, const int32_t *style,
                      int numThresholds, int flags, irt_overlay_segment *out, size_t capacity,
                      size_t *count, size_t *countPerThreshold);
int irt_contour_grid(irt_context *ctx, const float *d_value, const uint8_t *d_found,
                     const float *lat, int numLat, const float *lon, int numLon,
                     const float *threshold, const int32_t *style, int numThresholds, int flags,
                     irt_overlay_segment *d_out, size_t capacity, size_t *count,
                     size_t *countPerThreshold, void *stream);
int irt_contour_latlon(irt_context *ctx, int mode, const float *lat, int numLat, const float *lon,
                       int numLon, float radius, const float *threshold, const int32_t *style,
                       int numThresholds, int flags, irt_overlay_segment *d_out, size_t capacity,
                       size_t *count, size_t *countPerThreshold, void *stream);

/* == clearFramebuffer (common/pipeline.cu:171-199): fb = make_rgba(0), accum = 0. */
int irt_clear_frame(irt_context *ctx, uint32_t *d_fb, irt_vec4f *d_accum, size_t numPixels,
                    void *stream);

/* == one Pipeline::launch() of the raygen over the full width x height launch
 * (pipeline.cu:1061-1074 / owlLaunch2D 1064).  d_fb / d_accum are device arrays of
 * width*height, pixel (x,y) at x + width*y (deviceCode.cu:286). */
int irt_render(irt_context *ctx, const irt_launch_params *lp, int width, int height,
               uint32_t *d_fb, irt_vec4f *d_accum, void *stream);

/* Frame-tile subset of the same launch, for multi-GPU frame splitting: renders the
 * 64x64 tiles t = tileBegin, tileBegin+tileStride, ... (row-major tile ids over
 * ceil(width/64) x ceil(height/64)) into PACKED buffers: tile k of this subset at
 * d_fb_tiles[k*4096 + ly*64 + lx].  Pixel seeds/cameras use the full-launch (x,y,width,
 * height), so every pixel is bit-identical to irt_render's.  Returns the tile count in
 * *numTiles when non-NULL. */
int irt_render_tiles(irt_context *ctx, const irt_launch_params *lp, int width, int height,
                     int tileBegin, int tileStride, uint32_t *d_fb_tiles,
                     irt_vec4f *d_accum_tiles, int *numTiles, void *stream);

/* The reference's progressive accumulation (`--sample-limit N`: Pipeline::isRunning /
 * launch, pipeline.cu:991-1075, with accumID = frameID, hostCode.cu:947-958) batched:
 * numFrames consecutive frames accumID = lp->accumID .. lp->accumID+numFrames-1 in one
 * launch, bit-identical to numFrames irt_render calls with accumID incremented (each
 * frame's lerp(new, old, 1/(accumID+1)), deviceCode.cu:333-334, applied in order; fb holds
 * the last frame's make_rgba(linear_to_srgb(accum))).  The _tiles form packs like
 * irt_render_tiles and is what each rank runs in the multi-GPU weak-scaling split.
 * The frames are chained per pixel inside the one launch (frame f's workgroup of a block
 * lerps once frame f - 1's has published the same pixels), so the next frame's workgroups
 * fill the chip while the previous frame's last ones finish.  Every frame's accum is written;
 * fb is converted and stored by the launch's last frame (earlier frames may skip it) and holds, when the launch ends,
 * the bytes numFrames separate launches would leave (a pixel whose ray misses the world box in
 * the last frame: those of its latest earlier hit in the launch; none: untouched).
 * A hand-off wait is bounded (~1 s).  If one ever gives up, the launch's frames were lerped
 * out of order, and the launch fails loudly instead of returning wrong pixels silently: the
 * next call on the context that sees it -- any irt_render* call, irt_get_render_stats*,
 * irt_reset_render_stats_total -- returns IRT_E_CHAIN, irt_last_error() names the launch, and
 * the context renders later multi-frame launches without chaining (per-frame sample buffer +
 * a lerp pass).  The call that returns IRT_E_CHAIN has NOT enqueued its own work: its frame(s)
 * were not rendered, and the caller re-issues the call (or restarts the accumulation from
 * accumID 0).  (The reference's launch either renders the frame or aborts,
 * pipeline.cu:1038-1075.)  Frames of 2^27 pixels or more are never chained. */
int irt_render_accumulate(irt_context *ctx, const irt_launch_params *lp, int width, int height,
                          int numFrames, uint32_t *d_fb, irt_vec4f *d_accum, void *stream);
/* A sequence of views in one launch: frame k renders lps[k] -- its own camera (org, dir_00,
 * dir_du, dir_dv) and accumID; every other member must equal lps[0]'s -- into the same fb and
 * accum, bit-identical to numFrames irt_render calls in order (the reference's render loop,
 * pipeline.cu:991-1075, with the camera moved between frames: an orbit or a camera path).  The
 * frames are chained per pixel in the launch, as in irt_render_accumulate; with a variant or
 * setting that cannot chain, one launch per frame. */
int irt_render_sequence(irt_context *ctx, const irt_launch_params *lps, int numFrames, int width,
                        int height, uint32_t *d_fb, irt_vec4f *d_accum, void *stream);
/* The same over one rank's tile list, packed as irt_render_tile_list packs it (the multi-GPU
 * split of a camera path: every rank renders its tiles of the same views). */
int irt_render_tile_list_sequence(irt_context *ctx, const irt_launch_params *lps, int numFrames,
                                  int width, int height, const int32_t *tiles, int numTiles,
                                  uint32_t *d_fb_tiles, irt_vec4f *d_accum_tiles, void *stream);
int irt_render_tiles_accumulate(irt_context *ctx, const irt_launch_params *lp, int width,
                                int height, int tileBegin, int tileStride, int numFrames,
                                uint32_t *d_fb_tiles, irt_vec4f *d_accum_tiles, int *numTiles,
                                void *stream);

/* Scatter packed tiles (as produced by irt_render_tiles on `numRanks` ranks and gathered
 * rank-major into d_gathered[rank][maxTilesPerRank][4096]) into a linear framebuffer. */
int irt_unpack_tiles(irt_context *ctx, const uint32_t *d_gathered, int numRanks,
                     int maxTilesPerRank, int width, int height, uint32_t *d_fb, void *stream);

/* Cost-balanced multi-GPU deal of a width x height launch's 64x64 tiles (no GPU needed;
 * the reference's CPU path hands the same tiles to a thread pool dynamically,
 * common/thread_pool.h:146-161, for_each.h:70-85).  Each tile's cost is estimated from the
 * camera (lp) and the shell radii (info->sphericalBounds): rays through an 8x8 subset of
 * its pixels, weighted by whether they reach the box and the shell and by their chord
 * through the shell.  Tiles go, heaviest first (ties by id), to the least-loaded rank
 * (longest-processing-time first; ties to the lowest rank); rank 0 starts loaded with
 * rank0Extra x the frame's total estimated cost (in [0, 1): the work rank 0 does beyond its
 * tiles, e.g. the framebuffer unpack per rendered frame).  Deterministic: every rank
 * computes the same table.  table: numRanks x maxTilesPerRank, rank-major, row r = rank r's
 * tiles in render order (heaviest first), -1 padding; table == NULL returns only
 * *maxTilesPerRank (the longest row). */
int irt_deal_tiles(const irt_launch_params *lp, const irt_volume_info *info, int width,
                   int height, int numRanks, float rank0Extra, int32_t *table, size_t capacity,
                   int *maxTilesPerRank);

/* irt_render_tiles / irt_render_tiles_accumulate over an explicit tile list (host array of
 * row-major tile ids, e.g. one row of irt_deal_tiles' table without its -1 padding):
 * list entry k is packed at d_fb_tiles[k*4096 ...].  numFrames >= 1 consecutive progressive
 * frames as irt_render_tiles_accumulate.  Every pixel is bit-identical to irt_render's. */
int irt_render_tile_list(irt_context *ctx, const irt_launch_params *lp, int width, int height,
                         const int32_t *tiles, int numTiles, int numFrames,
                         uint32_t *d_fb_tiles, irt_vec4f *d_accum_tiles, void *stream);

/* Scatter packed tiles gathered rank-major (d_gathered[rank][maxTilesPerRank][4096]) whose
 * tile ids are the host table[rank * maxTilesPerRank + k] (irt_deal_tiles; -1: empty). */
int irt_unpack_tile_table(irt_context *ctx, const uint32_t *d_gathered, int numRanks,
                          int maxTilesPerRank, const int32_t *table, int width, int height,
                          uint32_t *d_fb, void *stream);

/* Statistics of the most recent launch (waits for it).  Launches never wait for earlier
 * ones' statistics: counters are read back through a ring, so frames queue back to back
 * like the reference's GPU path (owlLaunch2D is asynchronous, pipeline.cu:1064).
 * Returns IRT_E_CHAIN once for a chained launch whose hand-off timed out (see
 * irt_render_accumulate). */
int irt_get_render_stats(const irt_context *ctx, irt_render_stats *stats);
/* Sums over every launch since the last reset; *launches = count.  kernelMs is the mean
 * of the timed launches times the launch count (see irt_set_timing_interval). */
int irt_get_render_stats_total(const irt_context *ctx, irt_render_stats *total,
                               long long *launches);
int irt_reset_render_stats_total(irt_context *ctx);
/* Kernel timing (HIP events on the launch stream) on every `every`-th launch only (default
 * 8; 1 = every launch): an event pair per frame adds ~10 us of stream gaps to a 0.17 ms
 * frame.  irt_render_stats.kernelMs of a launch is that of the most recent timed launch.
 * No counterpart in the reference, which times on the host (pipeline.cu:1062-1073). */
int irt_set_timing_interval(irt_context *ctx, int every);
/* The per-launch event counts of irt_render_stats (rays, sampleVolume calls, samples found,
 * candidates) on (1, the default) or off (0).  Counting costs each launch a store of every
 * workgroup's counts into pinned host memory -- ~1.5 % of a C3 frame, more of a small
 * multi-GPU share -- and the reference renders without it; with counting off the counts
 * read 0 (kernelMs stays).  Frames are identical either way.  No reference counterpart. */
int irt_set_statistics(irt_context *ctx, int on);

/* buildCuBQLAccel (hostCode.cu:557-649) for IRT_MODE_CUBQL: the wedges of every (cell,
 * layer) -- corners toCartesian(height[h|h+1], lat, lon), scalar
 * h == 0 ? getValue(height[0]) : (getValue(height[h-1]) + getValue(height[h])) * 0.5 on
 * all six vertices -- behind a cube-map locator of their primBounds (replacing the cuBQL
 * BVH).  `cells` must be the array given to irt_create.  A sample takes the first wedge,
 * in (cell, layer) order, whose bounds contain it and whose intersectWedgeEXT
 * (UElems.h:214-311) accepts it; cuBQL's own traversal order is not reproducible here
 * (the submodule is not vendored), so that order is the documented choice. */
int irt_build_wedge_accel(irt_context *ctx, const irt_icon_cell *cells, size_t n);
/* The same locator also serves IRT_MODE_TRIANGLES (buildTriangleAccel, hostCode.cu:440-484):
 * every cell's bottom triangle toCartesian(height[0], lat, lon) is listed too. */

/* Download the GRID_ACCEL_MODE grid (256^3 macrocells over the volume bounds,
 * hostCode.cu:668-682; index x + 256*(y + 256*z)), same conventions as irt_get_shell.
 * The grid (201 MB) is built on first use -- this call or the first IRT_ACCEL_GRID render --
 * not at irt_create as the reference's main() does (hostCode.cu:875): same grid, no cost to
 * sphere-mode runs. */
int irt_get_grid(const irt_context *ctx, float *valueRanges, float *maxOpacities);

/* Download the shell accelerator (for checking): valueRanges as 2 floats per
 * macrocell, maxOpacities as 1 float per macrocell; either may be NULL. */
int irt_get_shell(const irt_context *ctx, float *valueRanges, float *maxOpacities);

/* Number of tiles of a width x height launch. */
int irt_num_tiles(int width, int height);

/* ---------------------------------------------------------------- host helpers
 * (no GPU needed) -- the host-side setup of icon_rt's main() and common/, so a host
 * program (the C++ Pipeline mirror under icon-ray-tracing_amd/host, or Python) can
 * reproduce the reference's frame setup bit for bit. */

/* Load a raw `.ic` file (hostCode.cu:717-734): N = filesize/284; the first
 * min(N, maxNumCells) records if maxNumCells >= 0.  Call with out == NULL to get the
 * count in *count; then with capacity >= count. */
int irt_load_ic(const char *path, long maxNumCells, irt_icon_cell *out, size_t capacity,
                size_t *count);
int irt_save_ic(const char *path, const irt_icon_cell *cells, size_t count);

/* convert_icon (tools/convert_icon/convert_icon.cpp:168-391): DWD ICON netCDF inputs ->
 * `.ic` records, the convertToIC branch (353-391) evaluated exactly, including its
 * quirks: at most maxLayers data levels (24, 345-349), the last record of a column gets
 * `numLayers % 32 - 1` layers (365), heights R + HHL - HSURF with float/double mixing as
 * written (361, 371), values min/max-normalised in double (317-328), HHL and data files
 * sorted by their `height` level index, descending (274, 337).  Inputs are netCDF
 * classic files (CDF-1/2/5; the netCDF library is replaced by host/irt_netcdf.cpp);
 * netCDF-4/HDF5 inputs fail with IRT_E_IO.  Where the reference reads out of bounds
 * (too few HHL/data files for the layers, a data file with fewer than `cell` values)
 * this returns IRT_E_DATA.  Slots the reference leaves uninitialised are zero.
 * Two-call pattern: out == NULL returns the record count in *count. */
typedef struct irt_convert_opts {
  const char *hgridFile;          /* -hgrid: clon_vertices/clat_vertices (200-203) */
  const char *hsurfFile;          /* -hsurf: HSURF (225) */
  const char *const *hhlFiles;    /* -hhl: height + HHL per file (239-272) */
  int numHhlFiles;
  const char *const *dataFiles;   /* -data: ncells, height + the variable (282-335) */
  int numDataFiles;
  const char *varName;            /* NULL = "pres" (308) */
  int maxLayers;                  /* <= 0: 5 (24) */
} irt_convert_opts;
int irt_convert_icon(const irt_convert_opts *opts, irt_icon_cell *out, size_t capacity,
                     size_t *count);

/* convert_icon's UMesh output (tools/convert_icon/convert_icon.cpp:393-452, the tool's
 * default convertToUMesh branch): one wedge per (cell, layer) with six vertices of its own
 * at R + HSURF*50 / R + (HHL - HSURF)*50, each carrying the layer's value, written to
 * `path` in umesh's binary layout (u64 magic 0x234235567, then u64-counted arrays:
 * vertices vec3f, per-vertex f32 scalars, triangles, quads, tets, pyramids, wedges
 * (6 x i32), hexes).  Needs numLayers+1 HHL files (the reference reads hhl[j+1]).
 * The counts written go to *numVertices / *numWedges (either may be NULL). */
int irt_convert_icon_umesh(const irt_convert_opts *opts, const char *path, size_t *numVertices,
                           size_t *numWedges);

/* Lat/lon filter in degrees (hostCode.cu:736-758); stable, in place; returns the kept
 * count in *count. */
int irt_filter_cells(irt_icon_cell *cells, size_t n, irt_box1f latRangeDeg,
                     irt_box1f lonRangeDeg, size_t *count);

/* Volume facts without a GPU (same values irt_get_volume_info reports). */
int irt_compute_volume_info(const irt_icon_cell *cells, size_t n, irt_volume_info *info);

/* Default transfer function of hostCode.cu:823-836 after Pipeline::setTransfunc's
 * resampling to 300 entries (pipeline.cu:469-473): writes 300 entries to out300 and the
 * value range (dataRange, or [0,1] if empty) to *valueRange. */
int irt_default_transfunc(irt_box1f dataRange, irt_vec4f *out300, irt_box1f *valueRange);

/* resampleLUT (common/dvr_course-common.h:44-70). */
int irt_resample_lut(const irt_vec4f *src, int nsrc, irt_vec4f *dst, int ndst);

/* Camera (common/camera.h) -> LaunchParams.camera as hostCode.cu:939-945 computes it:
 * org = getPosition(), dir_00 = lower_left, dir_du = horizontal/imgW, dir_dv =
 * vertical/imgH.  irt_camera_view_all: Camera::viewAll (camera.h:98-104) with the
 * default fovy of 90 degrees; irt_camera_look_at: Pipeline's --camera vp vi vu / -fovy
 * path (pipeline.cu:444-454; fovy in degrees, <1e-3 -> 90). */
int irt_camera_view_all(irt_box3f bounds, float fovyDeg, int imgW, int imgH,
                        irt_launch_params *lp);
int irt_camera_look_at(irt_vec3f vp, irt_vec3f vi, irt_vec3f vu, float fovyDeg, int imgW,
                       int imgH, irt_launch_params *lp);

/* Synthetic RnBk icosahedral ICON grid (no netCDF offline): 20*rootN^2*4^bisections
 * triangles, `levels` layers with heights R + topHeight*(l/levels)^2, a smooth value
 * field normalised to [0,1] (plus `noise` * hash noise, seeded), stored as `.ic` records
 * of <= 31 layers, bottom to top, consecutive per column.  out == NULL -> count only. */
int irt_synth_grid(int rootN, int bisections, int levels, float topHeight, float noise,
                   uint32_t seed, irt_icon_cell *out, size_t capacity, size_t *count);
/* The same grid over terrain, as tools/convert_icon's `.ic` branch (convert_icon.cpp:353-391)
 * would write it from DWD-like fields: HSURF per column up to terrainHeight metres (~60 % of the
 * columns land), HHL terrain-following near the ground and flat above (the per-column offset
 * HSURF (1 - z/Zd)^2 shrinking with height z, Zd = min(topHeight, 20 km)), records with
 * H[0] = R + HSURF and H[j] = R + HHL - HSURF (so every land column's first layer is inverted)
 * and the last record of a column holding levels % 32 - 1 layers.  terrainHeight 0 ==
 * irt_synth_grid; needs levels % 32 != 0 and 2 terrainHeight < Zd. */
int irt_synth_grid_terrain(int rootN, int bisections, int levels, float topHeight, float noise,
                           uint32_t seed, float terrainHeight, irt_icon_cell *out,
                           size_t capacity, size_t *count);

#ifdef __cplusplus
}
#endif
#endif /* ICON_RT_HIP_H */
