// irt_context.h -- struct irt_context and the helpers its three translation units share:
// irt_context.hip (the scene side), irt_launch.hip (the launch side) and irt_debug_hooks.hip
// (the irt_debug_* hooks that need a context or a device).  Private to csrc/.
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>
#include <vector>

#include "irt_internal.h"
#include "irt_kernels.h"

// records the failed call as the last error (irt_context.hip); returns IRT_E_HIP
int irt_hip_failed(const char *call, hipError_t e, const char *file, int line);

#define IRT_HIP(call)                                                           \
  do {                                                                          \
    hipError_t e_ = (call);                                                     \
    if (e_ != hipSuccess) return irt_hip_failed(#call, e_, __FILE__, __LINE__); \
  } while (0)

// One entry of the launch ring (irt_context::ring; launch i lives in slot i % kSlots).
// Life cycle:
//   launched  the commit step of render_impl (irt_launch.hip) writes every field but the event
//             handles (created in irt_create_end, destroyed in free_all) and sets `pending`;
//   marked    optionally, done_event records evDone after the fact and sets `marked` -- the only
//             field written between launch and retirement;
//   retired   finish_slot waits for the launch, reads the record and clears `pending`; only then
//             may the slot be launched again.
// sched_prepare clears `costsOf` (whatever the slot's state) when the frame grid changes.
// What the device writes for a slot is not here but in pinned arrays of their own, indexed by the
// slot: h_chainFail, h_counters, h_wgCounts and h_schedCost.
struct LaunchSlot {
  hipEvent_t ev0 = nullptr, ev1 = nullptr;  // kernel timing, recorded when `timed`
  // after the launch (no timestamps).  Recorded with the launch only every kDoneEvery-th launch
  // or when its costs are copied, else when asked for (done_event): each marker on the queue
  // costs its launch ~1-2 us, and a later marker on the same stream completes after it as well
  hipEvent_t evDone = nullptr;
  bool pending = false;    // launched, not retired
  bool marked = false;     // evDone is recorded behind this launch
  bool timed = false;      // ev0 / ev1 surround the kernel
  bool block = false;      // k_stats_out copied the 16-counter block into h_counters
  hipStream_t stream = nullptr;
  long long launch = 0;    // the launch's index
  size_t numWG = 0;        // workgroups whose counts h_wgCounts holds (0: none to sum)
  long long costsOf = -1;  // launch whose workgroup costs h_schedCost holds for this slot (-1: none)
};

struct irt_context {
  int device = 0;
  hipStream_t stream = nullptr;
  irt_volume_info info{};
  uint32_t n = 0;
  int G = 0;
  // HBM
  uint4 *d_binHdr = nullptr;   // binned locator (irt_common.h)
  float4 *d_fat = nullptr;
  float4 *d_blocks = nullptr;
  irt::SlotTable slot;         // the slot table (irt_common.h kSlot4; IRT_SLOTS=0: none)
  bool slotAlways = false;     // every launch starts its scan from it (large scenes, IRT_SLOTS=1)
  bool slotLazy = false;       // a smaller scene builds it for a sparse transfer function
  bool slotTried = false;      // a build was attempted (never again)
  bool slotSparse = false;     // the current transfer function is sparse (kSparseTfSamples)
  double tfSamples = 0.0;      // its mean Woodcock samples per acceptance (k_accept_stat)
  double *d_tfStat = nullptr;  // k_accept_stat's sum and count
  size_t binEntries = 0;       // fat entries
  uint32_t numSph = 0;         // zero-thickness records (spheres): distinct radii
  uint32_t numSphRec = 0;      // ... and records
  float *d_sphR = nullptr;
  uint32_t *d_sphOff = nullptr;
  uint2 *d_sphRec = nullptr;
  uint32_t *d_sphBits = nullptr;
  // per-workgroup event counts of the launches in flight, written by the render kernel
  // straight into pinned host memory (kSlots x wgCap x kCnt u32) and summed on the host
  // when a launch's statistics are asked for (finish_slot): no statistics kernel, no
  // same-line atomics per frame.  A slot is rewritten only once its launch is retired.
  uint32_t *h_wgCounts = nullptr, *dh_wgCounts = nullptr;
  size_t wgCap = 0;             // workgroups per slot
  bool lastBlock = false;       // LaunchSlot::block of the previous launch (which zeroed this slot's)
  bool wgCountsOn = true;       // IRT_COUNTERS=atomic: device-scope atomics instead
  bool statsOff = false;        // irt_set_statistics(ctx, 0): no counts at all
  int countersProbe = 0;        // measurement only: IRT_COUNTERS=off (no counts), =device
                                // (per-workgroup stores into device memory, never read)
  uint32_t *d_probeCounts = nullptr;
  size_t probeCap = 0;          // workgroups d_probeCounts holds
  float4 *d_samples = nullptr;   // per-frame colours of a progressive batch
  size_t sampleCap = 0;
  float *d_srgb = nullptr;
  float *d_valueRanges = nullptr;
  float *d_maxOp = nullptr;
  // Value updates (irt_update_values*): the records' clamped shell rectangles as k_shell_build
  // found them (8 B per record; the records themselves are gone after creation), the data
  // range's reduction words (k_shell_rebuild), the marker a device-pointer update leaves on its
  // caller's stream, and whether an update awaits irt_update_values_end
  ushort4 *d_rects = nullptr;
  unsigned long long *d_updStat = nullptr;
  hipEvent_t evUpd = nullptr;
  bool updPending = false;
  // GRID_ACCEL_MODE's 256^3 grid, built on first use (ensure_grid): 201 MB and ~0.16 s at C5
  // that a sphere-mode run never needs
  bool gridBuilt = false;
  uint32_t *d_meta = nullptr;    // per record numLayers (+ quantised keys), for the grid build
  float *d_gridVR = nullptr;     // GRID_ACCEL_MODE: Grid::valueRanges, kGridDim^3 box1f
  float *d_gridMaxOp = nullptr;  // Grid::maxOpacities
  uint32_t *d_gridBits = nullptr;  // its empty-space bitmap (k_grid_bits)
  // CUBQL_MODE wedge locator (irt_build_wedge_accel; irt_internal.h WedgeScene)
  int wG = 0;
  uint32_t *d_wOff = nullptr, *d_wRec = nullptr;
  float4 *d_wBox = nullptr, *d_wTrig = nullptr;
  size_t numMCs = 0;
  float4 *d_lut = nullptr;
  int lutCap = 0;
  int lutSize = 0;
  float tfLo = 0.f, tfHi = 1.f, opScale = 1.f;
  bool tfSet = false;
  // Per-launch statistics, read back without stalling the host: a ring of kSlots launch
  // records (LaunchSlot) and counter blocks; a slot is finished (synchronised) only when it is
  // reused or its statistics are asked for.  The last finished launch is `stats`; every
  // finished launch also adds into `total`.
  static constexpr int kSlots = 32;
  static constexpr int kDoneEvery = 8;  // see LaunchSlot::evDone
  LaunchSlot ring[kSlots];
  long long launches = 0;     // slot of launch i: i % kSlots
  // launches with more workgroups (x frames) than this count through the device-atomic block
  // (the per-workgroup ring would need 1 KiB of pinned memory per workgroup: 256 MiB here)
  static constexpr size_t kWgCountsMax = size_t(1) << 18;
  size_t wgCountsMax = kWgCountsMax;  // IRT_WG_COUNTS_MAX overrides (tests)
  unsigned long long *d_counters = nullptr;  // kSlots x 16
  unsigned long long *d_counterBuckets = nullptr;  // kSlots x kCounterBuckets x 8 (zeroed)
  unsigned long long *h_counters = nullptr;  // pinned, kSlots x 16
  unsigned long long *dh_counters = nullptr; // h_counters as the device sees it
  hipStream_t lastStream = nullptr;  // stream of the previous launch
  // kernel-timing events on every n-th launch only (irt_set_timing_interval): an event
  // pair around every frame costs ~10 us of stream gaps against a 0.17 ms kernel
  int timingEvery = 8;
  float lastMs = 0.f;          // most recent timed launch
  double timedMs = 0.0;        // sum over the timed launches since the last reset
  long long timedLaunches = 0;
  irt_render_stats stats{};
  unsigned long long h_last[16] = {};
  irt_render_stats total{};
  long long totalLaunches = 0;
  size_t bytes = 0;
  // the render-kernel variant (forms->variant: irt_kernels.h OPT_* bits) as its row of the launcher's
  // table: never null, always a compiled variant
  const irt::VariantForms *forms = irt::forms_of(irt::kDefaultVariant);
  // Measured-cost workgroup scheduling of the one-kernel raygen: every launch records its
  // workgroups' durations (d_schedCost); now and then a launch copies them back
  // (h_schedCost, pinned, per launch slot), and once that copy has landed the host
  // orders the frame tiles by descending cost (longest-processing-time first) and uploads
  // the order (d_schedOrder) for later launches with the same grid.
  // Per order buffer (2, ping-pong; sched_stride words each): the block order (cap words), the
  // split packets (kMaxSplit words) and their bitmap (4 cap / 32 words); costs per packet
  // (4 cap words per launch slot)
  uint32_t *d_schedOrder = nullptr, *d_schedCost = nullptr;  // 2 x stride, 4 cap
  uint32_t *h_schedCost = nullptr, *h_schedOrder = nullptr;  // pinned: kSlots x 4 cap, 2 x stride
  uint32_t schedSplit[2] = {0, 0};  // split packets in each order buffer
  uint32_t lastNumSplit = 0;        // the last launch's split work items (parts x packets, padded to 8)
  int splitLg = 2;                  // parts per split packet: 2^splitLg (IRT_SPLIT_LG; 0: no splits)
  float splitFactor = 1.f;          // a packet splits when its cost exceeds this x the frame's ideal span
                                    // (IRT_SPLIT_FACTOR; scenes with holes: kSplitFactorHoles)
  bool splitFixed = false;          // IRT_SPLIT_FACTOR given
  int schedBuf = 0;             // the order buffer launches read now
  long long schedSwitch = 0;    // first launch reading it
  size_t schedCap = 0;
  bool schedOn = false;        // IRT_SCHED=1|2|3 enables (neutral on flat grids since the ramped loop;
                               // on by default, policy 1, for scenes with holes: irt_create_end)
  bool schedFixed = false;     // IRT_SCHED given: scenes keep it
  // cooperative Woodcock loop: a ray's lanes per round <= 2^(coopMaxLg + round) with the
  // ramp, 2^coopMaxLg without (IRT_COOP_MAXLG, IRT_COOP_RAMP; profiles/r02e_dist/)
  int coopMaxLg = 0;
  int coopRamp = 1;
  int probeExit = 0;           // IRT_PROBE_EXIT (measurement only, RenderArgs::probeExit)
  uint32_t *wgTrace = nullptr; // irt_debug_set_wg_trace (measurement only, RenderArgs::wgTrace)
  // chained progressive frames (RenderArgs::chain; IRT_CHAIN=0 / irt_debug_set_chain: the
  // sample buffer + k_accumulate instead): per (block, wave) publish words, the next epoch, and
  // the timeout word
  bool chainOn = true;
  uint32_t *d_chainFlag = nullptr;
  size_t chainCap = 0;           // words in d_chainFlag
  uint32_t chainEpoch = 1;
  // per launch slot, in pinned host memory: set by a chained wait of that launch that gave up
  // (RenderArgs::chainFail); finish_slot reports it (IRT_E_CHAIN) and turns chaining off
  uint32_t *h_chainFail = nullptr, *dh_chainFail = nullptr;
  long long chainFailLaunches = 0;  // launches reported so (irt_debug_chain_errors)
  uint32_t chainSpins = 0;          // irt_debug_set_chain_fault: poll cap (0: the kernel's default)
  int chainWithhold = -1;           // ... and the frame whose waves do not publish (-1: none)
  // irt_render_sequence: the frames' camera words on the device, and per launch slot their
  // pinned staging (a slot is reused only after its launch is retired)
  float4 *d_frameCams = nullptr;
  float4 *h_frameCams = nullptr;
  size_t frameCamCap = 0;        // frames per slot
  // void packets (RenderArgs::voidList; host/irt_void.cpp): the bitmap and the work-item list of the
  // last chained progressive launch's request (computed when the camera, frame, tiles or scene facts
  // change), the list's device copy, and per launch slot the pinned staging an upload goes through
  // (prepare_void)
  irt::VoidCache voidCache;
  uint32_t *d_voidList = nullptr;
  uint32_t *h_voidList = nullptr;
  size_t voidCap = 0;            // words in d_voidList, and per slot of h_voidList
  long long voidOnDevice = 0;    // the cache generation d_voidList holds (0: none)
  bool voidOnDeviceList = false; // ... as the work-item list (else as the bitmap)
  long long lastVoid = 0;        // packets the last launch rendered as void (irt_debug_void_use)
  long long lastInterior = 0;    // ... and flagged interior for its kernel (irt_debug_interior_use)
  long long lastWorkgroups = 0;  // the last launch's raygen grid (irt_debug_last_workgroups)
  irt::RenderPlan lastPlan{};    // ... and its kernel and grid as planned (irt_debug_last_plan)
  // persistent launches (RenderArgs::queue, IRT_QUEUE=0|1): every resident wave pulls 8x8
  // packets from per-slot queue counters (kSlots x kQueueWords u32, zero between launches)
  bool queueOn = false;
  uint32_t *d_queue = nullptr;
  int numCU = 0;
  int queuePerCU = 0;   // IRT_QUEUE_WGS: workgroups per CU of a persistent launch (0: occupancy)
  int lastQueueWG = 0;  // workgroups of the last persistent launch (irt_debug_get_queue)
  int schedPolicy = 2;         // IRT_SCHED: 1 tiles, 2 bands of tiles (a tile row; default), 3 reversed
  bool schedOrderValid = false;
  bool schedLastApplied = false;   // the last launch ran in a measured-cost order
  long long schedApplied = 0;      // launches that did
  long long schedKey[8] = {};
  long long schedSrc = -1;      // launch whose costs the current order came from
  long long schedLastCopy = -1000;
  // Resampling (irt_sample_points / irt_sample_latlon, irt_sample.hip).  The sampling kernels
  // only read the scene, so they stay out of the launch ring (no statistics, no chain state);
  // what must wait for "every launch already issued" also waits for evSample, recorded behind
  // every sampling kernel (wait_samples).  A sampling call on another stream than the previous
  // one's first makes its stream wait for that marker, so the newest marker ends them all.
  hipEvent_t evSample = nullptr;
  bool samplePending = false;       // evSample is recorded and not yet waited for
  hipStream_t sampleStream = nullptr;  // stream of the previous sampling call
  // The sampling calls' tables (irt_sample_latlon: {cos, sin} x numLat, {cos, sin} x numLon, radius x
  // numLevels; irt_column_latlon: the same and the weights; irt_render_column: radii, weights): the
  // device copy the kernel reads and the pinned staging its upload comes from (both grow when a
  // grid needs more floats); evSampleTab, behind the upload, says when the staging is free again
  float *d_sampleTab = nullptr, *h_sampleTab = nullptr;
  size_t sampleTabCap = 0;          // floats in each
  hipEvent_t evSampleTab = nullptr;
  bool sampleTabBusy = false;
  // Overlays (irt_overlay_create, irt_overlay.hip): the device objects this context owns, in the
  // order of their creation; irt_overlay_destroy takes one out, free_overlays the rest
  std::vector<irt_overlay *> overlays;
  // Isolines (irt_contour_grid / irt_contour_latlon, irt_contour.hip): the passes' scratch on the
  // device (tables, thresholds, counts, the packed per-cell counts, the per-workgroup totals), its
  // pinned counterpart (the tables' staging and the counts' landing), and the value / found grid
  // irt_contour_latlon samples into; each grows on demand, behind wait_samples
  void *d_contour = nullptr, *h_contour = nullptr, *d_contourGrid = nullptr;
  size_t contourCap = 0, contourHostCap = 0, contourGridCap = 0;  // bytes
  // streaming creation (irt_create_begin / _append / _end): the cells and their glibc
  // corner trig go to HBM chunk by chunk; the volume facts, column count and sphere
  // records are folded on the host in record order
  bool building = false;
  size_t expected = 0, received = 0;
  // Holes in the volume, folded in record order (append_chunk): columns that start at
  // different radii (convert_icon's first record of a land column starts at R + HSURF, so
  // nothing covers [R, R + HSURF)), or records that leave a gap in their column.  Samples
  // there are outside every cell and come in runs; the raygen's miss mode takes such a run
  // in one cooperative round (irt_render.hip Tracer::kMiss).  A scene without holes runs
  // the variant without it (OPT_NOMISS: 2-3 % faster where nearly every sample is located).
  float bottomMin = INFINITY, bottomMax = -INFINITY;
  bool voids = false;
  bool variantFixed = false;  // IRT_RENDER_VARIANT chose the variant
  irt_icon_cell *d_cells = nullptr;  // freed once the scene is built
  float4 *d_trig = nullptr;          // corner trig: kept for the lazy grid build
  irt::VolumeAcc vacc{};
  size_t numRuns = 0;
  irt_icon_cell last{};
  struct Sphere {
    float r;
    uint32_t rec;
    int32_t nl;
  };
  std::vector<Sphere> sph;  // zero-thickness records
  // device copies of the explicit tile lists / tables of irt_render_tile_list and
  // irt_unpack_tile_table, keyed by content (a multi-GPU deal is fixed for a run: uploaded
  // once, never rewritten while a launch may read it)
  struct TileTable {
    std::vector<int32_t> ids;
    int32_t *dev;
  };
  std::vector<TileTable> tileTables;
};

template <typename T>
int dalloc(irt_context *c, T **p, size_t count) {
  *p = nullptr;
  if (count == 0) count = 1;
  IRT_HIP(hipMalloc((void **)p, count * sizeof(T)));
  c->bytes += count * sizeof(T);
  return IRT_OK;
}

template <typename T>
int upload(irt_context *c, T **p, const T *src, size_t count) {
  int rc = dalloc(c, p, count);
  if (rc) return rc;
  if (count) IRT_HIP(hipMemcpyAsync(*p, src, count * sizeof(T), hipMemcpyHostToDevice, c->stream));
  return IRT_OK;
}

// irt_context.hip
int update_pending(const char *what);  // the error of a call between irt_update_values* and _end
int ensure_grid(irt_context *c);       // GRID_ACCEL_MODE's grid, built on first use
// irt_launch.hip
hipError_t wait_slot(irt_context *c, int i);  // waits for the launch in slot i (pending)
int finish_slot(irt_context *c, int i);       // retires it: its statistics, a chain failure
int finish_stats(irt_context *c);             // ... every pending launch, oldest first
int tile_table(irt_context *c, const int32_t *ids, size_t n, int lo, int total, const int32_t **out);
// irt_sample.hip
hipError_t wait_samples(irt_context *c);  // waits for every sampling call already issued
void free_sample_state(irt_context *c);   // after wait_samples: its events, tables and staging
// irt_overlay.hip
void free_overlays(irt_context *c);       // after wait_samples: every overlay the context still owns
// irt_contour.hip
void free_contour_state(irt_context *c);  // after wait_samples: the isoline passes' scratch

namespace irt {
// irt_launch.hip: what a frame's RenderArgs takes from the launch parameters, the transfer function
// and the caller's buffers -- the camera, accumID and its lerp weight, the ambient terms, the
// classification and the pixel write -- as every render launch fills them (fill_args)
void frame_args(const irt_context *c, const irt_launch_params *lp, uint32_t *fb, irt_vec4f *accum, RenderArgs &A);
// irt_sample.hip: what the sampling calls (irt_sample.hip, irt_levels.hip, irt_column.hip) share on the host.
// scene_args zeroes A and fills the scene side of a sampling launch's arguments; sample_check is
// the checks every sampling call makes before it touches the device; sample_begin takes the call's
// place behind the previous sampling call before anything is queued on `s`, sample_end marks its
// kernel's end
void scene_args(const irt_context *c, int mode, RenderArgs &A);
int sample_check(const irt_context *c, int mode, const char *what);
int sample_begin(irt_context *c, hipStream_t s);
int sample_end(irt_context *c, hipStream_t s);
// ... and the calls that pass tables (d_sampleTab): sample_tab_reserve, after sample_begin, leaves
// the pinned staging free and both copies at least `need` floats long; the call fills the staging;
// sample_tab_upload queues its first `need` floats into the device copy on `s`
int sample_tab_reserve(irt_context *c, size_t need);
int sample_tab_upload(irt_context *c, size_t need, hipStream_t s);
}  // namespace irt
