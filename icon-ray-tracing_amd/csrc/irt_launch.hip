// irt_launch.hip -- the launch side of the C ABI of include/icon_rt_hip.h: the launch ring and
// its statistics, the measured-cost scheduling glue, the growth of the per-context launch
// buffers, render_impl and every irt_render* / irt_unpack_* entry point.

#include <hip/hip_runtime.h>
#include <string.h>

#include <algorithm>
#include <initializer_list>

#include "irt_context.h"

using namespace irt;

// ---------------------------------------------------------------- tile tables

// The device copy of a tile list / table (see irt_context::tileTables): found by content, or
// uploaded (synchronously: a new allocation no launch in flight can be reading).  Entries
// must be in [lo, total).
int tile_table(irt_context *c, const int32_t *ids, size_t n, int lo, int total, const int32_t **out) {
  for (size_t k = 0; k < n; ++k)
    if (ids[k] < lo || ids[k] >= total) {
      set_error("tile id %d at %zu outside [%d, %d)", ids[k], k, lo, total);
      return IRT_E_INVALID;
    }
  for (auto &t : c->tileTables)
    if (t.ids.size() == n && std::equal(t.ids.begin(), t.ids.end(), ids)) {
      *out = t.dev;
      return IRT_OK;
    }
  if (c->tileTables.size() >= 64) {  // a camera per step would re-deal every frame: bounded
    IRT_HIP(hipDeviceSynchronize());
    for (auto &t : c->tileTables) (void)hipFree(t.dev);
    c->tileTables.clear();
  }
  int32_t *d = nullptr;
  IRT_HIP(hipMalloc((void **)&d, std::max<size_t>(n, 1) * sizeof(int32_t)));
  if (hipMemcpy(d, ids, n * sizeof(int32_t), hipMemcpyHostToDevice) != hipSuccess) {
    (void)hipFree(d);
    set_error("tile table upload failed");
    return IRT_E_HIP;
  }
  c->tileTables.push_back({std::vector<int32_t>(ids, ids + n), d});
  *out = d;
  return IRT_OK;
}

// ---------------------------------------------------------------- the launch ring (LaunchSlot)

namespace {
constexpr int kSlots = irt_context::kSlots;

// An event that completes after the launch in slot i (pending): the first marker among that
// launch and the later launches of the same stream, else a marker recorded now behind the
// newest of them.
hipEvent_t done_event(irt_context *c, int i) {
  const LaunchSlot &first = c->ring[i];
  int last = i;
  for (int k = 0; k < kSlots; ++k) {
    const int j = (i + k) % kSlots;
    const LaunchSlot &r = c->ring[j];
    if (!r.pending || r.launch != first.launch + k || r.stream != first.stream) break;
    if (r.marked) return r.evDone;
    last = j;
  }
  LaunchSlot &newest = c->ring[last];
  if (hipEventRecord(newest.evDone, newest.stream) == hipSuccess) {
    newest.marked = true;
    return newest.evDone;
  }
  // that stream is gone (destroyed by the caller after its last launch): wait for the device
  (void)hipGetLastError();
  (void)hipDeviceSynchronize();
  return nullptr;
}
}  // namespace

hipError_t wait_slot(irt_context *c, int i) {
  const hipEvent_t e = done_event(c, i);
  return e ? hipEventSynchronize(e) : hipSuccess;
}

int finish_slot(irt_context *c, int i) {
  LaunchSlot &r = c->ring[i];
  if (!r.pending) return IRT_OK;
  IRT_HIP(wait_slot(c, i));
  float ms = 0.f;
  if (r.timed) {
    IRT_HIP(hipEventElapsedTime(&ms, r.ev0, r.ev1));
    c->lastMs = ms;
    c->timedMs += ms;
    ++c->timedLaunches;
  }
  unsigned long long h[16] = {};
  if (r.block) memcpy(h, c->h_counters + 16 * i, sizeof(h));
  if (r.numWG) {  // the workgroups' counts, from pinned host memory
    const uint32_t *w = c->h_wgCounts + (size_t)i * c->wgCap * kCnt;
    for (size_t b = 0; b < r.numWG; ++b)
      for (int k = 0; k < 5; ++k) h[k] += w[b * kCnt + k];
  }
  irt_render_stats st;
  st.raysLaunched = h[0];
  st.raysInBox = h[1];
  st.locateCalls = h[2];
  st.samplesFound = h[3];
  st.candidatesTested = h[4];
  st.kernelMs = c->lastMs;
  c->stats = st;
  memcpy(c->h_last, h, sizeof(c->h_last));
  c->total.raysLaunched += st.raysLaunched;
  c->total.raysInBox += st.raysInBox;
  c->total.locateCalls += st.locateCalls;
  c->total.samplesFound += st.samplesFound;
  c->total.candidatesTested += st.candidatesTested;
  ++c->totalLaunches;
  r.pending = false;
  if (c->h_chainFail[i]) {
    // a chained wait of this launch gave up: its frames were lerped out of order.  Report it
    // (once), and render later multi-frame launches unchained (sample buffer + k_accumulate)
    c->h_chainFail[i] = 0;
    ++c->chainFailLaunches;
    c->chainOn = false;
    set_error("chained-frame hand-off timed out in launch %lld: its frames are not the sequential "
              "frames (chaining is now off for this context)", r.launch);
    return IRT_E_CHAIN;
  }
  return IRT_OK;
}

// finish every pending launch, oldest first (the last one ends up in c->stats)
int finish_stats(irt_context *c) {
  for (long long j = c->launches - kSlots; j < c->launches; ++j) {
    if (j < 0) continue;
    int rc = finish_slot(c, (int)(j % kSlots));
    if (rc) return rc;
  }
  return IRT_OK;
}

// The frame side of RenderArgs (irt_context.h): shared by every render launch (fill_args) and by
// irt_render_levels (irt_levels.hip), whose kernel runs the raygen's gen_ray, post_classify and
// write_pixel on it
void irt::frame_args(const irt_context *c, const irt_launch_params *lp, uint32_t *fb, irt_vec4f *accum,
                     RenderArgs &A) {
  A.org = make_float3(lp->org.x, lp->org.y, lp->org.z);
  A.dir00 = make_float3(lp->dir_00.x, lp->dir_00.y, lp->dir_00.z);
  A.du = make_float3(lp->dir_du.x, lp->dir_du.y, lp->dir_du.z);
  A.dv = make_float3(lp->dir_dv.x, lp->dir_dv.y, lp->dir_dv.z);
  A.accumID = lp->accumID;
  A.accumW = 1.f / (float)(lp->accumID + 1);  // the lerp weight (deviceCode.cu:333), per launch
  A.amb = make_float3(lp->ambientColor.x, lp->ambientColor.y, lp->ambientColor.z);
  A.ambRad = lp->ambientRadiance;
  A.tfLo = c->tfLo;
  A.tfHi = c->tfHi;
  const float tfSize = c->tfHi - c->tfLo;  // float, as the reference subtracts
  A.invTf = 1.0 / (double)tfSize;
  A.opacityScale = c->opScale;
  A.lut = c->d_lut;
  A.lutSize = c->lutSize;
  A.srgbTh = c->d_srgb;
  A.fb = fb;
  A.accum = (float4 *)accum;
}

namespace {

// ---------------------------------------------------------------- buffer growth

// What must happen before a per-context launch buffer is freed, so that nothing still uses it
enum class Retire {
  None,
  Stream,           // synchronise the launch's stream: only launches queued on it use the buffer
  SlotsThenStream,  // finish_stats (launches on any stream), then synchronise the stream
  Slots,            // finish_stats only: the host reads the buffer when a slot is retired
};
struct GrowBuf {
  void **p;
  size_t (*bytes)(size_t cap);  // its size at a capacity
  bool pinned;                  // host memory (not counted in irt_context::bytes)
};

int release(irt_context *c, std::initializer_list<GrowBuf> bufs, size_t cap) {
  for (const GrowBuf &b : bufs) {
    if (!*b.p) continue;
    IRT_HIP(b.pinned ? hipHostFree(*b.p) : hipFree(*b.p));
    *b.p = nullptr;
    if (!b.pinned) c->bytes -= b.bytes(cap);
  }
  return IRT_OK;
}

// The per-context buffers `bufs`, sized by one capacity *cap, must hold `need` (> *cap): retire
// their users by `rule`, free them and allocate them anew, keeping irt_context::bytes and
// info.deviceBytes right.  On failure the buffers are null and *cap is 0.  With allocFailed, a
// failed allocation is no error: it is flagged there and the call returns IRT_OK.
int grow(irt_context *c, Retire rule, hipStream_t s, size_t *cap, size_t need,
         std::initializer_list<GrowBuf> bufs, bool *allocFailed) {
  int rc;
  if ((rule == Retire::SlotsThenStream || rule == Retire::Slots) && (rc = finish_stats(c))) return rc;
  if (rule == Retire::Stream || rule == Retire::SlotsThenStream) IRT_HIP(hipStreamSynchronize(s));
  if ((rc = release(c, bufs, *cap))) return rc;
  *cap = 0;
  for (const GrowBuf &b : bufs) {
    const size_t n = b.bytes(need);
    hipError_t e = hipSuccess;
    if (b.pinned)
      e = hipHostMalloc(b.p, n);
    else
      rc = dalloc(c, (char **)b.p, n);
    if (e == hipSuccess && !rc) continue;
    if (e != hipSuccess) *b.p = nullptr;
    (void)release(c, bufs, need);
    c->info.deviceBytes = c->bytes;
    if (allocFailed) {
      (void)hipGetLastError();
      *allocFailed = true;
      return IRT_OK;
    }
    return rc ? rc : irt_hip_failed("hipHostMalloc(b.p, n)", e, __FILE__, __LINE__);
  }
  *cap = need;
  c->info.deviceBytes = c->bytes;
  return IRT_OK;
}

// ---------------------------------------------------------------- measured-cost scheduling

// words of one order buffer: the block order, the split list, the split bitmap
size_t sched_stride(size_t cap) { return cap + kMaxSplit + (4 * cap + 31) / 32; }

// Measured-cost scheduling, host side (see irt_context::d_schedOrder): (re)allocate for
// the grid, drop the order when the grid changes, and rebuild it (host/irt_sched.cpp
// sched_order) from the newest landed cost copy of a launch with the same grid.
int sched_prepare(irt_context *c, int numBlocks, int W, int H, int packed, int tileBegin,
                  int tileStride, int numTiles, const irt_launch_params *lp, bool wavewg, hipStream_t s) {
  if ((size_t)numBlocks > c->schedCap) {
    int rc = grow(c, Retire::Stream, s, &c->schedCap, (size_t)numBlocks,
                  {{(void **)&c->d_schedOrder, [](size_t n) { return 2 * sched_stride(n) * sizeof(uint32_t); }, false},
                   {(void **)&c->d_schedCost, [](size_t n) { return 4 * n * sizeof(uint32_t); }, false},
                   {(void **)&c->h_schedCost, [](size_t n) { return kSlots * 4 * n * sizeof(uint32_t); }, true},
                   {(void **)&c->h_schedOrder, [](size_t n) { return 2 * sched_stride(n) * sizeof(uint32_t); }, true}},
                  nullptr);
    if (rc) return rc;
    IRT_HIP(hipMemsetAsync(c->d_schedCost, 0, 4 * (size_t)numBlocks * sizeof(uint32_t), s));
    memset(c->h_schedCost, 0, (size_t)kSlots * 4 * numBlocks * sizeof(uint32_t));
    c->schedSplit[0] = c->schedSplit[1] = 0;
    c->schedOrderValid = false;
    for (LaunchSlot &r : c->ring) r.costsOf = -1;
  }
  const long long key[8] = {numBlocks, W, H, packed, tileBegin, tileStride, numTiles,
                            lp->accelMode * 4 + lp->mode};
  if (memcmp(key, c->schedKey, sizeof(key)) != 0) {
    memcpy(c->schedKey, key, sizeof(key));
    c->schedOrderValid = false;
    c->schedSrc = c->launches;  // costs of launches before this one belong to another grid
    for (LaunchSlot &r : c->ring) r.costsOf = -1;
  }
  // the newest cost copy that has landed -- from a launch no older than the first reader
  // of the current order buffer, so every launch reading the other buffer has finished and
  // it (and its pinned staging copy) may be rewritten without a stall
  long long best = -1;
  int bestSlot = -1;
  for (int i = 0; i < kSlots; ++i) {
    const LaunchSlot &r = c->ring[i];
    if (r.costsOf > c->schedSrc && r.costsOf >= c->schedSwitch && r.costsOf > best &&
        (!r.pending || (r.marked && hipEventQuery(r.evDone) == hipSuccess))) {
      best = r.costsOf;
      bestSlot = i;
    }
  }
  if (bestSlot < 0) return IRT_OK;
  const int nb = c->schedOrderValid ? 1 - c->schedBuf : c->schedBuf;
  const size_t stride = sched_stride(c->schedCap);
  uint32_t *h = c->h_schedOrder + (size_t)nb * stride;
  c->schedSplit[nb] = sched_order(c->h_schedCost + (size_t)bestSlot * 4 * c->schedCap, numBlocks, (W + 63) / 64,
                                  tileStride, c->schedPolicy, c->splitLg, c->splitFactor, c->numCU, wavewg,
                                  c->schedCap, kMaxSplit, h);
  uint32_t *dh = nullptr;
  IRT_HIP(hipHostGetDevicePointer((void **)&dh, h, 0));
  launch_copy_u32(dh, c->d_schedOrder + (size_t)nb * stride, stride, s);
  IRT_HIP(hipGetLastError());
  c->schedBuf = nb;
  c->schedSwitch = c->launches;
  c->schedOrderValid = true;
  c->schedSrc = best;
  return IRT_OK;
}

// ---------------------------------------------------------------- render_impl

// What an entry point asks of render_impl besides the camera and the frame buffers
struct RenderRequest {
  int W, H;
  int packed;                 // 1: the tiles' pixels packed tile after tile, 0: a W x H frame
  int tileBegin, tileStride;  // every tileStride-th 64x64 tile from tileBegin on, or
  const int32_t *tileList;    // ... the listed tiles (irt_render_tile_list; null: no list)
  int listCount;
  int numFrames;                 // progressive frames of one launch
  const irt_launch_params *seq;  // irt_render_sequence: their numFrames views (null: lp for all)
};

// One launch while render_impl puts it together
struct Launch {
  RenderArgs A;
  hipStream_t s;
  int slot;        // of the ring
  int numTiles;
  bool queued;     // a persistent launch ...
  int queueWG;     // ... of this many workgroups
  bool copyCosts;  // its workgroups' durations go to h_schedCost
  RenderPlan plan;  // its kernel and grid (plan_render), once A says which form it takes
  size_t numWG;     // plan.workgroups: the count ring's share, irt_debug_last_workgroups
};

// This launch runs the whole kernel: none of the measurement-only early exits (IRT_PROBE_EXIT
// 1..15), which leave the queue's done count, the chain words and the split parts unserved
bool whole_kernel(const irt_context *c) { return c->probeExit == 0 || c->probeExit >= 16; }

// Frames of one launch can be chained: the cooperative kernels (not the one-lane-per-ray A/B
// variant), grid launches (`queue`: a persistent one), no measurement-only early exit
bool chain_capable(const irt_context *c, bool queue) {
  return c->chainOn && !queue && whole_kernel(c) && (c->forms->variant & OPT_SERIAL) == 0;
}

bool stats_variant(const irt_context *c) { return (c->forms->variant & (OPT_STATS | OPT_TIMING)) != 0; }  // statistics, timing

int validate(const irt_context *c, const irt_launch_params *lp, const RenderRequest &r, const uint32_t *fb,
             const irt_vec4f *accum) {
  if (!c || !lp || r.W <= 0 || r.H <= 0 || !fb || !accum || r.tileStride <= 0 || r.tileBegin < 0 ||
      r.numFrames < 1 || r.numFrames > 65535 || r.listCount < 0 || (r.listCount > 0 && !r.tileList)) {
    set_error("irt_render: bad argument");
    return IRT_E_INVALID;
  }
  if (c->updPending) return update_pending("irt_render");
  if (!c->tfSet) {
    set_error("irt_render: no transfer function set (irt_set_transfunc)");
    return IRT_E_INVALID;
  }
  if (lp->raygen != IRT_RAYGEN_WITH_ACCEL && lp->raygen != IRT_RAYGEN_AE) {
    set_error("irt_render: unknown raygen %d", lp->raygen);
    return IRT_E_INVALID;
  }
  if (lp->accelMode != IRT_ACCEL_SPHERE && lp->accelMode != IRT_ACCEL_GRID) {
    set_error("irt_render: unknown accelMode %d", lp->accelMode);
    return IRT_E_INVALID;
  }
  if (lp->mode != IRT_MODE_USER_GEOM && lp->mode != IRT_MODE_CUBQL &&
      lp->mode != IRT_MODE_TRIANGLES) {
    set_error("irt_render: unknown sampler mode %d", lp->mode);
    return IRT_E_INVALID;
  }
  if (lp->mode != IRT_MODE_USER_GEOM && c->wG == 0 && c->n != 0) {
    set_error("irt_render: sampler mode %d needs irt_build_wedge_accel first (buildCuBQLAccel / "
              "buildTriangleAccel, hostCode.cu:557-649, 440-484)", lp->mode);
    return IRT_E_INVALID;
  }
  return IRT_OK;
}

// the launch's tiles: their count, and the device copy of an explicit list
int resolve_tiles(irt_context *c, const RenderRequest &r, Launch &L) {
  RenderArgs &A = L.A;
  A.tilesX = (r.W + 63) / 64;
  const int total = A.tilesX * ((r.H + 63) / 64);
  L.numTiles = r.tileBegin < total ? (total - r.tileBegin + r.tileStride - 1) / r.tileStride : 0;
  if (r.tileList) {  // irt_render_tile_list
    L.numTiles = r.listCount;
    if (r.listCount > 0) {
      int rc = tile_table(c, r.tileList, (size_t)r.listCount, 0, total, &A.tileList);
      if (rc) return rc;
    }
  }
  A.W = r.W;
  A.H = r.H;
  A.packed = r.packed;
  A.tileBegin = r.tileBegin;
  A.tileStride = r.tileStride;
  A.numTiles = L.numTiles;
  return IRT_OK;
}

// the camera and scene fields of RenderArgs
void fill_args(const irt_context *c, const irt_launch_params *lp, uint32_t *fb, irt_vec4f *accum, Launch &L) {
  RenderArgs &A = L.A;
  frame_args(c, lp, fb, accum, A);
  A.unitDistance = lp->unitDistance;
  A.raygen = lp->raygen;
  const irt_volume_info &I = c->info;
  A.bmin = make_float3(I.bounds.lower.x, I.bounds.lower.y, I.bounds.lower.z);
  A.bmax = make_float3(I.bounds.upper.x, I.bounds.upper.y, I.bounds.upper.z);
  A.dims = make_int3(I.shellDims[0], I.shellDims[1], I.shellDims[2]);
  A.sbLo = make_float3(I.sphericalBounds.lower.x, I.sphericalBounds.lower.y, I.sphericalBounds.lower.z);
  A.sbHi = make_float3(I.sphericalBounds.upper.x, I.sphericalBounds.upper.y, I.sphericalBounds.upper.z);
  A.maxOp = c->d_maxOp;
  A.accelMode = lp->accelMode;
  A.gridMaxOp = c->d_gridMaxOp;
  A.gridBits = c->d_gridBits;
  A.sampler = lp->mode;
  A.wG = c->wG;
  A.wOff = c->d_wOff;
  A.wRec = c->d_wRec;
  A.wBox = c->d_wBox;
  A.wTrig = c->d_wTrig;
  {
    const float sz[3] = {I.sphericalBounds.upper.x - I.sphericalBounds.lower.x,
                         I.sphericalBounds.upper.y - I.sphericalBounds.lower.y,
                         I.sphericalBounds.upper.z - I.sphericalBounds.lower.z};
    for (int k = 0; k < 3; ++k) A.invSb[k] = 1.0 / (double)sz[k];
  }
  A.coopMaxLg = c->coopMaxLg;
  A.coopRamp = c->coopRamp;
  A.probeExit = c->probeExit;
  A.wgTrace = c->wgTrace;
  A.numCells = c->n;
  A.G = c->G;
  A.counters = c->d_counters + 16 * L.slot;
  A.binHdr = c->d_binHdr;
  A.fat = c->d_fat;
  A.blocks = c->d_blocks;
  A.slots = c->slotAlways || c->slotSparse ? c->slot.slots : nullptr;
  A.slotBins = c->slot.bins;
  A.slotSubs = c->slot.subs;
  for (int k = 0; k < 3; ++k) A.slotEdge[k] = c->slot.edges[k];
  A.numSph = c->numSph;
  A.sphR = c->d_sphR;
  A.sphOff = c->d_sphOff;
  A.sphRec = c->d_sphRec;
  A.sphBits = c->d_sphBits;
}

// This launch's ring slot, free, and its place behind the context's previous launch
int claim_slot(irt_context *c, Launch &L) {
  // a launch in flight whose chained wait gave up (its pinned flag is set as it happens):
  // report it now, from the next call, instead of when its slot is retired
  for (int i = 0; i < kSlots; ++i)
    if (c->ring[i].pending && c->h_chainFail[i]) {
      int rc = finish_slot(c, i);
      if (rc) return rc;
    }
  if (c->ring[L.slot].pending) {  // the ring is full: retire that launch (long done by now)
    int rc = finish_slot(c, L.slot);
    if (rc) return rc;
  }
  // Launches of a context run in call order, also across streams: a launch on another stream
  // than the previous one waits for it before anything of this call is queued (the chain words,
  // the frame cameras and the counter block below are shared by every launch of the context;
  // two chained launches in flight at once on two streams would overwrite each other's words)
  hipStream_t s = L.s;
  if (c->launches > 0 && s != c->lastStream) {
    const int prev = (int)((c->launches - 1) % kSlots);
    if (c->ring[prev].pending) {
      const hipEvent_t e = done_event(c, prev);
      if (e) IRT_HIP(hipStreamWaitEvent(s, e, 0));
    }
  }
  c->lastStream = s;
  return IRT_OK;
}

// persistent launch: the cooperative kernels, not for the measurement-only early exits
// (every wave must reach the queue's done count)
void decide_queue(irt_context *c, int numFrames, Launch &L) {
  RenderArgs &A = L.A;
  L.queued = c->queueOn && L.numTiles > 0 && whole_kernel(c) && render_queue_ok(*c->forms, A);
  L.queueWG = 0;
  if (!L.queued) return;
  A.queue = c->d_queue + (size_t)kQueueWords * L.slot;
  A.numPackets = (uint32_t)L.numTiles * 64u * (uint32_t)numFrames;
  L.queueWG = c->queuePerCU > 0 ? std::min(c->queuePerCU * c->numCU, L.numTiles * 16 * numFrames)
                                : render_queue_wgs(*c->forms, c->numCU, L.numTiles * 16 * numFrames);
  c->lastQueueWG = L.queueWG;
}

// measured-cost scheduling: single-frame launches of the one-kernel raygen only
int decide_sched(irt_context *c, const irt_launch_params *lp, const RenderRequest &r, Launch &L) {
  RenderArgs &A = L.A;
  const int numBlocks = L.numTiles * 16;
  L.copyCosts = false;
  if (!(c->schedOn && r.numFrames == 1 && numBlocks > 0 && !A.tileList && !L.queued)) return IRT_OK;
  int rc = sched_prepare(c, numBlocks, r.W, r.H, r.packed, r.tileBegin, r.tileStride, L.numTiles, lp,
                         render_split_ok(*c->forms, A), L.s);
  if (rc) return rc;
  const uint32_t *ob = c->d_schedOrder + (size_t)c->schedBuf * sched_stride(c->schedCap);
  A.schedOrder = c->schedOrderValid ? ob : nullptr;
  if (c->schedOrderValid && c->schedSplit[c->schedBuf] && render_split_ok(*c->forms, A) && whole_kernel(c)) {
    A.splitList = ob + c->schedCap;
    A.splitMask = ob + c->schedCap + kMaxSplit;
    A.numSplit = c->schedSplit[c->schedBuf];
  }
  // every 8th launch writes its workgroups' durations straight into this slot's pinned
  // host copy; the others into device memory nobody reads
  L.copyCosts = c->launches - c->schedLastCopy >= 8;
  if (L.copyCosts) {
    uint32_t *dh = nullptr;
    IRT_HIP(hipHostGetDevicePointer((void **)&dh, c->h_schedCost + (size_t)L.slot * 4 * c->schedCap, 0));
    A.schedCost = dh;
  } else {
    A.schedCost = c->d_schedCost;
  }
  return IRT_OK;
}

// Whether the frames are chained
void decide_chain(const irt_context *c, const RenderRequest &r, Launch &L) {
  RenderArgs &A = L.A;
  // The hand-off's buffer resources address accum with 32-bit byte offsets: frames of 2^27
  // pixels or more (11,585^2) go through the sample buffer instead
  const uint64_t outPixels = r.packed ? (uint64_t)L.numTiles * 4096u : (uint64_t)r.W * (uint64_t)r.H;
  // (decided from whether this launch is in fact queued: see render_sequence)
  A.chain = r.numFrames > 1 && chain_capable(c, L.queued) && outPixels * 16u <= 0x7FFFFFFFull ? 1 : 0;
  A.numSamples = r.numFrames;
}

// Where the launch counts its events: per workgroup in pinned memory (A.wgCounts), in the
// device-atomic block (A.counters alone), or, measurement only, nowhere / in device memory
int choose_counters(irt_context *c, Launch &L) {
  RenderArgs &A = L.A;
  // Per-workgroup counts need kSlots x 32 B of pinned host memory per workgroup and frame
  // (1 KiB): a launch past kWgCountsMax workgroups (a large progressive batch) counts through
  // the device-atomic block instead, for that launch only.
  const bool useWG = c->wgCountsOn && L.numWG <= c->wgCountsMax;
  if (useWG && L.numWG > c->wgCap) {
    // Every slot's launch must be retired before the ring is reallocated.  A huge progressive
    // batch may not get its kSlots x 1 KiB of pinned memory per workgroup and frame -- then the
    // counters go through the device-atomic block from here on (IRT_COUNTERS=atomic), which
    // needs no per-workgroup memory
    bool failed = false;
    int rc = grow(c, Retire::Slots, L.s, &c->wgCap, L.numWG,
                  {{(void **)&c->h_wgCounts, [](size_t n) { return n * kSlots * kCnt * sizeof(uint32_t); }, true}},
                  &failed);
    if (rc) return rc;
    if (!failed && hipHostGetDevicePointer((void **)&c->dh_wgCounts, c->h_wgCounts, 0) != hipSuccess) {
      (void)hipGetLastError();
      (void)hipHostFree(c->h_wgCounts);
      c->h_wgCounts = nullptr;
      c->wgCap = 0;
      failed = true;
    }
    if (failed) {
      c->dh_wgCounts = nullptr;
      c->wgCountsOn = false;
    }
  }
  A.wgCounts = useWG && c->wgCountsOn ? c->dh_wgCounts + (size_t)L.slot * c->wgCap * kCnt : nullptr;
  if (c->countersProbe == 1 || c->statsOff) {
    // measurement only: no counts -- except that the statistics and timing variants add into
    // the counter block unconditionally, so it stays
    A.wgCounts = nullptr;
    if (!stats_variant(c)) A.counters = nullptr;
  } else if (c->countersProbe == 2) {
    if (L.numWG > c->probeCap) {  // per-workgroup stores into device memory: one slot per workgroup
      int rc = grow(c, Retire::Stream, L.s, &c->probeCap, L.numWG,
                    {{(void **)&c->d_probeCounts, [](size_t n) { return n * kCnt * sizeof(uint32_t); }, false}}, nullptr);
      if (rc) return rc;
    }
    A.wgCounts = c->d_probeCounts;
  }
  return IRT_OK;
}

// chained frames: the publish words (one per (block, wave)), this launch's epochs, the timeout word
int setup_chain(irt_context *c, int numFrames, Launch &L) {
  RenderArgs &A = L.A;
  if (!A.chain) return IRT_OK;
  const size_t words = (size_t)L.numTiles * 16 * 4;
  if (words > c->chainCap || c->chainEpoch > 0xF0000000u - (uint32_t)numFrames) {
    if (words > c->chainCap) {
      // every launch that may still read the old words, on any stream
      int rc = grow(c, Retire::SlotsThenStream, L.s, &c->chainCap, words,
                    {{(void **)&c->d_chainFlag, [](size_t n) { return n * sizeof(uint32_t); }, false}}, nullptr);
      if (rc) return rc;
    }
    IRT_HIP(hipMemsetAsync(c->d_chainFlag, 0, c->chainCap * sizeof(uint32_t), L.s));
    c->chainEpoch = 1;  // never 0: the zeroed words match no epoch
  }
  A.chainFlag = c->d_chainFlag;
  c->h_chainFail[L.slot] = 0;
  A.chainFail = c->dh_chainFail + L.slot;
  A.chainSpins = c->chainSpins ? c->chainSpins : kChainSpinsDefault;
  A.chainWithhold = c->chainWithhold;
  A.chainEpoch = c->chainEpoch;
  c->chainEpoch += (uint32_t)numFrames;
  return IRT_OK;
}

// Void packets (RenderArgs::voidList, host/irt_void.cpp): chained progressive frames of one camera
// render the packets that can only ever give the zero colour once per launch, and dispatch no other
// workgroup for them: the launch runs rows of work items (VoidLists) instead of the plain grid
// (plan_render, from the arguments set here).  Only launches that can use the list compute it --
// several chained frames of one camera through the default kernels (render_void_ok), the raygen over the shell's spheres, at
// most 65,535 of them (a grid's rows: a void wave's counts, 64 x numFrames, then fit its 32-bit
// words); not with the chain test hook set
// (its withheld frame must stall every packet), a measurement-only exit or the statistics and
// timing variants (their per-wave figures) -- and the cache computes it only when the same request
// comes a second time (VoidCache::lookup, defer): a progressive sequence once, at its second
// launch (0.4 ms of host time at 1024^2, 0.8 ms at 2048^2 -- DESIGN.md section 5.1 -- against 0.02
// and 0.1 ms saved per launch of 8 frames); a camera that gets one launch, and a new camera with
// single-frame launches, never.  The list does not depend on the number of frames (the rows' void
// parts are dealt from it by index).  The device copy is one buffer, as d_frameCams and d_chainFlag
// are: it is rewritten on the launching stream when the cache has computed a new list (or the launch
// needs the other of list and bitmap), which is behind
// every launch that reads the old one only because a context's launches run in call order, also
// across streams (claim_slot); the upload goes through this launch slot's pinned staging.
int prepare_void(irt_context *c, const irt_launch_params *lp, const RenderRequest &r, Launch &L) {
  RenderArgs &A = L.A;
  c->lastVoid = 0;
  c->lastInterior = 0;
  if (!(A.chain && !r.seq && r.numFrames > 1 && r.numFrames <= 65535 && L.numTiles > 0 &&
        c->chainWithhold < 0 && c->probeExit == 0 && !stats_variant(c) &&
        lp->raygen == IRT_RAYGEN_WITH_ACCEL && lp->accelMode == IRT_ACCEL_SPHERE &&
        render_void_ok(*c->forms, A)))
    return IRT_OK;
  c->voidCache.lookup(void_request(*lp, c->info, r.W, r.H, r.tileBegin, r.tileStride, L.numTiles, r.tileList), true);
  const VoidLists &vl = c->voidCache.lists;
  if (!c->voidCache.count || vl.items.empty()) return IRT_OK;
  // The flat kernel: the work-item list, where its rows are shorter than the plain grid's (in a tiny
  // frame the residues' padding can outweigh the merged packets: 64x64 FRAMING, 64 + 8 against 64) --
  // so no launch has more workgroups than irt_debug_launch_workgroups says.  Every other launch: the
  // bitmap on the plain grid (the terrain kernels always).
  const bool list = c->forms->voidList.fn != nullptr &&
                    (size_t)vl.live + void_row(vl.count, r.numFrames) < (size_t)L.numTiles * 64;
  // the interior class (the same request, computed in the same pass): the list's live items carry it
  // in their top bit, the bitmap form as a second bitmap behind the first
  const size_t words = list ? vl.items.size() : 2 * void_words(L.numTiles);
  if (words > c->voidCap) {
    // every launch that may still read the old words, on any stream, and every slot's staging
    int rc = grow(c, Retire::SlotsThenStream, L.s, &c->voidCap, words,
                  {{(void **)&c->d_voidList, [](size_t n) { return n * sizeof(uint32_t); }, false},
                   {(void **)&c->h_voidList, [](size_t n) { return kSlots * n * sizeof(uint32_t); }, true}},
                  nullptr);
    c->voidOnDevice = 0;
    if (rc) return rc;
  }
  if (c->voidOnDevice != c->voidCache.generation || c->voidOnDeviceList != list) {
    uint32_t *h = c->h_voidList + (size_t)L.slot * c->voidCap;
    if (list) {
      const std::vector<uint32_t> &in = c->voidCache.interior;
      for (size_t k = 0; k < words; ++k) {
        const uint32_t p = vl.items[k];
        h[k] = k < vl.live && p != kVoidEmpty && ((in[p >> 5] >> (p & 31)) & 1u) ? p | kItemInterior : p;
      }
    } else {
      memcpy(h, c->voidCache.bits.data(), words / 2 * sizeof(uint32_t));
      memcpy(h + words / 2, c->voidCache.interior.data(), words / 2 * sizeof(uint32_t));
    }
    c->voidOnDeviceList = list;
    IRT_HIP(hipMemcpyAsync(c->d_voidList, h, words * sizeof(uint32_t), hipMemcpyHostToDevice, L.s));
    c->voidOnDevice = c->voidCache.generation;
  }
  if (list) {
    A.voidList = c->d_voidList;
    A.voidLive = vl.live;
    A.voidRow = void_row(vl.count, r.numFrames);
    A.voidCount = vl.count;
  } else {
    A.voidBits = c->d_voidList;
  }
  A.interior = c->voidCache.interiorCount;
  c->lastVoid = c->voidCache.count;
  c->lastInterior = c->voidCache.interiorCount;
  return IRT_OK;
}

// a sequence of views (irt_render_sequence): frame k's camera and accumID as 4 float4
int stage_sequence(irt_context *c, const RenderRequest &r, Launch &L) {
  RenderArgs &A = L.A;
  if (!r.seq) return IRT_OK;
  if (!A.chain) {
    set_error("irt_render_sequence: needs chained frames (a cooperative variant, IRT_CHAIN on)");
    return IRT_E_INVALID;
  }
  const int numFrames = r.numFrames;
  if ((size_t)numFrames > c->frameCamCap) {
    // every slot's staging retired before it is reallocated
    int rc = grow(c, Retire::SlotsThenStream, L.s, &c->frameCamCap, (size_t)numFrames,
                  {{(void **)&c->d_frameCams, [](size_t n) { return n * 4 * sizeof(float4); }, false},
                   {(void **)&c->h_frameCams, [](size_t n) { return kSlots * n * 4 * sizeof(float4); }, true}},
                  nullptr);
    if (rc) return rc;
  }
  float4 *h = c->h_frameCams + (size_t)L.slot * c->frameCamCap * 4;
  for (int k = 0; k < numFrames; ++k) {
    const irt_launch_params &q = r.seq[k];
    h[4 * k + 0] = make_float4(q.org.x, q.org.y, q.org.z, __builtin_bit_cast(float, q.accumID));
    h[4 * k + 1] = make_float4(q.dir_00.x, q.dir_00.y, q.dir_00.z, 0.f);
    h[4 * k + 2] = make_float4(q.dir_du.x, q.dir_du.y, q.dir_du.z, 0.f);
    h[4 * k + 3] = make_float4(q.dir_dv.x, q.dir_dv.y, q.dir_dv.z, 0.f);
  }
  IRT_HIP(hipMemcpyAsync(c->d_frameCams, h, (size_t)numFrames * 4 * sizeof(float4), hipMemcpyHostToDevice, L.s));
  A.frameCams = c->d_frameCams;
  return IRT_OK;
}

// unchained progressive frames: every frame's colours, for k_accumulate
int ensure_samples(irt_context *c, int numFrames, Launch &L) {
  if (numFrames > 1 && !L.A.chain) {
    const size_t need = (size_t)L.numTiles * 4096 * (size_t)numFrames;
    if (need > c->sampleCap) {
      int rc = grow(c, Retire::Stream, L.s, &c->sampleCap, need,
                    {{(void **)&c->d_samples, [](size_t n) { return n * sizeof(float4); }, false}}, nullptr);
      if (rc) return rc;
    }
  }
  L.A.sampleBuf = c->d_samples;
  return IRT_OK;
}

// queue the launch on its stream and commit its ring slot (LaunchSlot: "launched")
int launch_and_commit(irt_context *c, Launch &L) {
  RenderArgs &A = L.A;
  hipStream_t s = L.s;
  LaunchSlot &r = c->ring[L.slot];
  c->schedLastApplied = A.schedOrder != nullptr;
  c->lastNumSplit = A.numSplit;
  c->lastWorkgroups = L.numTiles > 0 ? (long long)L.numWG : 0;
  c->lastPlan = L.plan;
  c->schedApplied += c->schedLastApplied ? 1 : 0;
  // the 16-counter block (device atomics) is only needed by the statistics variant and the
  // IRT_COUNTERS=atomic mode; it must start zeroed
  // the atomic fallback of the per-workgroup counts adds into this slot's buckets
  A.counterBuckets = A.counters && !A.wgCounts ? c->d_counterBuckets + (size_t)L.slot * kCounterBuckets * 8 : nullptr;
  const bool block = A.counters && (!A.wgCounts || stats_variant(c));
  if (block && !c->lastBlock) IRT_HIP(hipMemsetAsync(A.counters, 0, 16 * sizeof(unsigned long long), s));
  r.timed = c->launches % c->timingEvery == 0;
  if (r.timed) IRT_HIP(hipEventRecord(r.ev0, s));
  if (L.numTiles > 0) launch_render(A, L.plan, s);
  IRT_HIP(hipGetLastError());
  if (r.timed) IRT_HIP(hipEventRecord(r.ev1, s));
  if (block) {
    launch_stats_out(A.counters, c->dh_counters + 16 * L.slot,
                     c->d_counters + 16 * ((c->launches + 1) % kSlots), A.counterBuckets, s);
    IRT_HIP(hipGetLastError());
  }
  r.block = block;
  c->lastBlock = block;
  r.numWG = (A.wgCounts && c->countersProbe == 0 && !c->statsOff && L.numTiles > 0) ? L.numWG : 0;
  r.costsOf = -1;
  if (L.copyCosts) {
    r.costsOf = c->launches;
    c->schedLastCopy = c->launches;
  }
  r.stream = s;
  r.launch = c->launches;
  r.marked = c->launches % irt_context::kDoneEvery == irt_context::kDoneEvery - 1 || L.copyCosts;
  if (r.marked) IRT_HIP(hipEventRecord(r.evDone, s));
  r.pending = true;
  ++c->launches;
  return IRT_OK;
}

int render_impl(irt_context *c, const irt_launch_params *lp, const RenderRequest &r, uint32_t *fb,
                irt_vec4f *accum, int *numTilesOut, void *stream) {
  int rc = validate(c, lp, r, fb, accum);
  if (rc) return rc;
  IRT_HIP(hipSetDevice(c->device));
  if (lp->accelMode == IRT_ACCEL_GRID && (rc = ensure_grid(c))) return rc;
  Launch L;
  memset(&L.A, 0, sizeof(L.A));
  // NULL is the null stream itself (ordered with the caller's blocking streams), never the
  // context's private non-blocking stream
  L.s = (hipStream_t)stream;
  L.slot = (int)(c->launches % kSlots);
  if ((rc = resolve_tiles(c, r, L))) return rc;
  if (numTilesOut) *numTilesOut = L.numTiles;
  fill_args(c, lp, fb, accum, L);
  if ((rc = claim_slot(c, L))) return rc;
  decide_queue(c, r.numFrames, L);
  if ((rc = decide_sched(c, lp, r, L))) return rc;
  decide_chain(c, r, L);
  if ((rc = prepare_void(c, lp, r, L))) return rc;
  // the launch's form is settled: its kernel and grid, which the count ring is sized by
  L.plan = plan_render(*c->forms, L.A, L.queueWG);
  L.numWG = L.plan.workgroups;
  if ((rc = choose_counters(c, L)) || (rc = setup_chain(c, r.numFrames, L)) ||
      (rc = stage_sequence(c, r, L)) ||
      (rc = ensure_samples(c, r.numFrames, L)))
    return rc;
  return launch_and_commit(c, L);
}

// the three forms of a request
RenderRequest whole_frame(int W, int H, int numFrames) { return {W, H, 0, 0, 1, nullptr, 0, numFrames, nullptr}; }
RenderRequest strided_tiles(int W, int H, int tileBegin, int tileStride, int numFrames) {
  return {W, H, 1, tileBegin, tileStride, nullptr, 0, numFrames, nullptr};
}
// (an empty list still is a list: it renders nothing)
RenderRequest listed_tiles(int W, int H, const int32_t *tiles, int numTiles, int numFrames) {
  static const int32_t none = 0;
  return {W, H, 1, 0, 1, numTiles > 0 ? tiles : &none, numTiles, numFrames, nullptr};
}

// irt_render_sequence and its tile-list form: one chained launch, or one launch per view
int render_sequence(irt_context *c, const irt_launch_params *lps, int numFrames, int W, int H,
                    const int32_t *tiles, int numTiles, uint32_t *fb, irt_vec4f *accum, void *stream) {
  if (!c || !lps || numFrames < 1 || numTiles < 0 || (numTiles > 0 && !tiles)) {
    set_error("irt_render_sequence: bad argument");
    return IRT_E_INVALID;
  }
  // only the camera and accumID may change from frame to frame
  const size_t fixed = offsetof(irt_launch_params, ambientColor);
  for (int k = 1; k < numFrames; ++k)
    if (memcmp((const char *)&lps[k] + fixed, (const char *)&lps[0] + fixed, sizeof(irt_launch_params) - fixed)) {
      set_error("irt_render_sequence: frame %d differs from frame 0 in more than the camera and accumID", k);
      return IRT_E_INVALID;
    }
  // Not the decision render_impl makes (decide_chain): here persistent launches being on
  // (queueOn) rules chaining out, there only a launch that is in fact queued does, and there the
  // 2^27-pixel limit applies too.  With queueOn and a launch the queue cannot take, the views
  // therefore go one per launch although one launch could chain them; past the pixel limit the
  // one launch is refused by stage_sequence.  Both outcomes are kept as they are.
  const bool chainable = chain_capable(c, c->queueOn);
  RenderRequest r = tiles ? listed_tiles(W, H, tiles, numTiles, 1) : whole_frame(W, H, 1);
  if (numFrames == 1 || !chainable) {  // one launch per frame
    for (int k = 0; k < numFrames; ++k) {
      int rc = render_impl(c, &lps[k], r, fb, accum, nullptr, stream);
      if (rc) return rc;
    }
    return IRT_OK;
  }
  r.numFrames = numFrames;
  r.seq = lps;
  return render_impl(c, &lps[0], r, fb, accum, nullptr, stream);
}

}  // namespace

// ---------------------------------------------------------------- entry points

extern "C" {

int irt_clear_frame(irt_context *c, uint32_t *fb, irt_vec4f *accum, size_t n, void *stream) {
  if (!c) {
    set_error("irt_clear_frame: null context");
    return IRT_E_INVALID;
  }
  IRT_HIP(hipSetDevice(c->device));
  launch_clear(fb, (float4 *)accum, n, (hipStream_t)stream);
  IRT_HIP(hipGetLastError());
  return IRT_OK;
}

int irt_render(irt_context *c, const irt_launch_params *lp, int W, int H, uint32_t *fb,
               irt_vec4f *accum, void *stream) {
  return render_impl(c, lp, whole_frame(W, H, 1), fb, accum, nullptr, stream);
}

int irt_render_tiles(irt_context *c, const irt_launch_params *lp, int W, int H, int tileBegin,
                     int tileStride, uint32_t *fb, irt_vec4f *accum, int *numTiles,
                     void *stream) {
  return render_impl(c, lp, strided_tiles(W, H, tileBegin, tileStride, 1), fb, accum, numTiles, stream);
}

int irt_render_accumulate(irt_context *c, const irt_launch_params *lp, int W, int H,
                          int numFrames, uint32_t *fb, irt_vec4f *accum, void *stream) {
  return render_impl(c, lp, whole_frame(W, H, numFrames), fb, accum, nullptr, stream);
}

int irt_render_sequence(irt_context *c, const irt_launch_params *lps, int numFrames, int W, int H,
                        uint32_t *fb, irt_vec4f *accum, void *stream) {
  return render_sequence(c, lps, numFrames, W, H, nullptr, 0, fb, accum, stream);
}

int irt_render_tile_list_sequence(irt_context *c, const irt_launch_params *lps, int numFrames, int W, int H,
                                  const int32_t *tiles, int numTiles, uint32_t *fb, irt_vec4f *accum,
                                  void *stream) {
  if (numTiles < 0 || (numTiles > 0 && !tiles)) {
    set_error("irt_render_tile_list_sequence: bad tile list");
    return IRT_E_INVALID;
  }
  static const int32_t none = 0;
  return render_sequence(c, lps, numFrames, W, H, numTiles > 0 ? tiles : &none, numTiles, fb, accum, stream);
}

int irt_render_tiles_accumulate(irt_context *c, const irt_launch_params *lp, int W, int H,
                                int tileBegin, int tileStride, int numFrames, uint32_t *fb,
                                irt_vec4f *accum, int *numTiles, void *stream) {
  return render_impl(c, lp, strided_tiles(W, H, tileBegin, tileStride, numFrames), fb, accum, numTiles, stream);
}

int irt_unpack_tiles(irt_context *c, const uint32_t *g, int numRanks, int maxTiles, int W, int H,
                     uint32_t *fb, void *stream) {
  if (!c || !g || !fb || numRanks <= 0 || maxTiles < 0 || W <= 0 || H <= 0) {
    set_error("irt_unpack_tiles: bad argument");
    return IRT_E_INVALID;
  }
  IRT_HIP(hipSetDevice(c->device));
  if (maxTiles > 0) launch_unpack(g, numRanks, maxTiles, W, H, fb, (hipStream_t)stream);
  IRT_HIP(hipGetLastError());
  return IRT_OK;
}

int irt_render_tile_list(irt_context *c, const irt_launch_params *lp, int W, int H,
                         const int32_t *tiles, int numTiles, int numFrames, uint32_t *fb,
                         irt_vec4f *accum, void *stream) {
  if (numTiles < 0 || (numTiles > 0 && !tiles)) {
    set_error("irt_render_tile_list: bad tile list");
    return IRT_E_INVALID;
  }
  return render_impl(c, lp, listed_tiles(W, H, tiles, numTiles, numFrames), fb, accum, nullptr, stream);
}

int irt_unpack_tile_table(irt_context *c, const uint32_t *g, int numRanks, int maxTiles,
                          const int32_t *table, int W, int H, uint32_t *fb, void *stream) {
  if (!c || !g || !fb || !table || numRanks <= 0 || maxTiles < 0 || W <= 0 || H <= 0) {
    set_error("irt_unpack_tile_table: bad argument");
    return IRT_E_INVALID;
  }
  IRT_HIP(hipSetDevice(c->device));
  if (maxTiles == 0) return IRT_OK;
  const int total = irt_num_tiles(W, H);
  const int32_t *d = nullptr;
  int rc = tile_table(c, table, (size_t)numRanks * (size_t)maxTiles, -1, total, &d);
  if (rc) return rc;
  launch_unpack(g, numRanks, maxTiles, W, H, fb, (hipStream_t)stream, d);
  IRT_HIP(hipGetLastError());
  return IRT_OK;
}

int irt_get_render_stats(const irt_context *cc, irt_render_stats *st) {
  irt_context *c = const_cast<irt_context *>(cc);
  if (!c || !st) {
    set_error("irt_get_render_stats: null argument");
    return IRT_E_INVALID;
  }
  int rc = finish_stats(c);
  if (rc) return rc;
  *st = c->stats;
  return IRT_OK;
}

int irt_get_render_stats_total(const irt_context *cc, irt_render_stats *total, long long *launches) {
  irt_context *c = const_cast<irt_context *>(cc);
  if (!c || !total) {
    set_error("irt_get_render_stats_total: null argument");
    return IRT_E_INVALID;
  }
  int rc = finish_stats(c);
  if (rc) return rc;
  *total = c->total;
  total->kernelMs = c->timedLaunches
                        ? (float)(c->timedMs / (double)c->timedLaunches * (double)c->totalLaunches)
                        : 0.f;
  if (launches) *launches = c->totalLaunches;
  return IRT_OK;
}

int irt_set_timing_interval(irt_context *c, int every) {
  if (!c || every < 1) {
    set_error("irt_set_timing_interval: null context or interval < 1");
    return IRT_E_INVALID;
  }
  c->timingEvery = every;
  return IRT_OK;
}

int irt_set_statistics(irt_context *c, int on) {
  if (!c) {
    set_error("irt_set_statistics: null context");
    return IRT_E_INVALID;
  }
  c->statsOff = on == 0;
  return IRT_OK;
}

int irt_reset_render_stats_total(irt_context *c) {
  if (!c) {
    set_error("irt_reset_render_stats_total: null context");
    return IRT_E_INVALID;
  }
  int rc = finish_stats(c);
  if (rc) return rc;
  c->total = irt_render_stats{};
  c->totalLaunches = 0;
  c->timedMs = 0.0;
  c->timedLaunches = 0;
  return IRT_OK;
}

}  // extern "C"
