// irt_context.hip -- the scene side of the C ABI of include/icon_rt_hip.h on the HIP runtime:
// context lifetime, HBM layout, accelerator builds, transfer function and value updates.  Frame
// launches are in irt_launch.hip, the irt_debug_* hooks in irt_debug_hooks.hip; struct
// irt_context is in irt_context.h.  Host-side preparation (planes, locator, tables) lives in
// host/*.cpp (compiled by g++).

#include <hip/hip_runtime.h>
#include <string.h>

#include <algorithm>
#include <cfloat>
#include <chrono>
#include <cstdio>
#include <thread>
#include <vector>

#include "irt_build.h"
#include "irt_context.h"

using namespace irt;

int irt_hip_failed(const char *call, hipError_t e, const char *file, int line) {
  set_error("%s failed: %s (%s:%d)", call, hipGetErrorString(e), file, line);
  return IRT_E_HIP;
}

// the split threshold of single frames of scenes with holes (irt_context::splitFactor)
constexpr float kSplitFactorHoles = 0.35f;
// A transfer function whose mean Woodcock samples per acceptance over the shell's macrocells
// (k_accept_stat) is at least this is sparse: launches on a scene whose headers fit the
// last-level cache then start their candidate scan from the slot table (built on the first such
// TF), which the dense default TF does not pay for.  Quads on the C3 grid (2.0 GB): the comb TF
// (32 samples per acceptance) -3.8 %, the default TF (1.3) +3.0 % (profiles/r06zl/).
constexpr double kSparseTfSamples = 8.0;

namespace {

void free_all(irt_context *c) {
  if (c->device >= 0) (void)hipSetDevice(c->device);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  (void)wait_samples(c);  // sampling kernels in flight read the arrays freed below
  free_sample_state(c);
  free_overlays(c);
  free_contour_state(c);
  void *ptrs[] = {c->d_binHdr, c->d_fat, c->slot.slots, c->d_blocks, c->d_sphR, c->d_sphOff, c->d_sphRec,
                  c->d_sphBits, c->d_samples, c->d_maxOp, c->d_gridVR, c->d_gridMaxOp, c->d_gridBits, c->d_wOff, c->d_wRec, c->d_wBox, c->d_wTrig, c->d_schedOrder, c->d_schedCost, c->d_srgb, c->d_valueRanges,
                  c->d_lut, c->d_counters, c->d_counterBuckets, c->d_meta, c->d_queue, c->d_chainFlag,
                  c->d_frameCams, c->d_tfStat, c->d_rects, c->d_updStat, c->d_probeCounts, c->d_voidList};
  for (void *p : ptrs)
    if (p) (void)hipFree(p);
  if (c->d_cells) (void)hipFree(c->d_cells);
  if (c->d_trig) (void)hipFree(c->d_trig);
  if (c->h_counters) (void)hipHostFree(c->h_counters);
  if (c->h_wgCounts) (void)hipHostFree(c->h_wgCounts);
  if (c->h_schedCost) (void)hipHostFree(c->h_schedCost);
  if (c->h_schedOrder) (void)hipHostFree(c->h_schedOrder);
  if (c->h_frameCams) (void)hipHostFree(c->h_frameCams);
  if (c->h_chainFail) (void)hipHostFree(c->h_chainFail);
  if (c->h_voidList) (void)hipHostFree(c->h_voidList);
  for (LaunchSlot &r : c->ring) {
    if (r.ev0) (void)hipEventDestroy(r.ev0);
    if (r.ev1) (void)hipEventDestroy(r.ev1);
    if (r.evDone) (void)hipEventDestroy(r.evDone);
  }
  if (c->evUpd) (void)hipEventDestroy(c->evUpd);
  for (auto &t : c->tileTables) (void)hipFree(t.dev);
  c->tileTables.clear();
  if (c->stream) (void)hipStreamDestroy(c->stream);
}

}  // namespace

// between the first irt_update_values* and irt_update_values_end the accelerators are stale
int update_pending(const char *what) {
  set_error("%s: a value update is pending (irt_update_values_end commits it)", what);
  return IRT_E_INVALID;
}

// buildICONGrid (hostCode.cu:668-682: initGrid + buildGrid_ICON over volbounds) on first
// use of GRID_ACCEL_MODE (a render with IRT_ACCEL_GRID, irt_get_grid), from the scene's
// blocks, meta words and corner trig, then the grid's majorants for the current transfer
// function.  The reference builds it in main() whatever the accel mode (hostCode.cu:875);
// the grid is the same whenever it is built.
int ensure_grid(irt_context *c) {
  if (c->gridBuilt) return IRT_OK;
  const size_t gridMCs = (size_t)kGridDim * kGridDim * kGridDim;
  int rc;
  if (!c->d_gridVR && (rc = dalloc(c, &c->d_gridVR, 2 * gridMCs))) return rc;
  if (!c->d_gridMaxOp && (rc = dalloc(c, &c->d_gridMaxOp, gridMCs))) return rc;
  if (!c->d_gridBits && (rc = dalloc(c, &c->d_gridBits, (size_t)kGridBitWords))) return rc;
  IRT_HIP(hipMemsetAsync(c->d_gridBits, 0, kGridBitWords * sizeof(uint32_t), c->stream));
  launch_shell_init(c->d_gridVR, gridMCs, c->stream);  // initGrid(Grid) (hostCode.cu:205-214)
  IRT_HIP(hipMemsetAsync(c->d_gridMaxOp, 0, gridMCs * sizeof(float), c->stream));
  if (c->n) {
    const irt_box3f &vb = c->info.bounds;
    launch_grid_build(c->d_blocks, c->d_meta, c->d_trig, c->n, make_float3(vb.lower.x, vb.lower.y, vb.lower.z),
                      make_float3(vb.upper.x, vb.upper.y, vb.upper.z), c->d_gridVR, c->stream);
  }
  if (c->tfSet) {
    launch_max_opacities(c->d_gridVR, gridMCs, c->d_lut, c->lutSize, c->tfLo, c->tfHi, c->d_gridMaxOp,
                         c->stream);
    launch_grid_bits(c->d_gridMaxOp, c->d_gridBits, c->stream);
  }
  IRT_HIP(hipGetLastError());
  IRT_HIP(hipStreamSynchronize(c->stream));
  c->gridBuilt = true;
  c->info.deviceBytes = c->bytes;
  return IRT_OK;
}

extern "C" {

int irt_create_begin(size_t numCells, int device, irt_context **out) {
  if (!out) {
    set_error("irt_create: null argument");
    return IRT_E_INVALID;
  }
  *out = nullptr;
  if (numCells > 0xFFFFFFF0ull) {
    set_error("too many cells (%zu)", numCells);
    return IRT_E_INVALID;
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
    set_error("irt_create: no HIP device visible (this product has no CPU fallback)");
    return IRT_E_HIP;
  }
  if (device < 0 || device >= ndev) {
    set_error("irt_create: device %d out of range (%d devices)", device, ndev);
    return IRT_E_INVALID;
  }
  irt_context *c = new irt_context();
  c->device = device;
  if (const char *v = getenv("IRT_RENDER_VARIANT")) {
    const int var = atoi(v);
    if (const VariantForms *f = forms_of(var)) {
      c->forms = f;
      c->variantFixed = true;
    }
  }
  auto fail = [&](int code) {
    free_all(c);
    delete c;
    return code;
  };
  if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) {
    set_error("irt_create: cannot initialise device %d", device);
    return fail(IRT_E_HIP);
  }
  if (const char *e = getenv("IRT_SPLIT_LG")) c->splitLg = std::min(3, std::max(0, atoi(e)));
  if (const char *e = getenv("IRT_SPLIT_FACTOR")) {
    c->splitFactor = (float)atof(e);
    c->splitFixed = true;
  }
  if (const char *e = getenv("IRT_SCHED")) {
    c->schedOn = atoi(e) != 0;
    c->schedPolicy = atoi(e);
    c->schedFixed = true;
  }
  // 16 B more than the records: k_shell_build stages them as whole float4, and 284 B records end
  // on a 16-B boundary only for numCells % 4 == 0 (the bytes past the last record are never used)
  if (hipMalloc((void **)&c->d_cells, std::max<size_t>(numCells, 1) * sizeof(irt_icon_cell) + 16) != hipSuccess ||
      hipMalloc((void **)&c->d_trig, std::max<size_t>(numCells, 1) * 3 * sizeof(float4)) != hipSuccess) {
    set_error("irt_create: cannot allocate %zu cells in HBM", numCells);
    return fail(IRT_E_HIP);
  }
  volume_acc_init(c->vacc);
  c->expected = numCells;
  c->building = true;
  *out = c;
  return IRT_OK;
}

namespace {
// One chunk of records: validation, glibc corner trig and getBounds, and the record-order
// folds (volume facts, column count, sphere records), per contiguous slice of records in
// parallel; the slices' partial folds are combined in slice order, which selects the same
// elements as one sequential fold (volume_acc_merge).  Then the cells and their trig go to
// HBM: synchronously from the caller's memory, or, with `trigPinned` (cells already in
// pinned memory, irt_create_synth), asynchronously on the context stream.
int append_chunk(irt_context *c, const irt_icon_cell *cells, size_t n, float *trigPinned) {
  const size_t base = c->received;
  std::vector<float> trigHeap;
  float *trig = trigPinned;
  if (!trig) {
    trigHeap.resize(n * 12);
    trig = trigHeap.data();
  }
  const int threads = n < 4096 ? 1 : default_threads();
  const size_t slice = (n + threads - 1) / threads;
  struct Part {
    VolumeAcc acc;
    size_t runs = 0, bad = SIZE_MAX;
    std::vector<irt_context::Sphere> sph;
    float bottomMin = INFINITY, bottomMax = -INFINITY;  // height[0] of the columns' first records
    bool gap = false;  // a record that does not continue its column (or holds no radius)
  };
  std::vector<Part> part(threads);
  auto work = [&](int t) {
    Part &P = part[t];
    volume_acc_init(P.acc);
    const size_t b = (size_t)t * slice, e = std::min(n, b + slice);
    for (size_t i = b; i < e; ++i) {
      const irt_icon_cell &x = cells[i];
      bool ok = x.numLayers >= 0 && x.numLayers <= 31;
      for (int k = 0; ok && k < 3; ++k) ok = std::isfinite(x.lat[k]) && std::isfinite(x.lon[k]);
      for (int j = 0; ok && j <= x.numLayers; ++j) ok = std::isfinite(x.height[j]);
      if (!ok) {
        P.bad = i;
        return;
      }
      float *tr = &trig[12 * i];
      if (i > b && same_corners(x.lat, x.lon, cells[i - 1].lat, cells[i - 1].lon))
        memcpy(tr, tr - 12, 12 * sizeof(float));  // same column, same corners
      else
        corner_trig(x, tr);
      float lo[3], hi[3];
      cell_bounds(x, tr, lo, hi);
      volume_acc_add(P.acc, x, lo, hi);
      const irt_icon_cell &prev = i ? cells[i - 1] : c->last;
      if (base + i == 0 || !same_corners(x.lat, x.lon, prev.lat, prev.lon)) {
        ++P.runs;
        P.bottomMin = std::min(P.bottomMin, x.height[0]);
        P.bottomMax = std::max(P.bottomMax, x.height[0]);
      } else if (!(x.height[0] == prev.height[prev.numLayers])) {
        P.gap = true;
      }
      if (!(x.height[0] <= x.height[x.numLayers])) P.gap = true;
      if (x.height[0] == x.height[x.numLayers])  // a sphere record
        P.sph.push_back({x.height[0], (uint32_t)(base + i), x.numLayers});
    }
  };
  if (threads == 1) {
    work(0);
  } else {
    std::vector<std::thread> ts;
    for (int t = 0; t < threads; ++t) ts.emplace_back(work, t);
    for (auto &t : ts) t.join();
  }
  size_t bad = SIZE_MAX;
  for (const Part &P : part) bad = std::min(bad, P.bad);
  if (bad != SIZE_MAX) {  // the first bad record, as a sequential check would report
    const irt_icon_cell &x = cells[bad];
    if (x.numLayers < 0 || x.numLayers > 31)
      set_error("cell %zu: numLayers %d outside [0,31] (MAX_LAYERS 32, ICONGrid.h:57)", base + bad, x.numLayers);
    else
      set_error("cell %zu: non-finite lat/lon/height", base + bad);
    return IRT_E_DATA;
  }
  for (const Part &P : part) {
    volume_acc_merge(c->vacc, P.acc);
    c->numRuns += P.runs;
    c->sph.insert(c->sph.end(), P.sph.begin(), P.sph.end());
    c->bottomMin = std::min(c->bottomMin, P.bottomMin);
    c->bottomMax = std::max(c->bottomMax, P.bottomMax);
    c->voids = c->voids || P.gap;
  }
  IRT_HIP(hipSetDevice(c->device));
  if (trigPinned) {
    IRT_HIP(hipMemcpyAsync(c->d_cells + base, cells, n * sizeof(irt_icon_cell), hipMemcpyHostToDevice, c->stream));
    IRT_HIP(hipMemcpyAsync(c->d_trig + 3 * base, trig, n * 12 * sizeof(float), hipMemcpyHostToDevice, c->stream));
  } else {
    IRT_HIP(hipMemcpy(c->d_cells + base, cells, n * sizeof(irt_icon_cell), hipMemcpyHostToDevice));
    IRT_HIP(hipMemcpy(c->d_trig + 3 * base, trig, n * 12 * sizeof(float), hipMemcpyHostToDevice));
  }
  c->last = cells[n - 1];
  c->received += n;
  return IRT_OK;
}
}  // namespace

int irt_create_append(irt_context *c, const irt_icon_cell *cells, size_t n) {
  if (!c || !c->building || (n && !cells)) {
    set_error("irt_create_append: no context being created, or null cells");
    return IRT_E_INVALID;
  }
  if (n > c->expected - c->received) {
    set_error("irt_create_append: %zu more cells than irt_create_begin announced", n - (c->expected - c->received));
    return IRT_E_INVALID;
  }
  if (n == 0) return IRT_OK;
  return append_chunk(c, cells, n, nullptr);
}

// The slot table of a built scene (irt_kernels.h build_slots_device), if its cells share their
// radial edges and it fits: at most IRT_SLOTS_MAX_GB, half the device's memory and its free memory
// less 16 GiB.  Sub-cells per slot unit (irt_common.h slot_unit): by default the finest unit -- 1
// sub-cell, a pair or a quad -- whose table is at most the scene's own bytes (C5: quads, 32 GB
// beside 38.7 GB of headers, entries and blocks); IRT_SLOT_SUBS=1, 2 or 4 asks for one.
int build_slot_table(irt_context *c, bool forced) {
  c->slotTried = true;
  // the kernel's slot index (cell * kSubCells^2 + sub) is 32-bit
  const bool indexable = (uint64_t)6 * c->G * c->G * kSubCells * kSubCells < ((uint64_t)1 << 32);
  int slotSubs = 0;
  if (const char *v = getenv("IRT_SLOT_SUBS")) slotSubs = atoi(v);
  // the scene's own bytes: the locator and the records it indexes (headers, entries, blocks)
  const size_t hdrBytes = (size_t)6 * c->G * c->G * kBinHdrWords * 4;
  const size_t sceneBytes = hdrBytes + c->binEntries * kFatStride4 * 16 + (size_t)c->n * kBlk4 * 16;
  size_t fr = 0, tot = 0;
  IRT_HIP(hipMemGetInfo(&fr, &tot));
  size_t cap = fr > ((size_t)16 << 30) ? fr - ((size_t)16 << 30) : 0;
  cap = std::min(cap, tot / 2);
  if (const char *g = getenv("IRT_SLOTS_MAX_GB")) cap = std::min(cap, (size_t)(atof(g) * (double)(1ull << 30)));
  if (!indexable) {
    c->slot = SlotTable{};
    c->slot.skipped = "the cube map has 2^28 cells or more (32-bit slot index)";
  } else if (int rc = build_slots_device(reinterpret_cast<const uint32_t *>(c->d_binHdr), c->d_fat, 6u * c->G * c->G,
                                         cap, slotSubs, sceneBytes, c->stream, c->slot)) {
    return rc;
  }
  c->bytes += c->slot.bytes;
  c->info.deviceBytes = c->bytes;
  if (c->slot.bytes)
    fprintf(stderr, "icon_rt_hip: slot table built on device %d: %.1f GB of HBM, %d sub-cells per slot (IRT_SLOTS=0: none)\n",
            c->device, c->slot.bytes / 1e9, c->slot.subs);
  else if (forced)
    fprintf(stderr, "icon_rt_hip: IRT_SLOTS=1 but no slot table was built: %s\n",
            c->slot.skipped ? c->slot.skipped : "unknown reason");
  return IRT_OK;
}

namespace {
// the slot table, when the cells share their radial edges, their headers outgrow the
// last-level cache (kSlotAutoHdrBytes) and it fits: at most IRT_SLOTS_MAX_GB, by default half
// the device's memory and never more than its free memory less 16 GiB (a process sharing the
// GPU keeps the rest); IRT_SLOTS=1: whatever the headers' size, 0: none.  Without IRT_SLOTS a
// smaller scene gets it when a sparse transfer function is set (irt_set_transfunc).  A built
// table is announced on stderr with its size; an explicit IRT_SLOTS=1 that builds none says why.
int choose_slot_table(irt_context *c) {
  int rc;
  const char *e = getenv("IRT_SLOTS");
  const bool forced = e && atoi(e) != 0;
  const char *sp = getenv("IRT_SLOTS_SPARSE_TF");  // 0: not for sparse transfer functions either
  c->slotLazy = !e && (!sp || atoi(sp) != 0);
  const size_t hdrBytes = (size_t)6 * c->G * c->G * kBinHdrWords * 4;
  if (e ? forced : hdrBytes > kSlotAutoHdrBytes) {
    if ((rc = build_slot_table(c, forced))) return rc;
    c->slotAlways = c->slot.slots != nullptr;
  }
  return IRT_OK;
}

// zero-thickness records (spheres): sorted by (radius, record) -- see host/irt_scene.cpp
int upload_sphere_table(irt_context *c) {
  int rc;
  std::sort(c->sph.begin(), c->sph.end(), [](const irt_context::Sphere &a, const irt_context::Sphere &b) {
    return a.r < b.r || (a.r == b.r && a.rec < b.rec);
  });
  std::vector<float> R;
  std::vector<uint32_t> off(1, 0u), bits(kSphBitWords, 0u);
  std::vector<uint2> rec;
  for (size_t k = 0; k < c->sph.size(); ++k) {
    if (k == 0 || c->sph[k].r != c->sph[k - 1].r) {
      if (k) off.push_back((uint32_t)rec.size());
      R.push_back(c->sph[k].r);
    }
    rec.push_back(make_uint2(c->sph[k].rec, (uint32_t)c->sph[k].nl));
  }
  if (!c->sph.empty()) off.push_back((uint32_t)rec.size());
  for (float r : R) {
    const uint32_t h = sph_hash(r);
    bits[h >> 5] |= 1u << (h & 31);
  }
  c->numSph = (uint32_t)R.size();
  c->numSphRec = (uint32_t)rec.size();
  if ((rc = upload(c, &c->d_sphR, R.data(), R.size())) || (rc = upload(c, &c->d_sphOff, off.data(), off.size())) ||
      (rc = upload(c, &c->d_sphRec, rec.data(), rec.size())) ||
      (rc = upload(c, &c->d_sphBits, bits.data(), bits.size())))
    return rc;
  IRT_HIP(hipStreamSynchronize(c->stream));
  std::vector<irt_context::Sphere>().swap(c->sph);
  return IRT_OK;
}

// What launches need besides the scene (irt_launch.hip): the counter blocks, the ring's events,
// the chain and queue words, and the IRT_* switches of the launch path
int create_launch_state(irt_context *c) {
  int rc;
  if ((rc = dalloc(c, &c->d_counters, 16 * irt_context::kSlots))) return rc;
  if ((rc = dalloc(c, &c->d_counterBuckets, (size_t)kCounterBuckets * 8 * irt_context::kSlots))) return rc;
  IRT_HIP(hipMemsetAsync(c->d_counterBuckets, 0, (size_t)kCounterBuckets * 8 * irt_context::kSlots * sizeof(unsigned long long),
                         c->stream));
  IRT_HIP(hipHostMalloc((void **)&c->h_counters, 16 * irt_context::kSlots * sizeof(unsigned long long)));
  for (LaunchSlot &r : c->ring) {
    IRT_HIP(hipEventCreate(&r.ev0));
    IRT_HIP(hipEventCreate(&r.ev1));
    // no timestamps: this event only orders the slot's reuse (a timing event's marker costs more)
    IRT_HIP(hipEventCreateWithFlags(&r.evDone, hipEventDisableTiming));
  }
  memset(c->h_counters, 0, 16 * irt_context::kSlots * sizeof(unsigned long long));
  if (const char *e = getenv("IRT_COUNTERS")) {
    c->wgCountsOn = strcmp(e, "atomic") != 0;
    c->countersProbe = strcmp(e, "off") == 0 ? 1 : (strcmp(e, "device") == 0 ? 2 : 0);
  }
  if (const char *e = getenv("IRT_TIMING_EVERY")) c->timingEvery = std::max(1, atoi(e));
  if (const char *e = getenv("IRT_WG_COUNTS_MAX")) c->wgCountsMax = (size_t)std::max(0LL, atoll(e));
  if (const char *e = getenv("IRT_COOP_MAXLG")) c->coopMaxLg = std::min(6, std::max(0, atoi(e)));
  if (const char *e = getenv("IRT_COOP_RAMP")) c->coopRamp = std::min(6, std::max(0, atoi(e)));
  if (const char *e = getenv("IRT_PROBE_EXIT")) c->probeExit = atoi(e);
  if (const char *e = getenv("IRT_QUEUE")) c->queueOn = atoi(e) != 0 && render_queue_compiled();
  if (const char *e = getenv("IRT_QUEUE_WGS")) c->queuePerCU = std::max(0, atoi(e));
  if (const char *e = getenv("IRT_CHAIN")) c->chainOn = atoi(e) != 0;
  IRT_HIP(hipHostMalloc((void **)&c->h_chainFail, irt_context::kSlots * sizeof(uint32_t)));
  memset(c->h_chainFail, 0, irt_context::kSlots * sizeof(uint32_t));
  IRT_HIP(hipHostGetDevicePointer((void **)&c->dh_chainFail, c->h_chainFail, 0));
  if ((rc = dalloc(c, &c->d_queue, (size_t)kQueueWords * irt_context::kSlots))) return rc;
  IRT_HIP(hipMemsetAsync(c->d_queue, 0, (size_t)kQueueWords * irt_context::kSlots * sizeof(uint32_t), c->stream));
  IRT_HIP(hipDeviceGetAttribute(&c->numCU, hipDeviceAttributeMultiprocessorCount, c->device));
  IRT_HIP(hipHostGetDevicePointer((void **)&c->dh_counters, c->h_counters, 0));
  IRT_HIP(hipMemsetAsync(c->d_counters, 0, 16 * irt_context::kSlots * sizeof(unsigned long long), c->stream));
  return IRT_OK;
}

}  // namespace

int irt_create_end(irt_context *c) {
  if (!c || !c->building) {
    set_error("irt_create_end: no context being created");
    return IRT_E_INVALID;
  }
  if (c->received != c->expected) {
    set_error("irt_create_end: %zu of %zu cells appended", c->received, c->expected);
    return IRT_E_INVALID;
  }
  IRT_HIP(hipSetDevice(c->device));
  const size_t numCells = c->expected;
  const bool verbose = getenv("IRT_BUILD_VERBOSE") != nullptr;
  auto t0 = std::chrono::steady_clock::now();
  auto mark = [&](const char *what) {
    if (!verbose) return;
    (void)hipStreamSynchronize(c->stream);
    const auto t = std::chrono::steady_clock::now();
    fprintf(stderr, "[irt create] %-20s %8.1f ms\n", what, std::chrono::duration<double, std::milli>(t - t0).count());
    t0 = t;
  };
  volume_acc_finish(c->vacc, c->info);
  c->n = (uint32_t)numCells;
  const bool holes = c->voids || c->bottomMin < c->bottomMax;
  if (!c->variantFixed && c->forms->variant == kDefaultVariant) c->forms = &render_forms(scene_variant(holes));
  // single frames of a scene with holes: longest 64x64 tiles first, by the durations every 8th
  // launch records (the voids' limb packets run 190-240 us against a 29 us median; C3t -7 %, flat
  // scenes even: profiles/r05r_sched/)
  if (!c->schedFixed && holes) {
    c->schedOn = true;
    c->schedPolicy = 1;
  }
  // ... and their packets longer than 0.35 x the frame's ideal span split (C3t one frame 0.177 ->
  // 0.144 ms against 1.0 x, profiles/r06y/; chained launches never split)
  if (!c->splitFixed && holes) c->splitFactor = kSplitFactorHoles;
  c->G = locator_resolution(c->numRuns);
  // the scene build on the device (irt_build.hip)
  DeviceScene D;
  int rc = build_scene_device(c->d_cells, c->d_trig, numCells, c->numRuns, c->G, c->stream, D);
  c->d_blocks = D.blocks;
  c->d_meta = D.meta;
  c->d_binHdr = D.binHdr;
  c->d_fat = D.fat;
  c->bytes += D.bytes;
  if (rc) return rc;
  c->info.locatorFaceRes = c->G;
  c->info.locatorEntries = D.entries;
  c->binEntries = D.binEntries;
  mark("device scene build");
  if ((rc = choose_slot_table(c))) return rc;
  mark("slot table");
  if ((rc = upload_sphere_table(c))) return rc;
  mark("sphere table");
  float th[256];
  srgb_thresholds(th);
  mark("sRGB thresholds");
  const int dims[3] = {c->info.shellDims[0], c->info.shellDims[1], c->info.shellDims[2]};
  c->numMCs = (size_t)dims[0] * dims[1] * dims[2];
  if ((rc = dalloc(c, &c->d_maxOp, c->numMCs))) return rc;
  IRT_HIP(hipMemsetAsync(c->d_maxOp, 0, c->numMCs * sizeof(float), c->stream));
  if ((rc = upload(c, &c->d_srgb, th, 256))) return rc;
  if ((rc = create_launch_state(c))) return rc;

  // ShellAccel{vec3i(1,1024,1024), sphericalBounds} + initGrid + buildShell_ICON
  // (hostCode.cu:652-666), majorants zero until a transfer function arrives
  // (+ each record's shell rectangle and the reduction words, for irt_update_values_end)
  if ((rc = dalloc(c, &c->d_valueRanges, 2 * c->numMCs))) return rc;
  if ((rc = dalloc(c, &c->d_rects, numCells)) || (rc = dalloc(c, &c->d_updStat, 3))) return rc;
  IRT_HIP(hipEventCreateWithFlags(&c->evUpd, hipEventDisableTiming));
  launch_shell_init(c->d_valueRanges, c->numMCs, c->stream);
  if (numCells) {
    const irt_box3f &sb = c->info.sphericalBounds;
    launch_shell_build(c->d_cells, numCells, make_int3(dims[0], dims[1], dims[2]),
                       make_float3(sb.lower.x, sb.lower.y, sb.lower.z),
                       make_float3(sb.upper.x, sb.upper.y, sb.upper.z), c->d_valueRanges, c->d_rects,
                       c->stream);
  }
  prewarm_render(*c->forms, c->stream);
  IRT_HIP(hipGetLastError());
  IRT_HIP(hipStreamSynchronize(c->stream));
  mark("shell build");
  // the records themselves are not needed again: the GRID_ACCEL_MODE grid, if ever asked
  // for, is built from the blocks, meta words and corner trig (ensure_grid)
  IRT_HIP(hipFree(c->d_cells));
  c->d_cells = nullptr;
  c->bytes += std::max<size_t>(numCells, 1) * 3 * sizeof(float4);  // d_trig, kept
  c->building = false;
  c->info.deviceBytes = c->bytes;
  // Every scene runs the default 5 waves/SIMD.  (Until the 5-wave kernel lost its scratch
  // spills, scenes past 16 GiB ran the 4-wave build: C5 was 1.9 % faster at 4 waves then,
  // and is 2.8 % slower at 4 waves now -- profiles/r03u_waves/, profiles/r03zg_waves/.)
  return IRT_OK;
}

int irt_create(const irt_icon_cell *cells, size_t numCells, int device, irt_context **out) {
  if (!out || (numCells && !cells)) {
    set_error("irt_create: null argument");
    return IRT_E_INVALID;
  }
  irt_context *c = nullptr;
  int rc = irt_create_begin(numCells, device, &c);
  if (rc) return rc;
  if ((rc = irt_create_append(c, cells, numCells)) || (rc = irt_create_end(c))) {
    irt_destroy(c);
    *out = nullptr;
    return rc;
  }
  *out = c;
  return IRT_OK;
}

// streamed creation helpers: records arrive in chunks of kChunk
static constexpr size_t kChunk = size_t(1) << 20;

int irt_create_from_file(const char *path, long maxNumCells, int device, irt_context **out) {
  if (!path || !out) {
    set_error("irt_create_from_file: null argument");
    return IRT_E_INVALID;
  }
  *out = nullptr;
  FILE *f = fopen(path, "rb");
  if (!f) {
    set_error("irt_create_from_file: cannot open %s", path);
    return IRT_E_IO;
  }
  fseek(f, 0, SEEK_END);
  const long size = ftell(f);
  fseek(f, 0, SEEK_SET);
  size_t n = (size_t)size / sizeof(irt_icon_cell);  // hostCode.cu:725
  if (maxNumCells >= 0) n = std::min(n, (size_t)maxNumCells);  // hostCode.cu:728-730
  irt_context *c = nullptr;
  int rc = irt_create_begin(n, device, &c);
  if (rc) {
    fclose(f);
    return rc;
  }
  std::vector<irt_icon_cell> buf(std::min(n, kChunk));
  for (size_t at = 0; at < n && !rc; at += buf.size()) {
    const size_t m = std::min(buf.size(), n - at);
    if (fread(buf.data(), sizeof(irt_icon_cell), m, f) != m) {
      set_error("irt_create_from_file: short read at record %zu", at);
      rc = IRT_E_IO;
      break;
    }
    rc = irt_create_append(c, buf.data(), m);
  }
  fclose(f);
  if (!rc) rc = irt_create_end(c);
  if (rc) {
    irt_destroy(c);
    return rc;
  }
  *out = c;
  return IRT_OK;
}

int irt_create_synth(int rootN, int bisections, int levels, float topHeight, float noise,
                     uint32_t seed, int device, irt_context **out) {
  return irt_create_synth_terrain(rootN, bisections, levels, topHeight, noise, seed, 0.f, device, out);
}

int irt_create_synth_terrain(int rootN, int bisections, int levels, float topHeight, float noise,
                             uint32_t seed, float terrainHeight, int device, irt_context **out) {
  if (!out) {
    set_error("irt_create_synth: null argument");
    return IRT_E_INVALID;
  }
  *out = nullptr;
  void *gen = nullptr;
  size_t n = 0;
  int rc = synth_open(rootN, bisections, levels, topHeight, noise, seed, terrainHeight, &gen, &n);
  if (rc) return rc;
  irt_context *c = nullptr;
  if ((rc = irt_create_begin(n, device, &c))) {
    synth_close(gen);
    return rc;
  }
  // two pinned chunk buffers: chunk k+1 is synthesised and prepared while chunk k's
  // asynchronous upload runs
  const size_t cap = std::max<size_t>(1, std::min(n, kChunk));
  irt_icon_cell *cb[2] = {nullptr, nullptr};
  float *tb[2] = {nullptr, nullptr};
  hipEvent_t ev[2] = {nullptr, nullptr};
  for (int k = 0; k < 2 && !rc; ++k) {
    if (hipHostMalloc((void **)&cb[k], cap * sizeof(irt_icon_cell)) != hipSuccess ||
        hipHostMalloc((void **)&tb[k], cap * 12 * sizeof(float)) != hipSuccess ||
        hipEventCreateWithFlags(&ev[k], hipEventDisableTiming) != hipSuccess) {
      set_error("irt_create_synth: pinned staging buffers");
      rc = IRT_E_HIP;
    }
  }
  size_t k = 0;
  for (size_t at = 0; at < n && !rc; at += cap, ++k) {
    const int b = (int)(k & 1);
    if (k >= 2 && hipEventSynchronize(ev[b]) != hipSuccess) {
      set_error("irt_create_synth: upload failed");
      rc = IRT_E_HIP;
      break;
    }
    const size_t m = std::min(cap, n - at);
    synth_fill(gen, at, m, cb[b]);
    rc = append_chunk(c, cb[b], m, tb[b]);
    if (!rc && hipEventRecord(ev[b], c->stream) != hipSuccess) rc = IRT_E_HIP;
  }
  if (hipStreamSynchronize(c->stream) != hipSuccess && !rc) {
    set_error("irt_create_synth: upload failed");
    rc = IRT_E_HIP;
  }
  for (int q = 0; q < 2; ++q) {
    if (cb[q]) (void)hipHostFree(cb[q]);
    if (tb[q]) (void)hipHostFree(tb[q]);
    if (ev[q]) (void)hipEventDestroy(ev[q]);
  }
  synth_close(gen);
  if (!rc) rc = irt_create_end(c);
  if (rc) {
    irt_destroy(c);
    return rc;
  }
  *out = c;
  return IRT_OK;
}

void irt_destroy(irt_context *c) {
  if (!c) return;
  free_all(c);
  delete c;
}

namespace {
// A sparse transfer function (many samples per acceptance) on a scene whose table is not used by
// every launch starts its launches' scans from the slot table, built on the first such TF
// (irt_context::slotSparse).  Decided from the shell's ranges and majorants for the current
// transfer function: whenever either changes (irt_set_transfunc, irt_update_values_end).
int sparse_tf_decision(irt_context *c) {
  c->slotSparse = false;
  if (!c->slotAlways && (c->slot.slots || (c->slotLazy && !c->slotTried)) && c->numMCs > 0) {
    if (!c->d_tfStat) {  // once per context (a hipFree per TF change would synchronise the device)
      int rc = dalloc(c, &c->d_tfStat, 2);
      if (rc) return rc;
    }
    double h[2] = {0.0, 0.0};
    IRT_HIP(hipMemsetAsync(c->d_tfStat, 0, 2 * sizeof(double), c->stream));
    launch_accept_stat(c->d_valueRanges, c->d_maxOp, c->numMCs, c->d_lut, c->lutSize, c->tfLo, c->tfHi,
                       c->d_tfStat, c->stream);
    IRT_HIP(hipGetLastError());
    IRT_HIP(hipMemcpyAsync(h, c->d_tfStat, sizeof(h), hipMemcpyDeviceToHost, c->stream));
    IRT_HIP(hipStreamSynchronize(c->stream));
    c->tfSamples = h[1] > 0.0 ? h[0] / h[1] : 0.0;
    if (c->tfSamples >= kSparseTfSamples) {
      if (!c->slot.slots && !c->slotTried) {
        int rc = build_slot_table(c, false);
        if (rc) return rc;
      }
      c->slotSparse = c->slot.slots != nullptr;
    }
  }
  return IRT_OK;
}
}  // namespace

int irt_get_volume_info(const irt_context *c, irt_volume_info *info) {
  if (!c || !info) {
    set_error("irt_get_volume_info: null argument");
    return IRT_E_INVALID;
  }
  *info = c->info;
  return IRT_OK;
}

int irt_set_transfunc(irt_context *c, const irt_vec4f *lut, int size, irt_box1f valueRange,
                      float opacityScale) {
  if (!c || !lut || size <= 0) {
    set_error("irt_set_transfunc: bad argument");
    return IRT_E_INVALID;
  }
  if (c->updPending) return update_pending("irt_set_transfunc");
  IRT_HIP(hipSetDevice(c->device));
  // frames still in flight on the caller's stream read the LUT and the majorants: the
  // update is serialized after them, as the reference's TF handler is after its launches
  if (c->launches > 0) {
    const int last = (int)((c->launches - 1) % irt_context::kSlots);
    if (c->ring[last].pending) IRT_HIP(wait_slot(c, last));
  }
  IRT_HIP(wait_samples(c));  // a sparse transfer function may build the slot table they would read
  if (size > c->lutCap) {
    if (c->d_lut) {
      IRT_HIP(hipStreamSynchronize(c->stream));
      IRT_HIP(hipFree(c->d_lut));
      c->bytes -= c->lutCap * sizeof(float4);
      c->d_lut = nullptr;
    }
    int rc = dalloc(c, &c->d_lut, (size_t)size);
    if (rc) return rc;
    c->lutCap = size;
  }
  IRT_HIP(hipMemcpyAsync(c->d_lut, lut, size * sizeof(float4), hipMemcpyHostToDevice, c->stream));
  c->lutSize = size;
  c->tfLo = valueRange.lower;
  c->tfHi = valueRange.upper;
  c->opScale = opacityScale;
  // transfuncUpdateHandler -> computeMaxOpacities (hostCode.cu:878-909); the majorants
  // ignore opacityScale exactly like the reference kernel (hostCode.cu:362-397)
  launch_max_opacities(c->d_valueRanges, c->numMCs, c->d_lut, size, valueRange.lower,
                       valueRange.upper, c->d_maxOp, c->stream);
  if (c->gridBuilt) {  // GRID_ACCEL_MODE's majorants, once its grid exists (ensure_grid)
    launch_max_opacities(c->d_gridVR, (size_t)kGridDim * kGridDim * kGridDim, c->d_lut, size,
                         valueRange.lower, valueRange.upper, c->d_gridMaxOp, c->stream);
    launch_grid_bits(c->d_gridMaxOp, c->d_gridBits, c->stream);
  }
  IRT_HIP(hipGetLastError());
  if (int rc = sparse_tf_decision(c)) return rc;
  IRT_HIP(hipStreamSynchronize(c->stream));
  c->tfSet = true;
  c->info.deviceBytes = c->bytes;
  return IRT_OK;
}

namespace {
// irt_update_values*: the argument checks, and the wait that orders the update after every
// launch of the context already issued (launches run in call order, so the last one's end is
// everyone's), as irt_set_transfunc's
int update_begin(irt_context *c, size_t first, size_t n, const void *values, const char *what) {
  if (!c || c->building || (n && !values) || !update_range_ok(first, n, c ? c->n : 0)) {
    set_error("%s: null context or values, a context still being created, or records [%zu, %zu + %zu) "
              "outside the context's %zu", what, first, first, n, c ? (size_t)c->n : (size_t)0);
    return IRT_E_INVALID;
  }
  IRT_HIP(hipSetDevice(c->device));
  if (c->launches > 0) {
    const int last = (int)((c->launches - 1) % irt_context::kSlots);
    if (c->ring[last].pending) IRT_HIP(wait_slot(c, last));
  }
  IRT_HIP(wait_samples(c));  // sampling calls count as launches: they read the values
  return IRT_OK;
}
// records per staged chunk of a host-pointer update (128 MiB of HBM while the call runs)
constexpr size_t kUpdateChunk = size_t(1) << 20;
}  // namespace

int irt_update_values(irt_context *c, size_t first, size_t n, const float *values) {
  int rc = update_begin(c, first, n, values, "irt_update_values");
  if (rc) return rc;
  c->updPending = true;
  if (n == 0) return IRT_OK;
  float *stage = nullptr;
  const size_t cap = std::min(n, kUpdateChunk);
  IRT_HIP(hipMallocAsync((void **)&stage, cap * 32 * sizeof(float), c->stream));
  hipError_t e = hipSuccess;
  for (size_t at = 0; at < n && e == hipSuccess; at += cap) {
    const size_t m = std::min(cap, n - at);
    // stream order keeps a chunk's copy behind the previous chunk's scatter
    e = hipMemcpyAsync(stage, values + at * 32, m * 32 * sizeof(float), hipMemcpyHostToDevice, c->stream);
    if (e != hipSuccess) break;
    launch_value_scatter(stage, first + at, m, c->d_blocks, c->stream);
    e = hipGetLastError();
  }
  (void)hipFreeAsync(stage, c->stream);
  // the caller's array is free again on return, whatever the runtime does with pageable memory
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e != hipSuccess) {
    set_error("irt_update_values: %s", hipGetErrorString(e));
    return IRT_E_HIP;
  }
  return IRT_OK;
}

int irt_update_values_device(irt_context *c, size_t first, size_t n, const float *d_values, void *stream) {
  int rc = update_begin(c, first, n, d_values, "irt_update_values_device");
  if (rc) return rc;
  c->updPending = true;
  if (n == 0) return IRT_OK;
  hipStream_t s = (hipStream_t)stream;
  // behind the previous device-pointer update, whatever its stream (a marker never recorded
  // holds nothing up): updates apply in call order
  IRT_HIP(hipStreamWaitEvent(s, c->evUpd, 0));
  launch_value_scatter(d_values, first, n, c->d_blocks, s);
  IRT_HIP(hipGetLastError());
  // the commit (and every other update) runs on the context's stream: behind this scatter
  IRT_HIP(hipEventRecord(c->evUpd, s));
  IRT_HIP(hipStreamWaitEvent(c->stream, c->evUpd, 0));
  return IRT_OK;
}

int irt_update_values_end(irt_context *c) {
  if (!c || c->building) {
    set_error("irt_update_values_end: null context, or a context still being created");
    return IRT_E_INVALID;
  }
  if (!c->updPending) return IRT_OK;
  IRT_HIP(hipSetDevice(c->device));
  // initGrid + buildShell_ICON again (hostCode.cu:652-666), from the blocks; the data range with it
  // (the previous commit's pass ended with its stream synchronised: the words are idle)
  const unsigned long long init[3] = {float_key(INFINITY), float_key(-INFINITY), 0ull};
  IRT_HIP(hipMemcpy(c->d_updStat, init, sizeof(init), hipMemcpyHostToDevice));
  launch_shell_init(c->d_valueRanges, c->numMCs, c->stream);
  launch_shell_rebuild(c->d_blocks, c->d_meta, c->d_rects, c->n,
                       make_int3(c->info.shellDims[0], c->info.shellDims[1], c->info.shellDims[2]),
                       c->d_valueRanges, c->d_updStat, c->stream);
  IRT_HIP(hipGetLastError());
  // the majorants for the current transfer function (zero until one is set)
  if (c->tfSet)
    launch_max_opacities(c->d_valueRanges, c->numMCs, c->d_lut, c->lutSize, c->tfLo, c->tfHi, c->d_maxOp,
                         c->stream);
  if (c->gridBuilt) {  // GRID_ACCEL_MODE's grid, if it exists: as ensure_grid built it
    const size_t gridMCs = (size_t)kGridDim * kGridDim * kGridDim;
    launch_shell_init(c->d_gridVR, gridMCs, c->stream);
    if (c->n) {
      const irt_box3f &vb = c->info.bounds;
      launch_grid_build(c->d_blocks, c->d_meta, c->d_trig, c->n, make_float3(vb.lower.x, vb.lower.y, vb.lower.z),
                        make_float3(vb.upper.x, vb.upper.y, vb.upper.z), c->d_gridVR, c->stream);
    }
    if (c->tfSet) {
      launch_max_opacities(c->d_gridVR, gridMCs, c->d_lut, c->lutSize, c->tfLo, c->tfHi, c->d_gridMaxOp,
                           c->stream);
      launch_grid_bits(c->d_gridMaxOp, c->d_gridBits, c->stream);
    }
  }
  IRT_HIP(hipGetLastError());
  if (c->tfSet) {
    if (int rc = sparse_tf_decision(c)) return rc;
  }
  unsigned long long st[3];
  IRT_HIP(hipMemcpyAsync(st, c->d_updStat, sizeof(st), hipMemcpyDeviceToHost, c->stream));
  IRT_HIP(hipStreamSynchronize(c->stream));
  // irt_compute_volume_info's fold of fminf/fmaxf over value[0:numLayers) in record order: the
  // least and greatest value; where that is a zero, the fold (ties to the later argument) ends
  // on the sign of the last zero in record order
  auto unkey = [](unsigned long long k) {
    const uint32_t u = (uint32_t)k;
    return u2f((u & 0x80000000u) ? (u ^ 0x80000000u) : ~u);
  };
  float lo = unkey(st[0]), hi = unkey(st[1]);
  if (st[2]) {
    const float z = ((st[2] - 1ull) & 1ull) ? -0.f : 0.f;
    if (lo == 0.f) lo = z;
    if (hi == 0.f) hi = z;
  }
  c->info.dataRange = {lo, hi};
  c->info.deviceBytes = c->bytes;
  c->updPending = false;
  return IRT_OK;
}

int irt_build_wedge_accel(irt_context *c, const irt_icon_cell *cells, size_t n) {
  if (!c || (n && !cells)) {
    set_error("irt_build_wedge_accel: null argument");
    return IRT_E_INVALID;
  }
  if (n != c->n) {
    set_error("irt_build_wedge_accel: %zu cells, the context has %u", n, c->n);
    return IRT_E_INVALID;
  }
  if (c->wG) return IRT_OK;  // built once per context, like buildCuBQLAccel
  WedgeScene W;
  int rc = build_wedges(cells, n, W);
  if (rc) return rc;
  IRT_HIP(hipSetDevice(c->device));
  if ((rc = upload(c, &c->d_wOff, W.offsets.data(), W.offsets.size())) ||
      (rc = upload(c, &c->d_wRec, W.recs.data(), W.recs.size())) ||
      (rc = upload(c, &c->d_wBox, (const float4 *)W.box.data(), W.box.size() / 4)) ||
      (rc = upload(c, &c->d_wTrig, (const float4 *)W.trig.data(), W.trig.size() / 4)))
    return rc;
  IRT_HIP(hipStreamSynchronize(c->stream));
  c->wG = W.G;
  return IRT_OK;
}

int irt_get_grid(const irt_context *c, float *valueRanges, float *maxOpacities) {
  if (!c) {
    set_error("irt_get_grid: null context");
    return IRT_E_INVALID;
  }
  if (c->updPending) return update_pending("irt_get_grid");
  IRT_HIP(hipSetDevice(c->device));
  // the grid is a cache built on first use: building it changes no observable state
  int rc = ensure_grid(const_cast<irt_context *>(c));
  if (rc) return rc;
  IRT_HIP(hipStreamSynchronize(c->stream));
  const size_t n = (size_t)kGridDim * kGridDim * kGridDim;
  if (valueRanges)
    IRT_HIP(hipMemcpy(valueRanges, c->d_gridVR, 2 * n * sizeof(float), hipMemcpyDeviceToHost));
  if (maxOpacities)
    IRT_HIP(hipMemcpy(maxOpacities, c->d_gridMaxOp, n * sizeof(float), hipMemcpyDeviceToHost));
  return IRT_OK;
}

int irt_get_shell(const irt_context *c, float *valueRanges, float *maxOpacities) {
  if (!c) {
    set_error("irt_get_shell: null context");
    return IRT_E_INVALID;
  }
  if (c->updPending) return update_pending("irt_get_shell");
  IRT_HIP(hipSetDevice(c->device));
  IRT_HIP(hipStreamSynchronize(c->stream));
  if (valueRanges)
    IRT_HIP(hipMemcpy(valueRanges, c->d_valueRanges, 2 * c->numMCs * sizeof(float), hipMemcpyDeviceToHost));
  if (maxOpacities)
    IRT_HIP(hipMemcpy(maxOpacities, c->d_maxOp, c->numMCs * sizeof(float), hipMemcpyDeviceToHost));
  return IRT_OK;
}

}  // extern "C"
