// irt_sample.hip -- resampling (include/icon_rt_hip.h, "resampling"): the field's value at given
// points and on a regular lat x lon x level grid, through the raygen's own point location
// (irt_tracer.h: Tracer::locate_wave for the cell sampler, Tracer<kSamplerVariant>::locate for the
// wedge and triangle samplers) -- sampleVolume (deviceCode.cu:58-125) without a ray around it.
// The kernels, their launch and ordering glue, and the two context entry points; the host side
// (the grid's trig rows, irt_latlon_points, the guard's host compilation) is host/irt_latlon.cpp.
//
// The guard in front of the locator (admit) and sampleVolume of a wave's points (wave_locate) are
// in irt_sample_dev.h, which irt_levels.hip shares; so are this file's scene_args, sample_check,
// sample_begin and sample_end (declared in irt_context.h).

#include <hip/hip_runtime.h>
#include <string.h>

#include <algorithm>

#include "irt_build.h"
#include "irt_context.h"
#include "irt_sample_dev.h"

namespace irt {

// What the sampling kernels need beyond RenderArgs (which stays the kernels' FIRST argument:
// Tracer's late reads go through fresh_args(), the kernarg segment read as a RenderArgs).
struct SampleArgs {
  const float *xyz;      // k_sample_points: 3 floats per point
  const float *latCS;    // k_sample_latlon: {cosf lat, sinf lat} per row ...
  const float *lonCS;    // ... {cosf lon, sinf lon} per column ...
  const float *radius;   // ... and the levels' radii
  int numLat, numLon, numLevels;
  uint32_t patchesLat, patchesLon;  // 8 x 8 patches per level (the patch form)
  unsigned long long n;  // points (k_sample_points) or patches (k_sample_latlon)
  float *value;
  uint8_t *found;        // may be null
  float missValue;
  float rLo, rHi;        // the scene's sphericalBounds.lower.x / upper.x (cell sampler's cut)
};

// The scene side of a sampling launch's arguments (what debug_locate* fill for the hooks)
void scene_args(const irt_context *c, int mode, RenderArgs &A) {
  memset(&A, 0, sizeof(A));
  A.numCells = c->n;
  A.sampler = mode;
  A.blocks = c->d_blocks;
  if (mode == IRT_MODE_USER_GEOM) {
    A.G = c->G;
    A.binHdr = c->d_binHdr;
    A.fat = c->d_fat;
    A.slots = c->slotAlways || c->slotSparse ? c->slot.slots : nullptr;  // as the frames (launch_args)
    A.slotBins = c->slot.bins;
    A.slotSubs = c->slot.subs;
    for (int k = 0; k < 3; ++k) A.slotEdge[k] = c->slot.edges[k];
    A.numSph = c->numSph;
    A.sphR = c->d_sphR;
    A.sphOff = c->d_sphOff;
    A.sphRec = c->d_sphRec;
    A.sphBits = c->d_sphBits;
  } else {
    A.wG = c->wG;
    A.wOff = c->d_wOff;
    A.wRec = c->d_wRec;
    A.wBox = c->d_wBox;
    A.wTrig = c->d_wTrig;
  }
}

// The checks every sampling call makes before it touches the device
int sample_check(const irt_context *c, int mode, const char *what) {
  if (!c || c->building) {
    set_error("%s: null context, or a context still being created", what);
    return IRT_E_INVALID;
  }
  if (mode != IRT_MODE_USER_GEOM && mode != IRT_MODE_CUBQL && mode != IRT_MODE_TRIANGLES) {
    set_error("%s: sampler mode %d is none of IRT_MODE_USER_GEOM, IRT_MODE_CUBQL, IRT_MODE_TRIANGLES", what,
              mode);
    return IRT_E_INVALID;
  }
  if (c->updPending) return update_pending(what);
  if (mode != IRT_MODE_USER_GEOM && c->wG == 0 && c->n != 0) {  // (an empty scene has nothing to list)
    set_error("%s: sampler mode %d needs irt_build_wedge_accel first", what, mode);
    return IRT_E_INVALID;
  }
  return IRT_OK;
}

// Before a sampling call queues anything on `s`: its place behind the previous sampling call
int sample_begin(irt_context *c, hipStream_t s) {
  IRT_HIP(hipSetDevice(c->device));
  if (!c->evSample) IRT_HIP(hipEventCreateWithFlags(&c->evSample, hipEventDisableTiming));
  if (c->samplePending && s != c->sampleStream) IRT_HIP(hipStreamWaitEvent(s, c->evSample, 0));
  c->sampleStream = s;
  return IRT_OK;
}
// ... and after its kernel
int sample_end(irt_context *c, hipStream_t s) {
  IRT_HIP(hipGetLastError());
  IRT_HIP(hipEventRecord(c->evSample, s));
  c->samplePending = true;
  return IRT_OK;
}

// The sampling calls' tables (irt_context.h d_sampleTab): before a call fills the pinned staging
// with `need` floats -- the previous call's upload has left it, and both copies hold that many,
// grown on demand
int sample_tab_reserve(irt_context *c, size_t need) {
  int rc;
  if (!c->evSampleTab) IRT_HIP(hipEventCreateWithFlags(&c->evSampleTab, hipEventDisableTiming));
  if (c->sampleTabBusy) {  // the previous call's upload still reads the staging
    IRT_HIP(hipEventSynchronize(c->evSampleTab));
    c->sampleTabBusy = false;
  }
  if (need > c->sampleTabCap) {
    IRT_HIP(wait_samples(c));  // an earlier grid's kernel may still read the device copy
    if (c->d_sampleTab) {
      IRT_HIP(hipFree(c->d_sampleTab));
      c->d_sampleTab = nullptr;
      c->bytes -= c->sampleTabCap * sizeof(float);
    }
    if (c->h_sampleTab) {
      IRT_HIP(hipHostFree(c->h_sampleTab));
      c->h_sampleTab = nullptr;
    }
    c->sampleTabCap = 0;
    c->info.deviceBytes = c->bytes;
    const size_t cap = std::max<size_t>(need + need / 2, 4096);
    IRT_HIP(hipHostMalloc((void **)&c->h_sampleTab, cap * sizeof(float)));
    if ((rc = dalloc(c, &c->d_sampleTab, cap))) return rc;  // (the staging stays, with capacity 0: the next
                                                            // call frees it and allocates both anew)
    c->sampleTabCap = cap;
    c->info.deviceBytes = c->bytes;
  }
  return IRT_OK;
}
// ... and after it: the staging's first `need` floats into the device copy on `s`, behind every
// earlier sampling kernel (same stream: stream order; another: sample_begin's wait)
int sample_tab_upload(irt_context *c, size_t need, hipStream_t s) {
  IRT_HIP(hipMemcpyAsync(c->d_sampleTab, c->h_sampleTab, need * sizeof(float), hipMemcpyHostToDevice, s));
  IRT_HIP(hipEventRecord(c->evSampleTab, s));
  c->sampleTabBusy = true;
  return IRT_OK;
}

namespace {

// One located point's outputs: streaming stores (nobody re-reads them in this kernel), as the
// raygen's last frame stores its pixels.
__device__ __forceinline__ void put(const SampleArgs &S, unsigned long long i, bool hit, float v) {
  __builtin_nontemporal_store(hit ? v : S.missValue, &S.value[i]);
  if (S.found) __builtin_nontemporal_store((uint8_t)(hit ? 1 : 0), &S.found[i]);
}

// One lane per point, 64 consecutive points per one-wave workgroup.
template <int O>
__global__ void __launch_bounds__(64) k_sample_points(RenderArgs A, SampleArgs S) {
  __shared__ SampleLds<(O & OPT_WEDGE) == 0> L;
  const unsigned long long w = workgroup_index();
  if (w * 64ull >= S.n) return;  // wave-uniform (the last grid row's tail)
  const unsigned long long i = w * 64ull + threadIdx.x;
  const bool live = i < S.n;
  float x = 0.f, y = 0.f, z = 0.f;
  if (live) {
    x = S.xyz[3 * i];
    y = S.xyz[3 * i + 1];
    z = S.xyz[3 * i + 2];
  }
  float v = 0.f;
  const bool hit = wave_locate<O>(A, S.rLo, S.rHi, live, x, y, z, v, L);
  if (live) put(S, i, hit, v);
}

// The lat x lon x level grid, its points made from the three tables exactly as
// to_cartesian_trig (irt_build.h) makes them; no xyz array exists.  A wave takes an 8 x 8
// lat x lon patch of one level (lane = 8 * dlat + dlon), the shape of the raygen's packet:
// neighbouring lanes share header lines, fat entries and height/value blocks.  S.n = patches;
// patch w = (level, patch row, patch column).
template <int O>
__global__ void __launch_bounds__(64) k_sample_latlon(RenderArgs A, SampleArgs S) {
  __shared__ SampleLds<(O & OPT_WEDGE) == 0> L;
  const unsigned long long w = workgroup_index();
  if (w >= S.n) return;  // wave-uniform
  const unsigned long long perLevel = (unsigned long long)S.patchesLat * S.patchesLon;
  const unsigned long long k = w / perLevel;  // < numLevels: w < S.n = numLevels * perLevel
  const unsigned long long q = w - k * perLevel;
  const unsigned long long j = (q / S.patchesLon) * 8ull + (threadIdx.x >> 3);
  const unsigned long long i = (q % S.patchesLon) * 8ull + (threadIdx.x & 7u);
  // live lanes index the tables inside their sizes: j < numLat, i < numLon
  const bool live = j < (unsigned long long)S.numLat && i < (unsigned long long)S.numLon;
  float x = 0.f, y = 0.f, z = 0.f;
  if (live) {
    const float r = S.radius[k];
    const float t[4] = {S.latCS[2 * j], S.latCS[2 * j + 1], S.lonCS[2 * i], S.lonCS[2 * i + 1]};
    to_cartesian_trig(r, t, x, y, z);
  }
  float v = 0.f;
  const bool hit = wave_locate<O>(A, S.rLo, S.rHi, live, x, y, z, v, L);
  if (live) put(S, (k * (unsigned long long)S.numLat + j) * (unsigned long long)S.numLon + i, hit, v);
}

template <int O>
void launch_points(const RenderArgs &A, const SampleArgs &S, hipStream_t s) {
  hipLaunchKernelGGL(k_sample_points<O>, sample_grid((S.n + 63ull) / 64ull), dim3(64), 0, s, A, S);
}
template <int O>
void launch_latlon(const RenderArgs &A, const SampleArgs &S, hipStream_t s) {
  hipLaunchKernelGGL(k_sample_latlon<O>, sample_grid(S.n), dim3(64), 0, s, A, S);
}

void launch_sample(const irt_context *c, int mode, const RenderArgs &A, const SampleArgs &S, bool latlon,
                   hipStream_t s) {
  if (mode != IRT_MODE_USER_GEOM) {
    latlon ? launch_latlon<kSamplerVariant>(A, S, s) : launch_points<kSamplerVariant>(A, S, s);
  } else if (A.slots) {
    latlon ? launch_latlon<kCellVariant | OPT_SLOT>(A, S, s) : launch_points<kCellVariant | OPT_SLOT>(A, S, s);
  } else {
    latlon ? launch_latlon<kCellVariant>(A, S, s) : launch_points<kCellVariant>(A, S, s);
  }
}

}  // namespace
}  // namespace irt

using namespace irt;

hipError_t wait_samples(irt_context *c) {
  if (!c->samplePending) return hipSuccess;
  const hipError_t e = hipEventSynchronize(c->evSample);
  if (e == hipSuccess) c->samplePending = false;
  return e;
}

void free_sample_state(irt_context *c) {
  if (c->sampleTabBusy) (void)hipEventSynchronize(c->evSampleTab);
  if (c->d_sampleTab) (void)hipFree(c->d_sampleTab);
  if (c->h_sampleTab) (void)hipHostFree(c->h_sampleTab);
  if (c->evSample) (void)hipEventDestroy(c->evSample);
  if (c->evSampleTab) (void)hipEventDestroy(c->evSampleTab);
  c->d_sampleTab = c->h_sampleTab = nullptr;
  c->evSample = c->evSampleTab = nullptr;
  c->sampleTabCap = 0;
  c->samplePending = c->sampleTabBusy = false;
}

extern "C" {

int irt_sample_points(irt_context *c, int mode, const float *d_xyz, size_t n, float *d_value, uint8_t *d_found,
                      float missValue, void *stream) {
  int rc = sample_check(c, mode, "irt_sample_points");
  if (rc) return rc;
  if ((uint64_t)n > kSampleMaxPoints) {
    set_error("irt_sample_points: %zu points are more than 2^36 (or a negative count)", n);
    return IRT_E_INVALID;
  }
  if (n && (!d_xyz || !d_value)) {
    set_error("irt_sample_points: null d_xyz or d_value");
    return IRT_E_INVALID;
  }
  if (n == 0) return IRT_OK;
  hipStream_t s = (hipStream_t)stream;
  if ((rc = sample_begin(c, s))) return rc;
  RenderArgs A;
  scene_args(c, mode, A);
  SampleArgs S;
  memset(&S, 0, sizeof(S));
  S.xyz = d_xyz;
  S.n = n;
  S.value = d_value;
  S.found = d_found;
  S.missValue = missValue;
  S.rLo = c->info.sphericalBounds.lower.x;
  S.rHi = c->info.sphericalBounds.upper.x;
  launch_sample(c, mode, A, S, false, s);
  return sample_end(c, s);
}

int irt_sample_latlon(irt_context *c, int mode, const float *lat, int numLat, const float *lon, int numLon,
                      const float *radius, int numLevels, float *d_value, uint8_t *d_found, float missValue,
                      void *stream) {
  int rc = sample_check(c, mode, "irt_sample_latlon");
  if (rc) return rc;
  size_t total = 0;
  if ((rc = latlon_args("irt_sample_latlon", lat, numLat, lon, numLon, radius, numLevels, &total))) return rc;
  if (total && !d_value) {
    set_error("irt_sample_latlon: null d_value");
    return IRT_E_INVALID;
  }
  if (total == 0) return IRT_OK;
  hipStream_t s = (hipStream_t)stream;
  if ((rc = sample_begin(c, s))) return rc;
  // the tables: through the context's pinned staging into its device copy
  const size_t need = 2 * (size_t)numLat + 2 * (size_t)numLon + (size_t)numLevels;
  if ((rc = sample_tab_reserve(c, need))) return rc;
  float *latCS = c->h_sampleTab, *lonCS = latCS + 2 * (size_t)numLat, *rad = lonCS + 2 * (size_t)numLon;
  latlon_trig(lat, numLat, lon, numLon, latCS, lonCS);
  memcpy(rad, radius, (size_t)numLevels * sizeof(float));
  if ((rc = sample_tab_upload(c, need, s))) return rc;

  RenderArgs A;
  scene_args(c, mode, A);
  SampleArgs S;
  memset(&S, 0, sizeof(S));
  S.latCS = c->d_sampleTab;
  S.lonCS = S.latCS + 2 * (size_t)numLat;
  S.radius = S.lonCS + 2 * (size_t)numLon;
  S.numLat = numLat;
  S.numLon = numLon;
  S.numLevels = numLevels;
  S.patchesLat = ((uint32_t)numLat + 7u) / 8u;
  S.patchesLon = ((uint32_t)numLon + 7u) / 8u;
  S.n = (unsigned long long)numLevels * S.patchesLat * S.patchesLon;
  S.value = d_value;
  S.found = d_found;
  S.missValue = missValue;
  S.rLo = c->info.sphericalBounds.lower.x;
  S.rHi = c->info.sphericalBounds.upper.x;
  launch_sample(c, mode, A, S, true, s);
  return sample_end(c, s);
}

}  // extern "C"
