// irt_debug_hooks.hip -- the irt_debug_* entry points of include/icon_rt_hip_debug.h that need a
// device or a context (the host-only ones are in host/irt_debug.cpp), with their kernels.

#include <hip/hip_runtime.h>
#include <string.h>

#include <algorithm>

#include "icon_rt_hip_debug.h"
#include "irt_context.h"
#include "irt_device.h"

using namespace irt;

// ---------------------------------------------------------------- debug (device math)
namespace {
__global__ void k_debug_math(const float *a, const float *y, const float *x, int n, float *oa,
                             float *ot) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  oa[i] = glibc_asinf(a[i]);
  ot[i] = glibc_atan2f(y[i], x[i]);
}
}  // namespace

extern "C" int irt_debug_device_math(int device, const float *a, const float *y, const float *x,
                                     int n, float *oa, float *ot) {
  if (n <= 0 || !a || !y || !x || !oa || !ot) {
    set_error("irt_debug_device_math: bad argument");
    return IRT_E_INVALID;
  }
  IRT_HIP(hipSetDevice(device));
  float *d = nullptr;
  IRT_HIP(hipMalloc((void **)&d, 5 * (size_t)n * sizeof(float)));
  hipError_t e = hipSuccess;
  e = e == hipSuccess ? hipMemcpy(d, a, n * sizeof(float), hipMemcpyHostToDevice) : e;
  e = e == hipSuccess ? hipMemcpy(d + n, y, n * sizeof(float), hipMemcpyHostToDevice) : e;
  e = e == hipSuccess ? hipMemcpy(d + 2 * (size_t)n, x, n * sizeof(float), hipMemcpyHostToDevice) : e;
  if (e == hipSuccess) {
    hipLaunchKernelGGL(k_debug_math, dim3((n + 255) / 256), dim3(256), 0, 0, d, d + n,
                       d + 2 * (size_t)n, n, d + 3 * (size_t)n, d + 4 * (size_t)n);
    e = hipGetLastError();
  }
  e = e == hipSuccess ? hipMemcpy(oa, d + 3 * (size_t)n, n * sizeof(float), hipMemcpyDeviceToHost) : e;
  e = e == hipSuccess ? hipMemcpy(ot, d + 4 * (size_t)n, n * sizeof(float), hipMemcpyDeviceToHost) : e;
  (void)hipFree(d);
  if (e != hipSuccess) {
    set_error("irt_debug_device_math: %s", hipGetErrorString(e));
    return IRT_E_HIP;
  }
  return IRT_OK;
}

namespace {
// Exhaustive error bounds of the certified fast lat/lon (irt_device.h kLatErr / kLonErr),
// as the bit patterns of non-negative doubles (ordered like their values) in out[0..3]:
//   [0] max |fast_asin(x) - glibc_asinf(x)| over every float x in [-1, 1]
//   [1] max |fast_atan(q) - atan(q)|, [2] max |glibc_atanf(q) - atan(q)| over every float q in
//       [0, 2^59] (atan in double)
//   [3] max |rcp(b) b - 1| of the hardware reciprocal over every float b in [2^-100, 2^100]
__device__ __forceinline__ void wave_max_out(unsigned long long *out, double v) {
  unsigned long long b = __double_as_longlong(v);
  for (int off = 32; off > 0; off >>= 1) {
    const unsigned long long o = __shfl_xor(b, off, 64);
    b = o > b ? o : b;
  }
  if (__lane_id() == 0) atomicMax(out, b);
}
__global__ void __launch_bounds__(256) k_fast_math_bounds(unsigned long long *out) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x, stride = gridDim.x * blockDim.x;
  double m0 = 0.0, m1 = 0.0, m2 = 0.0, m3 = 0.0;
  for (uint32_t u = t; u <= 0x3f800000u; u += stride) {
    const float x = __uint_as_float(u);
    const double a = fabs((double)fast_asin(x) - (double)glibc_asinf(x));
    const double b = fabs((double)fast_asin(-x) - (double)glibc_asinf(-x));
    m0 = fmax(m0, fmax(a, b));
    if (!(a == a) || !(b == b)) m0 = __longlong_as_double(0x7ff8000000000000ll);
  }
  for (uint32_t u = t; u <= 0x5d000000u; u += stride) {
    const float q = __uint_as_float(u);
    const double ref = atan((double)q);
    const double a = fabs((double)fast_atan(q) - ref), b = fabs((double)glibc_atanf(q) - ref);
    m1 = (a == a) ? fmax(m1, a) : __longlong_as_double(0x7ff8000000000000ll);
    m2 = (b == b) ? fmax(m2, b) : __longlong_as_double(0x7ff8000000000000ll);
  }
  for (uint32_t u = 0x0d800000u + t; u <= 0x71800000u; u += stride) {
    const float b = __uint_as_float(u);
    m3 = fmax(m3, fabs((double)__builtin_amdgcn_rcpf(b) * (double)b - 1.0));
  }
  wave_max_out(out + 0, m0);
  wave_max_out(out + 1, m1);
  wave_max_out(out + 2, m2);
  wave_max_out(out + 3, m3);
}
}  // namespace

extern "C" int irt_debug_fast_math_bounds(int device, double *out4) {
  if (!out4) {
    set_error("irt_debug_fast_math_bounds: null argument");
    return IRT_E_INVALID;
  }
  IRT_HIP(hipSetDevice(device));
  unsigned long long *d = nullptr;
  IRT_HIP(hipMalloc((void **)&d, 4 * sizeof(unsigned long long)));
  hipError_t e = hipMemset(d, 0, 4 * sizeof(unsigned long long));
  if (e == hipSuccess) {
    hipLaunchKernelGGL(k_fast_math_bounds, dim3(8192), dim3(256), 0, 0, d);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpy(out4, d, 4 * sizeof(double), hipMemcpyDeviceToHost);
  (void)hipFree(d);
  if (e != hipSuccess) {
    set_error("irt_debug_fast_math_bounds: %s", hipGetErrorString(e));
    return IRT_E_HIP;
  }
  return IRT_OK;
}

extern "C" void irt_debug_fast_spherical_consts(float *out2) {
  out2[0] = kLatErr;
  out2[1] = kLonErr;
}

namespace {
__global__ void k_debug_wlog(float *out) {
  __shared__ LogfTab t[16];
  if (threadIdx.x < 16) t[threadIdx.x] = kLogfTab[threadIdx.x];
  __syncthreads();
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  out[j] = woodcock_log(j, t);  // lcg_float uses the low 24 bits only
}
}  // namespace

extern "C" int irt_debug_device_woodcock_log(int device, float *out) {
  if (!out) {
    set_error("irt_debug_device_woodcock_log: null argument");
    return IRT_E_INVALID;
  }
  IRT_HIP(hipSetDevice(device));
  float *d = nullptr;
  const size_t n = (size_t)1 << 24;
  IRT_HIP(hipMalloc((void **)&d, n * sizeof(float)));
  hipLaunchKernelGGL(k_debug_wlog, dim3((unsigned)(n / 256)), dim3(256), 0, 0, d);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipMemcpy(out, d, n * sizeof(float), hipMemcpyDeviceToHost);
  (void)hipFree(d);
  if (e != hipSuccess) {
    set_error("irt_debug_device_woodcock_log: %s", hipGetErrorString(e));
    return IRT_E_HIP;
  }
  return IRT_OK;
}

namespace {
__global__ void k_debug_srgb(const float *th, const float *x, uint32_t *out, int n) {
  __shared__ float s_th[256];
  s_th[threadIdx.x] = th[threadIdx.x];
  __syncthreads();
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j < n) out[j] = srgb_byte(s_th, x[j]);
}
}  // namespace

extern "C" int irt_debug_device_srgb(int device, const float *x, uint32_t *out, int n) {
  if (!x || !out || n < 0) {
    set_error("irt_debug_device_srgb: bad argument");
    return IRT_E_INVALID;
  }
  IRT_HIP(hipSetDevice(device));
  float th[256];
  srgb_thresholds(th);
  float *d = nullptr;
  const size_t m = 256 + 2 * (size_t)n;  // thresholds, x, out
  IRT_HIP(hipMalloc((void **)&d, m * sizeof(float)));
  hipError_t e = hipMemcpy(d, th, sizeof(th), hipMemcpyHostToDevice);
  e = e == hipSuccess ? hipMemcpy(d + 256, x, n * sizeof(float), hipMemcpyHostToDevice) : e;
  if (e == hipSuccess && n > 0) {
    hipLaunchKernelGGL(k_debug_srgb, dim3((n + 255) / 256), dim3(256), 0, 0, d, d + 256,
                       reinterpret_cast<uint32_t *>(d + 256 + n), n);
    e = hipGetLastError();
  }
  e = e == hipSuccess ? hipMemcpy(out, d + 256 + n, n * sizeof(uint32_t), hipMemcpyDeviceToHost) : e;
  (void)hipFree(d);
  if (e != hipSuccess) {
    set_error("irt_debug_device_srgb: %s", hipGetErrorString(e));
    return IRT_E_HIP;
  }
  return IRT_OK;
}

static int debug_locate(irt_context *c, const float *xyz, int n, int *found, float *value, bool wave) {
  if (!c || !xyz || !found || !value || n < 0) {
    set_error("irt_debug_locate: bad argument");
    return IRT_E_INVALID;
  }
  IRT_HIP(hipSetDevice(c->device));
  RenderArgs A;
  memset(&A, 0, sizeof(A));
  A.numCells = c->n;
  A.G = c->G;
  A.binHdr = c->d_binHdr;
  A.fat = c->d_fat;
  A.blocks = c->d_blocks;
  A.slots = c->slot.slots;
  A.slotBins = c->slot.bins;
  A.slotSubs = c->slot.subs;
  for (int k = 0; k < 3; ++k) A.slotEdge[k] = c->slot.edges[k];
  A.numSph = c->numSph;
  A.sphR = c->d_sphR;
  A.sphOff = c->d_sphOff;
  A.sphRec = c->d_sphRec;
  A.sphBits = c->d_sphBits;
  float *d = nullptr;
  IRT_HIP(hipMalloc((void **)&d, (size_t)std::max(n, 1) * 5 * sizeof(float)));
  hipError_t e = hipMemcpy(d, xyz, (size_t)n * 3 * sizeof(float), hipMemcpyHostToDevice);
  int *dFound = reinterpret_cast<int *>(d + 3 * (size_t)n);
  float *dValue = d + 4 * (size_t)n;
  if (e == hipSuccess) {
    launch_debug_locate(A, d, n, dFound, dValue, 0, wave);
    e = hipGetLastError();
  }
  e = e == hipSuccess ? hipMemcpy(found, dFound, (size_t)n * sizeof(int), hipMemcpyDeviceToHost) : e;
  e = e == hipSuccess ? hipMemcpy(value, dValue, (size_t)n * sizeof(float), hipMemcpyDeviceToHost) : e;
  (void)hipFree(d);
  if (e != hipSuccess) {
    set_error("irt_debug_locate: %s", hipGetErrorString(e));
    return IRT_E_HIP;
  }
  return IRT_OK;
}

extern "C" int irt_debug_locate(irt_context *c, const float *xyz, int n, int *found, float *value) {
  return debug_locate(c, xyz, n, found, value, false);
}

extern "C" int irt_debug_locate_wave(irt_context *c, const float *xyz, int n, int *found, float *value) {
  return debug_locate(c, xyz, n, found, value, true);
}

extern "C" int irt_debug_locate_sampler(irt_context *c, int mode, const float *xyz, int n, int *found,
                                        float *value) {
  if (!c || c->building || n < 0 || (n && (!xyz || !found || !value))) {
    set_error("irt_debug_locate_sampler: bad argument");
    return IRT_E_INVALID;
  }
  if (mode != IRT_MODE_CUBQL && mode != IRT_MODE_TRIANGLES) {
    set_error("irt_debug_locate_sampler: sampler mode %d is neither IRT_MODE_CUBQL nor IRT_MODE_TRIANGLES", mode);
    return IRT_E_INVALID;
  }
  if (c->updPending) return update_pending("irt_debug_locate_sampler");
  if (c->wG == 0 && c->n != 0) {
    set_error("irt_debug_locate_sampler: sampler mode %d needs irt_build_wedge_accel first", mode);
    return IRT_E_INVALID;
  }
  if (n == 0) return IRT_OK;
  IRT_HIP(hipSetDevice(c->device));
  RenderArgs A;
  memset(&A, 0, sizeof(A));
  A.numCells = c->n;
  A.sampler = mode;
  A.wG = c->wG;
  A.wOff = c->d_wOff;
  A.wRec = c->d_wRec;
  A.wBox = c->d_wBox;
  A.wTrig = c->d_wTrig;
  A.blocks = c->d_blocks;
  float *d = nullptr;
  IRT_HIP(hipMalloc((void **)&d, (size_t)n * 5 * sizeof(float)));
  hipError_t e = hipMemcpy(d, xyz, (size_t)n * 3 * sizeof(float), hipMemcpyHostToDevice);
  int *dFound = reinterpret_cast<int *>(d + 3 * (size_t)n);
  float *dValue = d + 4 * (size_t)n;
  if (e == hipSuccess) {
    launch_debug_locate_sampler(A, d, n, dFound, dValue, 0);
    e = hipGetLastError();
  }
  e = e == hipSuccess ? hipMemcpy(found, dFound, (size_t)n * sizeof(int), hipMemcpyDeviceToHost) : e;
  e = e == hipSuccess ? hipMemcpy(value, dValue, (size_t)n * sizeof(float), hipMemcpyDeviceToHost) : e;
  (void)hipFree(d);
  if (e != hipSuccess) {
    set_error("irt_debug_locate_sampler: %s", hipGetErrorString(e));
    return IRT_E_HIP;
  }
  return IRT_OK;
}

extern "C" int irt_debug_sched(irt_context *c, int *policy, int *lastApplied, long long *applied) {
  if (!c || !policy || !lastApplied || !applied) {
    set_error("irt_debug_sched: null argument");
    return IRT_E_INVALID;
  }
  *policy = c->schedOn ? c->schedPolicy : 0;
  *lastApplied = c->schedLastApplied ? 1 : 0;
  *applied = c->schedApplied;
  return IRT_OK;
}

extern "C" int irt_debug_counters(irt_context *c, unsigned long long *out16) {
  if (!c || !out16) {
    set_error("irt_debug_counters: null argument");
    return IRT_E_INVALID;
  }
  int rc = finish_stats(c);
  if (rc) return rc;
  memcpy(out16, c->h_last, 16 * sizeof(unsigned long long));
  return IRT_OK;
}

extern "C" int irt_debug_default_variant(void) { return kDefaultVariant; }
// 1 when the context's launches start their candidate scan from the slot table (the OPT_SLOT
// kernels), 0 otherwise; -1 without a context.  *tfSamples (if given): the current transfer
// function's mean Woodcock samples per acceptance (k_accept_stat; 0 when not computed).
extern "C" int irt_debug_slot_use(const irt_context *c, double *tfSamples) {
  if (!c) return -1;
  if (tfSamples) *tfSamples = c->tfSamples;
  return c->slot.slots && (c->slotAlways || c->slotSparse) ? 1 : 0;
}

extern "C" long long irt_debug_void_use(const irt_context *c) { return c ? c->lastVoid : -1; }
extern "C" long long irt_debug_interior_use(const irt_context *c) { return c ? c->lastInterior : -1; }
extern "C" long long irt_debug_last_workgroups(const irt_context *c) { return c ? c->lastWorkgroups : -1; }

extern "C" int irt_debug_context_array(const irt_context *c, int which, void *dst, size_t capacity,
                                       size_t *bytes) {
  if (!c || !bytes || c->building) {
    set_error("irt_debug_context_array: null argument or context not built");
    return IRT_E_INVALID;
  }
  const void *src = nullptr;
  size_t n = 0;
  switch (which) {
    case IRT_DEBUG_ARRAY_BIN_HDR: src = c->d_binHdr; n = (size_t)6 * c->G * c->G * kBinHdrWords * 4; break;
    case IRT_DEBUG_ARRAY_FAT: src = c->d_fat; n = c->binEntries * kFatStride4 * 16; break;
    case IRT_DEBUG_ARRAY_BLOCKS: src = c->d_blocks; n = (size_t)c->n * kBlk4 * 16; break;
    case IRT_DEBUG_ARRAY_SPH_R: src = c->d_sphR; n = (size_t)c->numSph * 4; break;
    case IRT_DEBUG_ARRAY_SPH_OFF: src = c->d_sphOff; n = c->numSph ? ((size_t)c->numSph + 1) * 4 : 4; break;
    case IRT_DEBUG_ARRAY_SPH_REC: src = c->d_sphRec; n = (size_t)c->numSphRec * 8; break;
    case IRT_DEBUG_ARRAY_SPH_BITS: src = c->d_sphBits; n = (size_t)kSphBitWords * 4; break;
    case IRT_DEBUG_ARRAY_SLOTS: src = c->slot.slots; n = c->slot.bytes; break;
    case IRT_DEBUG_ARRAY_GRID_BITS: src = c->d_gridBits; n = c->gridBuilt ? (size_t)kGridBitWords * 4 : 0; break;
    default:
      set_error("irt_debug_context_array: unknown array %d", which);
      return IRT_E_INVALID;
  }
  *bytes = n;
  if (dst && capacity >= n && n) {
    IRT_HIP(hipSetDevice(c->device));
    IRT_HIP(hipStreamSynchronize(c->stream));
    IRT_HIP(hipMemcpy(dst, src, n, hipMemcpyDeviceToHost));
  }
  return IRT_OK;
}

extern "C" int irt_debug_get_variant(const irt_context *c) { return c ? c->forms->variant : -1; }

extern "C" int irt_debug_variants(int *out, int capacity) { return render_variants(out, capacity); }

extern "C" int irt_debug_set_queue(irt_context *c, int on) {
  if (!c) {
    set_error("irt_debug_set_queue: null context");
    return IRT_E_INVALID;
  }
  if (on && !render_queue_compiled()) {
    set_error("irt_debug_set_queue: persistent launches are compiled into the A/B library only "
              "(make VARIANTS=all, libicon_rt_hip_all.so)");
    return IRT_E_INVALID;
  }
  c->queueOn = on != 0;
  return IRT_OK;
}

extern "C" int irt_debug_set_wg_trace(irt_context *c, uint32_t *trace) {
  if (!c) {
    set_error("irt_debug_set_wg_trace: null context");
    return IRT_E_INVALID;
  }
  c->wgTrace = trace;
  return IRT_OK;
}

extern "C" long long irt_debug_launch_workgroups(const irt_context *c, int numTiles, int numFrames) {
  if (!c || numTiles < 0 || numFrames < 1) {
    set_error("irt_debug_launch_workgroups: bad argument");
    return -1;
  }
  return irt_debug_variant_workgroups(c->forms->variant, c->schedOn ? 1 : 0, numTiles, numFrames);
}

extern "C" long long irt_debug_variant_workgroups(int variant, int sched, int numTiles, int numFrames) {
  if (numTiles < 0 || numFrames < 1) {
    set_error("irt_debug_variant_workgroups: bad argument");
    return -1;
  }
  // the user-geometry sphere path's plain grid (no other path has more workgroups)
  const int per = 256 / render_forms(variant).plain.threads;
  // a single frame in measured-cost order may add its work items (at most kMaxSplit workgroups);
  // allowed for with every one-wave-workgroup variant, also those without a split form
  const size_t extra = sched && numFrames == 1 && per == 4 ? (size_t)kMaxSplit : 0;
  return (long long)((size_t)numTiles * 16 * per * numFrames + extra);
}

namespace {
int plan_out(const RenderPlan &P, int out[5]) {
  out[0] = P.form.id;
  out[1] = P.form.threads;
  out[2] = (int)P.grid.x;
  out[3] = (int)P.grid.y;
  out[4] = P.accumBlocks;
  return IRT_OK;
}
}  // namespace

extern "C" int irt_debug_plan(int variant, int sampler, int accelMode, int flags, int numTiles, int numFrames,
                              uint32_t numSplit, uint32_t voidLive, uint32_t voidRow, int queueWG, int out[5]) {
  const VariantForms *F = forms_of(variant);
  if (!F || !out || numTiles < 0 || numFrames < 1) {
    set_error("irt_debug_plan: variant %d not compiled, or bad argument", variant);
    return IRT_E_INVALID;
  }
  alignas(16) static uint32_t set[4];  // what a flag's pointer points to (plan_render reads none of them)
  RenderArgs A;
  memset(&A, 0, sizeof(A));
  A.sampler = sampler;
  A.accelMode = accelMode;
  A.numTiles = numTiles;
  A.numSamples = numFrames;
  A.numSplit = numSplit;
  A.voidLive = voidLive;
  A.voidRow = voidRow;
  if (flags & IRT_DEBUG_PLAN_SLOTS) A.slots = reinterpret_cast<const float4 *>(set);
  if (flags & IRT_DEBUG_PLAN_VOID_BITS) A.voidBits = set;
  if (flags & IRT_DEBUG_PLAN_VOID_LIST) A.voidList = set;
  if (flags & IRT_DEBUG_PLAN_QUEUE) A.queue = set;
  A.chain = (flags & IRT_DEBUG_PLAN_CHAIN) ? 1 : 0;
  return plan_out(plan_render(*F, A, queueWG), out);
}

extern "C" int irt_debug_last_plan(const irt_context *c, int out[5]) {
  if (!c || !out) {
    set_error("irt_debug_last_plan: null argument");
    return IRT_E_INVALID;
  }
  return plan_out(c->lastPlan, out);
}

extern "C" int irt_debug_sched_split(const irt_context *c, int *numSplit, int *splitLg) {
  if (!c || !numSplit || !splitLg) {
    set_error("irt_debug_sched_split: null argument");
    return IRT_E_INVALID;
  }
  *numSplit = (int)c->lastNumSplit;
  *splitLg = c->splitLg;
  return IRT_OK;
}

extern "C" int irt_debug_set_chain(irt_context *c, int on) {
  if (!c) {
    set_error("irt_debug_set_chain: null context");
    return IRT_E_INVALID;
  }
  c->chainOn = on != 0;
  return IRT_OK;
}

extern "C" int irt_debug_chain_errors(irt_context *c) {
  if (!c) {
    set_error("irt_debug_chain_errors: null context");
    return -1;
  }
  // retire every launch in flight (each reported hand-off failure is counted, not returned)
  for (long long j = c->launches - irt_context::kSlots; j < c->launches; ++j) {
    if (j < 0) continue;
    const int rc = finish_slot(c, (int)(j % irt_context::kSlots));
    if (rc && rc != IRT_E_CHAIN) return -1;
  }
  return (int)c->chainFailLaunches;
}

extern "C" int irt_debug_set_chain_fault(irt_context *c, uint32_t spins, int withholdFrame) {
  if (!c) {
    set_error("irt_debug_set_chain_fault: null context");
    return IRT_E_INVALID;
  }
  c->chainSpins = spins;
  c->chainWithhold = withholdFrame;
  return IRT_OK;
}

extern "C" int irt_debug_get_queue(const irt_context *c) { return c ? (c->queueOn ? 1 : 0) : -1; }

extern "C" int irt_debug_queue_wgs(const irt_context *c) { return c ? c->lastQueueWG : -1; }

extern "C" int irt_debug_set_variant(irt_context *c, int variant) {
  const VariantForms *f = forms_of(variant);
  if (!c || !f) {
    set_error("irt_debug_set_variant: variant %d not compiled", variant);
    return IRT_E_INVALID;
  }
  c->forms = f;
  return IRT_OK;
}
