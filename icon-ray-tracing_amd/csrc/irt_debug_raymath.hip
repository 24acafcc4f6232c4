// irt_debug_raymath.hip -- the irt_debug_* entry points of include/icon_rt_hip_debug.h that run the
// raygen's per-value arithmetic one value at a time (tests/test_gpu_raymath.py): the two division
// shortcuts (irt_device.h div_uniform, recip_d / div_recip), classification (irt_tracer.h
// Tracer::post_classify, classify_alpha), the ray tests (box_test, intersect_sphere,
// intersect_spheres, intersect_spheres_interior), gen_ray (irt_raygen.h) and the shell grid's
// coordinates (project_axis_inv, wrap_coord).  The kernels call the raygen's own inline functions,
// compiled with the raygen's flags (Makefile RENDER_FLAGS).
//
// Every kernel takes RenderArgs as its FIRST argument, by value: Tracer's late reads go through
// fresh_args(), the kernarg segment read as a RenderArgs.  The kernels that reach opaque_u (a
// readfirstlane: classification, the grid coordinates, the divisions' kernel for symmetry) keep
// every lane to the end -- the tail wave's lanes past n compute on a harmless input and store
// nothing; k_debug_ray_tests and k_debug_gen_ray call nothing wave-wide and let those lanes return.

#include <hip/hip_runtime.h>
#include <string.h>

#include <vector>

#include "icon_rt_hip_debug.h"
#include "irt_context.h"
#include "irt_raygen.h"
#include "irt_sample_dev.h"

namespace irt {
namespace {

__global__ void __launch_bounds__(256) k_debug_div(RenderArgs A, const float *a, const float *b, const double *invB,
                                                   int n, float *outUniform, float *outRecip) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  const bool live = i < n;
  const float x = live ? a[i] : 0.f, y = live ? b[i] : 1.f;
  const double inv = live ? invB[i] : 1.0;
  const float u = div_uniform(x, inv, y);
  const float r = recip_ok(y) ? div_recip(x, y, recip_d(y)) : x / y;
  if (live) {
    outUniform[i] = u;
    outRecip[i] = r;
  }
}

__global__ void __launch_bounds__(256) k_debug_classify(RenderArgs A, const float *v, int n, float4 *out,
                                                        float *alpha) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  const bool live = i < n;
  const float x = live ? v[i] : 0.f;
  Tracer<kCellVariant> T{{}, A, nullptr, A.sphBits, nullptr, {0, 0, 0, 0, 0, 0, 0}};
  const float4 c = T.post_classify(x);
  const float w = T.classify_alpha(x);
  if (live) {
    out[i] = c;
    alpha[i] = w;
  }
}

// per ray: org, dir (6 floats) -> flags and 14 floats {box t0 t1, sphere A near far, sphere B near
// far, intersect_spheres A near far B near far, intersect_spheres_interior A near far B near far};
// what a test leaves unwritten (a miss, an interior form not run) reads 0
__global__ void __launch_bounds__(256) k_debug_ray_tests(RenderArgs A, const float *rays, const uint8_t *interior,
                                                         int n, float rA, float rB, int32_t *flags, float *out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float *p = rays + 6 * (size_t)i;
  const Ray ray = {p[0], p[1], p[2], 0.f, p[3], p[4], p[5], 1e10f};
  float o[14];
  for (int k = 0; k < 14; ++k) o[k] = 0.f;
  int32_t f = 0;
  f |= box_test(ray, A, o[0], o[1]) ? IRT_DEBUG_RAY_BOX : 0;
  f |= intersect_sphere(ray, rA, o[2], o[3]) ? IRT_DEBUG_RAY_SPHERE_A : 0;
  f |= intersect_sphere(ray, rB, o[4], o[5]) ? IRT_DEBUG_RAY_SPHERE_B : 0;
  bool hA, hB;
  intersect_spheres(ray, rA, rB, hA, o[6], o[7], hB, o[8], o[9]);
  f |= (hA ? IRT_DEBUG_RAY_SPHERES_A : 0) | (hB ? IRT_DEBUG_RAY_SPHERES_B : 0);
  if (interior[i]) {
    intersect_spheres_interior(ray, rA, rB, o[10], o[11], o[12], o[13]);
    f |= IRT_DEBUG_RAY_INTERIOR;
  }
  flags[i] = f;
  for (int k = 0; k < 14; ++k) out[14 * (size_t)i + k] = o[k];
}

__global__ void __launch_bounds__(64) k_debug_gen_ray(RenderArgs A, float *dir, uint32_t *state) {
  const int x = blockIdx.x * 8 + (threadIdx.x & 7), y = blockIdx.y * 8 + (threadIdx.x >> 3);
  if (x >= A.W || y >= A.H) return;
  uint32_t st;
  float dx, dy, dz;
  gen_ray(A, A.accumID, x, y, st, dx, dy, dz);
  const size_t p = (size_t)x + (size_t)A.W * (size_t)y;
  dir[3 * p] = dx;
  dir[3 * p + 1] = dy;
  dir[3 * p + 2] = dz;
  state[p] = st;
}

__global__ void __launch_bounds__(256) k_debug_grid_coord(RenderArgs A, const float *s, int ns, float lo,
                                                          double invSize, int dim, int32_t *cell, const int32_t *c,
                                                          int nc, int d, int32_t *wrapped) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  const float x = i < ns ? s[i] : lo;
  const int cl = project_axis_inv(x, lo, invSize, dim);
  if (i < ns) cell[i] = cl;
  const int w = wrap_coord(i < nc ? c[i] : 0, d);
  if (i < nc) wrapped[i] = w;
}

// device copies of host arrays, freed together
struct Bufs {
  std::vector<void *> p;
  hipError_t e = hipSuccess;
  template <class T>
  T *up(const T *h, size_t n) {
    T *d = out<T>(n);
    if (d && n) note(hipMemcpy(d, h, n * sizeof(T), hipMemcpyHostToDevice));
    return d;
  }
  template <class T>
  T *out(size_t n) {
    void *d = nullptr;
    note(hipMalloc(&d, (n ? n : 1) * sizeof(T)));
    if (d) p.push_back(d);
    return (T *)d;
  }
  template <class T>
  void down(T *h, const T *d, size_t n) {
    if (e == hipSuccess && n) note(hipMemcpy(h, d, n * sizeof(T), hipMemcpyDeviceToHost));
  }
  void note(hipError_t x) {
    if (e == hipSuccess) e = x;
  }
  ~Bufs() {
    for (void *q : p) (void)hipFree(q);
  }
};

int finish(const Bufs &B, const char *what) {
  if (B.e != hipSuccess) {
    set_error("%s: %s", what, hipGetErrorString(B.e));
    return IRT_E_HIP;
  }
  return IRT_OK;
}

constexpr int kMaxValues = 1 << 18;  // per call

}  // namespace
}  // namespace irt

using namespace irt;

extern "C" int irt_debug_device_div(int device, const float *a, const float *b, int n, float *outUniform,
                                    float *outRecip) {
  const char *what = "irt_debug_device_div";
  if (n <= 0 || n > kMaxValues || !a || !b || !outUniform || !outRecip) {
    set_error("%s: bad argument (1 to 2^18 values)", what);
    return IRT_E_INVALID;
  }
  IRT_HIP(hipSetDevice(device));
  std::vector<double> inv((size_t)n);
  for (int i = 0; i < n; ++i) inv[i] = 1.0 / (double)b[i];  // as frame_args (irt_launch.hip) has it
  RenderArgs A;
  memset(&A, 0, sizeof(A));
  Bufs B;
  const float *da = B.up(a, n), *db = B.up(b, n);
  const double *di = B.up(inv.data(), n);
  float *du = B.out<float>(n), *dr = B.out<float>(n);
  if (B.e == hipSuccess) {
    hipLaunchKernelGGL(k_debug_div, dim3((n + 255) / 256), dim3(256), 0, 0, A, da, db, di, n, du, dr);
    B.note(hipGetLastError());
  }
  B.down(outUniform, du, n);
  B.down(outRecip, dr, n);
  return finish(B, what);
}

extern "C" int irt_debug_classify(irt_context *c, const float *v, int n, float *out4, float *alpha) {
  const char *what = "irt_debug_classify";
  if (!c || c->building || n <= 0 || n > kMaxValues || !v || !out4 || !alpha) {
    set_error("%s: bad argument (a built context, 1 to 2^18 values)", what);
    return IRT_E_INVALID;
  }
  if (c->updPending) return update_pending(what);
  if (!c->tfSet) {
    set_error("%s: no transfer function set (irt_set_transfunc)", what);
    return IRT_E_INVALID;
  }
  IRT_HIP(hipSetDevice(c->device));
  IRT_HIP(hipStreamSynchronize(c->stream));  // the transfer function's upload
  irt_launch_params lp;
  memset(&lp, 0, sizeof(lp));
  RenderArgs A;
  scene_args(c, IRT_MODE_USER_GEOM, A);
  frame_args(c, &lp, nullptr, nullptr, A);
  Bufs B;
  const float *dv = B.up(v, n);
  float4 *dout = B.out<float4>(n);
  float *dal = B.out<float>(n);
  if (B.e == hipSuccess) {
    hipLaunchKernelGGL(k_debug_classify, dim3((n + 255) / 256), dim3(256), 0, 0, A, dv, n, dout, dal);
    B.note(hipGetLastError());
  }
  B.down(reinterpret_cast<float4 *>(out4), dout, n);
  B.down(alpha, dal, n);
  return finish(B, what);
}

extern "C" int irt_debug_ray_tests(int device, const float *rays, const uint8_t *interior, int n, const float box6[6],
                                   float radiusA, float radiusB, int32_t *flags, float *out14) {
  const char *what = "irt_debug_ray_tests";
  if (n <= 0 || n > kMaxValues || !rays || !interior || !box6 || !flags || !out14) {
    set_error("%s: bad argument (1 to 2^18 rays)", what);
    return IRT_E_INVALID;
  }
  IRT_HIP(hipSetDevice(device));
  RenderArgs A;
  memset(&A, 0, sizeof(A));
  A.bmin = make_float3(box6[0], box6[1], box6[2]);
  A.bmax = make_float3(box6[3], box6[4], box6[5]);
  Bufs B;
  const float *dr = B.up(rays, 6 * (size_t)n);
  const uint8_t *di = B.up(interior, n);
  int32_t *df = B.out<int32_t>(n);
  float *dout = B.out<float>(14 * (size_t)n);
  if (B.e == hipSuccess) {
    hipLaunchKernelGGL(k_debug_ray_tests, dim3((n + 255) / 256), dim3(256), 0, 0, A, dr, di, n, radiusA, radiusB, df,
                       dout);
    B.note(hipGetLastError());
  }
  B.down(flags, df, n);
  B.down(out14, dout, 14 * (size_t)n);
  return finish(B, what);
}

extern "C" int irt_debug_gen_ray(int device, const irt_launch_params *lp, int width, int height, float *dir3,
                                 uint32_t *state) {
  const char *what = "irt_debug_gen_ray";
  if (!lp || width < 1 || height < 1 || (long long)width * height > kMaxValues || !dir3 || !state) {
    set_error("%s: bad argument (1 to 2^18 pixels)", what);
    return IRT_E_INVALID;
  }
  IRT_HIP(hipSetDevice(device));
  RenderArgs A;
  memset(&A, 0, sizeof(A));
  A.org = make_float3(lp->org.x, lp->org.y, lp->org.z);
  A.dir00 = make_float3(lp->dir_00.x, lp->dir_00.y, lp->dir_00.z);
  A.du = make_float3(lp->dir_du.x, lp->dir_du.y, lp->dir_du.z);
  A.dv = make_float3(lp->dir_dv.x, lp->dir_dv.y, lp->dir_dv.z);
  A.accumID = lp->accumID;
  A.W = width;
  A.H = height;
  const size_t n = (size_t)width * height;
  Bufs B;
  float *dd = B.out<float>(3 * n);
  uint32_t *ds = B.out<uint32_t>(n);
  if (B.e == hipSuccess) {
    hipLaunchKernelGGL(k_debug_gen_ray, dim3((width + 7) / 8, (height + 7) / 8), dim3(64), 0, 0, A, dd, ds);
    B.note(hipGetLastError());
  }
  B.down(dir3, dd, 3 * n);
  B.down(state, ds, n);
  return finish(B, what);
}

extern "C" int irt_debug_grid_coord(int device, const float *s, int ns, float lo, float hi, int dim, int32_t *cell,
                                    const int32_t *c, int nc, int d, int32_t *wrapped) {
  const char *what = "irt_debug_grid_coord";
  if (ns < 0 || nc < 0 || ns > kMaxValues || nc > kMaxValues || ns + nc == 0 || (ns && (!s || !cell)) ||
      (nc && (!c || !wrapped)) || dim < 1 || d < 1) {
    set_error("%s: bad argument (up to 2^18 values each, dim and d at least 1)", what);
    return IRT_E_INVALID;
  }
  IRT_HIP(hipSetDevice(device));
  const float size = hi - lo;  // float, as the reference subtracts
  const double invSize = 1.0 / (double)size;
  RenderArgs A;
  memset(&A, 0, sizeof(A));
  Bufs B;
  const float *ds = B.up(s, ns);
  const int32_t *dc = B.up(c, nc);
  int32_t *dcell = B.out<int32_t>(ns), *dw = B.out<int32_t>(nc);
  const int m = ns > nc ? ns : nc;
  if (B.e == hipSuccess) {
    hipLaunchKernelGGL(k_debug_grid_coord, dim3((m + 255) / 256), dim3(256), 0, 0, A, ds, ns, lo, invSize, dim,
                       dcell, dc, nc, d, dw);
    B.note(hipGetLastError());
  }
  B.down(cell, dcell, ns);
  B.down(wrapped, dw, nc);
  return finish(B, what);
}
