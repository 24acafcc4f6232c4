// irt_overlay.hip -- lines on the globe (include/icon_rt_hip.h, "overlay"; the definition is
// irt_overlay.h): the device object (irt_overlay_create / _destroy), the kernel that finds which
// segment covers each pixel's point on the sphere and composites the line layer with a frame's
// accum, and the context entry point irt_render_overlay.  The host side (the segments, the bin
// table, irt_overlay_cover) is host/irt_overlay.cpp.
//
// The kernel reads no scene array and runs no Tracer: per pixel the raygen's ray (irt_raygen.h
// gen_ray), its hit with the sphere (irt_device.h intersect_sphere), the bin of the hit's direction,
// the bin's list, and the pixel write of write_pixel (its lerp, srgb_byte, make_8bit).

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "irt_context.h"
#include "irt_overlay.h"
#include "irt_raygen.h"
#include "irt_sample_dev.h"

struct irt_overlay {
  irt_context *owner = nullptr;
  irt_overlay_segment *d_seg = nullptr;  // n records (hipMalloc: 256-byte aligned)
  irt::OverlayStyle *d_styles = nullptr; // IRT_OVERLAY_MAX_STYLES entries
  uint32_t *d_binStart = nullptr;        // 6 N^2 + 1
  uint32_t *d_binSeg = nullptr;          // the lists, each ascending
  uint32_t n = 0;
  int N = 1;
  size_t entries = 0;  // in d_binSeg
  size_t bytes = 0;
};

namespace irt {

// What the kernel needs beyond RenderArgs (of which it reads the camera, accumID and its lerp
// weight, W, H and the sRGB thresholds)
struct OverlayArgs {
  const irt_overlay_segment *seg;
  const OverlayStyle *styles;
  const uint32_t *binStart, *binSeg;
  uint32_t n;
  int N;
  uint32_t packetsX;    // 8 x 8 pixel packets per packet row ...
  uint32_t numPackets;  // ... and in the frame
  float surfaceRadius;
  int over;             // IRT_OVERLAY_OVER
  const float4 *accumIn;  // may be null
  float4 *cover;
  uint32_t *fb;
  int32_t *segment;     // may be null
};

namespace {

typedef const __attribute__((address_space(4))) float *ScalarFloats;

// One wave per workgroup, one 8 x 8 pixel packet per wave (lane = 8 dy + dx), the mapping of
// k_render_levels.  The 64 points of a packet fall into one to a few bins.
//
// !UNIFORM (the shipped form): each lane walks the list of its own bin with vector loads
// (overlay_find, as the host runs it); neighbouring lanes share a bin, so their loads share lines.
// UNIFORM: the wave takes the distinct bins of its live lanes one after the other -- the bin of the
// first lane still without an answer -- and reads that bin's list and each 64-B segment record
// through the scalar unit (the tables are written by the host before the launch: the constant address
// space); every lane of the bin tests the record from SGPRs, and a bin's walk ends when all its lanes
// have a hit (the lists ascend, so a lane's first hit is its lowest).  Measured at 1024^2 it is never
// faster and up to 3 times slower where lists are long: a wave waits out every record's load before
// it tests it, one record at a time and one bin after the other, while the lanes' vector loads of
// several bins are in flight together.  IRT_OVERLAY_UNIFORM=1 selects it, for
// profiles/overlay_rate.py only.
template <bool UNIFORM>
__global__ void __launch_bounds__(64) k_render_overlay(RenderArgs A, OverlayArgs S) {
  const uint32_t w = (uint32_t)workgroup_index();  // packets < 2^27
  if (w >= S.numPackets) return;                   // wave-uniform (the last grid row's tail)
  const uint32_t py = w / S.packetsX, px = w - py * S.packetsX;
  const int x = (int)(px * 8u + (threadIdx.x & 7u)), y = (int)(py * 8u + (threadIdx.x >> 3));
  const bool inFrame = x < A.W && y < A.H;
  uint32_t st = 0;
  float dx = 1.f, dy = 1.f, dz = 1.f;
  if (inFrame) gen_ray(A, A.accumID, x, y, st, dx, dy, dz);
  const Ray ray = {A.org.x, A.org.y, A.org.z, 0.f, dx, dy, dz, 1e10f};
  float tn = 0.f, tf = 0.f;
  const bool hit = inFrame && intersect_sphere(ray, S.surfaceRadius, tn, tf);
  const bool near = tn > 0.f;
  const bool live = hit && (near || tf > 0.f);
  const float t = near ? tn : tf;
  const float X = ray.ox + ray.dx * t, Y = ray.oy + ray.dy * t, Z = ray.oz + ray.dz * t;
  const float len = sqrtf((X * X + Y * Y) + Z * Z);
  const float u[3] = {X / len, Y / len, Z / len};

  int32_t s = -1;
  int style = 0;
  if (S.n != 0u) {  // wave-uniform
    if constexpr (UNIFORM) {
      const int bin = live ? overlay_bin(u, S.N) : -1;
      bool todo = live;
      unsigned long long m;
      while ((m = __ballot(todo)) != 0ull) {
        const int b = __builtin_amdgcn_readlane(bin, (int)__builtin_ctzll(m));  // in [0, 6 N^2)
        const bool mine = todo && bin == b;
        bool open = mine;
        const uint32_t k1 = scalar_word(S.binStart, (uint32_t)b + 1u);
#pragma nounroll
        for (uint32_t k = scalar_word(S.binStart, (uint32_t)b); k < k1 && __ballot(open) != 0ull; ++k) {
          const uint32_t i = scalar_word(S.binSeg, k);  // < n
          ScalarFloats r = (ScalarFloats)S.seg + 16u * (size_t)i;
          irt_overlay_segment g;
          for (int c = 0; c < 3; ++c) {
            g.a[c] = r[c];
            g.b[c] = r[3 + c];
            g.n[c] = r[6 + c];
            g.t[c] = r[9 + c];
          }
          g.sinHalf = r[12];
          const int gs = __builtin_bit_cast(int, r[13]);  // < IRT_OVERLAY_MAX_STYLES (checked at creation)
          ScalarFloats q = (ScalarFloats)S.styles + 8u * (uint32_t)gs;
          OverlayStyle os;
          os.sinW = q[4];
          os.chord2 = q[5];
          if (open && overlay_covers(g, os, u)) {
            s = (int32_t)i;
            style = gs;
            open = false;
          }
        }
        todo = todo && !mine;
      }
    } else {
      if (live) {
        s = overlay_find(S.seg, S.n, S.styles, S.binStart, S.binSeg, S.N, u);
        if (s >= 0) style = S.seg[s].style;
      }
    }
  }
  if (!inFrame) return;
  const size_t p = (size_t)x + (size_t)A.W * (size_t)y;
  float L[4] = {0.f, 0.f, 0.f, 0.f};
  if (s >= 0) {
    const float4 l = *reinterpret_cast<const float4 *>(S.styles[style].L);
    L[0] = l.x, L[1] = l.y, L[2] = l.z, L[3] = l.w;
  }
  const float4 oldK = S.cover[p];
  const float4 v4 = S.accumIn ? S.accumIn[p] : make_float4(0.f, 0.f, 0.f, 0.f);
  const float old[4] = {oldK.x, oldK.y, oldK.z, oldK.w}, V[4] = {v4.x, v4.y, v4.z, v4.w};
  float K[4], out[4];
  overlay_lerp(A.accumW, L, old, K);
  overlay_composite(S.over != 0, V, K, out);
  const uint32_t rgba = srgb_byte(A.srgbTh, out[0]) + (srgb_byte(A.srgbTh, out[1]) << 8) +
                        (srgb_byte(A.srgbTh, out[2]) << 16) + (make_8bit(out[3]) << 24);
  typedef float f4v __attribute__((ext_vector_type(4)));
  const f4v kv = {K[0], K[1], K[2], K[3]};
  __builtin_nontemporal_store(kv, reinterpret_cast<f4v *>(&S.cover[p]));
  __builtin_nontemporal_store(rgba, &S.fb[p]);
  if (S.segment) __builtin_nontemporal_store(s, &S.segment[p]);
}

int ov_alloc(irt_context *c, irt_overlay *ov, void **p, const void *src, size_t bytes) {
  *p = nullptr;
  const size_t size = std::max<size_t>(bytes, 256);
  IRT_HIP(hipMalloc(p, size));
  ov->bytes += size;
  if (bytes) IRT_HIP(hipMemcpy(*p, src, bytes, hipMemcpyHostToDevice));
  return IRT_OK;
}

void ov_free(irt_context *c, irt_overlay *ov) {
  void *ptrs[] = {ov->d_seg, ov->d_styles, ov->d_binStart, ov->d_binSeg};
  for (void *p : ptrs)
    if (p) (void)hipFree(p);
  c->bytes -= std::min(c->bytes, ov->bytes);
  c->info.deviceBytes = c->bytes;
  delete ov;
}

}  // namespace
}  // namespace irt

using namespace irt;

void free_overlays(irt_context *c) {
  for (irt_overlay *ov : c->overlays) ov_free(c, ov);
  c->overlays.clear();
}

extern "C" {

int irt_overlay_create(irt_context *c, const irt_overlay_segment *seg, size_t n, const irt_overlay_style *styles,
                       int numStyles, int binsPerEdge, irt_overlay **overlay) {
  const char *what = "irt_overlay_create";
  if (!c || c->building) {
    set_error("%s: null context, or a context still being created", what);
    return IRT_E_INVALID;
  }
  if (!overlay) {
    set_error("%s: null overlay", what);
    return IRT_E_INVALID;
  }
  OverlayStyle st[IRT_OVERLAY_MAX_STYLES];
  memset(st, 0, sizeof(st));
  int rc = overlay_styles(what, styles, numStyles, st);
  if (rc) return rc;
  if ((rc = overlay_segments_ok(what, seg, n, numStyles))) return rc;
  if (binsPerEdge < 0 || binsPerEdge > kOverlayMaxBins) {
    set_error("%s: binsPerEdge %d is outside [0, %d]", what, binsPerEdge, kOverlayMaxBins);
    return IRT_E_INVALID;
  }
  const float maxW = overlay_max_half_width(styles, numStyles);
  const int N = binsPerEdge ? binsPerEdge : overlay_auto_bins(seg, n, maxW);
  std::vector<uint32_t> binStart(6 * (size_t)N * N + 1, 0u), binSeg;
  size_t entries = 0;
  if (n) {
    if ((rc = irt_overlay_bins(seg, n, maxW, N, binStart.data(), nullptr, 0, &entries))) return rc;
    binSeg.resize(entries);
    if ((rc = irt_overlay_bins(seg, n, maxW, N, binStart.data(), binSeg.data(), entries, &entries))) return rc;
  }
  IRT_HIP(hipSetDevice(c->device));
  irt_overlay *ov = new irt_overlay;
  ov->owner = c;
  ov->n = (uint32_t)n;
  ov->N = N;
  ov->entries = entries;
  if ((rc = ov_alloc(c, ov, (void **)&ov->d_seg, seg, n * sizeof(irt_overlay_segment))) ||
      (rc = ov_alloc(c, ov, (void **)&ov->d_styles, st, sizeof(st))) ||
      (rc = ov_alloc(c, ov, (void **)&ov->d_binStart, binStart.data(), binStart.size() * sizeof(uint32_t))) ||
      (rc = ov_alloc(c, ov, (void **)&ov->d_binSeg, binSeg.data(), binSeg.size() * sizeof(uint32_t)))) {
    c->bytes += ov->bytes;  // (ov_free takes them off again)
    ov_free(c, ov);
    return rc;
  }
  c->bytes += ov->bytes;
  c->info.deviceBytes = c->bytes;
  c->overlays.push_back(ov);
  *overlay = ov;
  return IRT_OK;
}

int irt_overlay_destroy(irt_context *c, irt_overlay *overlay) {
  const char *what = "irt_overlay_destroy";
  if (!c || c->building) {
    set_error("%s: null context, or a context still being created", what);
    return IRT_E_INVALID;
  }
  auto it = std::find(c->overlays.begin(), c->overlays.end(), overlay);
  if (!overlay || it == c->overlays.end()) {
    set_error("%s: not an overlay of this context", what);
    return IRT_E_INVALID;
  }
  IRT_HIP(hipSetDevice(c->device));
  IRT_HIP(wait_samples(c));  // a render call in flight reads its arrays
  c->overlays.erase(it);
  ov_free(c, overlay);
  return IRT_OK;
}

int irt_overlay_get_bins(const irt_context *c, const irt_overlay *overlay, int *binsPerEdge, size_t *numEntries) {
  const char *what = "irt_overlay_get_bins";
  if (!c || c->building) {
    set_error("%s: null context, or a context still being created", what);
    return IRT_E_INVALID;
  }
  if (!overlay || std::find(c->overlays.begin(), c->overlays.end(), overlay) == c->overlays.end()) {
    set_error("%s: not an overlay of this context", what);
    return IRT_E_INVALID;
  }
  if (binsPerEdge) *binsPerEdge = overlay->N;
  if (numEntries) *numEntries = overlay->entries;
  return IRT_OK;
}

int irt_render_overlay(irt_context *c, const irt_overlay *overlay, const irt_launch_params *lp, int width, int height,
                       float surfaceRadius, int flags, const irt_vec4f *d_accum_in, irt_vec4f *d_cover,
                       uint32_t *d_fb, int32_t *d_segment, void *stream) {
  const char *what = "irt_render_overlay";
  if (c && !c->building && !lp) {
    set_error("%s: null lp", what);
    return IRT_E_INVALID;
  }
  int rc = sample_check(c, IRT_MODE_USER_GEOM, what);  // (no sampler is used: the cell mode asks for nothing)
  if (rc) return rc;
  if (!overlay) {
    set_error("%s: null overlay", what);
    return IRT_E_INVALID;
  }
  // (looked up, not dereferenced: a foreign pointer may be anything)
  if (std::find(c->overlays.begin(), c->overlays.end(), overlay) == c->overlays.end()) {
    set_error("%s: not an overlay of this context", what);
    return IRT_E_INVALID;
  }
  if (!(isfinite(surfaceRadius) && surfaceRadius > 0.f)) {
    set_error("%s: surfaceRadius = %g is not finite and positive", what, (double)surfaceRadius);
    return IRT_E_INVALID;
  }
  if (flags & ~IRT_OVERLAY_OVER) {
    set_error("%s: unknown flag bits 0x%x", what, (unsigned)(flags & ~IRT_OVERLAY_OVER));
    return IRT_E_INVALID;
  }
  // (irt_render_levels' limits)
  if (width < 1 || height < 1 || (uint64_t)width * (uint64_t)height >= (uint64_t(1) << 27)) {
    set_error("%s: a frame of %d x %d pixels (at least 1 x 1, fewer than 2^27 pixels)", what, width, height);
    return IRT_E_INVALID;
  }
  if (!d_cover || !d_fb) {
    set_error("%s: null d_cover or d_fb", what);
    return IRT_E_INVALID;
  }
  hipStream_t s = (hipStream_t)stream;
  if ((rc = sample_begin(c, s))) return rc;
  RenderArgs A;
  memset(&A, 0, sizeof(A));
  frame_args(c, lp, d_fb, nullptr, A);
  A.W = width;
  A.H = height;
  OverlayArgs S;
  memset(&S, 0, sizeof(S));
  S.seg = overlay->d_seg;
  S.styles = overlay->d_styles;
  S.binStart = overlay->d_binStart;
  S.binSeg = overlay->d_binSeg;
  S.n = overlay->n;
  S.N = overlay->N;
  S.packetsX = ((uint32_t)width + 7u) / 8u;
  S.numPackets = S.packetsX * (((uint32_t)height + 7u) / 8u);  // <= width * height < 2^27
  S.surfaceRadius = surfaceRadius;
  S.over = flags & IRT_OVERLAY_OVER;
  S.accumIn = (const float4 *)d_accum_in;
  S.cover = (float4 *)d_cover;
  S.fb = d_fb;
  S.segment = d_segment;
  // IRT_OVERLAY_UNIFORM=1: the wave-uniform form (measurement only, profiles/overlay_rate.py)
  const char *e = getenv("IRT_OVERLAY_UNIFORM");
  auto kernel = e && atoi(e) == 1 ? k_render_overlay<true> : k_render_overlay<false>;
  hipLaunchKernelGGL(kernel, sample_grid(S.numPackets), dim3(64), 0, s, A, S);
  return sample_end(c, s);
}

}  // extern "C"
