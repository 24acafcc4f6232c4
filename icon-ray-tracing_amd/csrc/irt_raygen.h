// irt_raygen.h -- the raygen's per-ray half, included by irt_render.hip (one translation unit):
// the per-pixel pieces (the frame grid's Pixel, gen_ray, the pixel writes, the chained-frame
// hand-off and replay, the counters' flush, the grid walk render_grid) and the full raygen of one
// pixel, one lane per ray (render_pixel) or as the per-lane state machine around the wave's one
// Woodcock call site (render_pixel_coop).
#pragma once

#include "irt_tracer.h"

namespace irt {

// ------------------------------------------------------------------ per-pixel pieces
// The frame grid: 256-thread workgroup b, thread t -> gid = 256 b + t.  Workgroup b covers
// 16x16 pixels of tile k = b / 16 of this launch (frame tile tileBegin + k*tileStride, or
// tileList[k]),
// wave w an 8x8 packet, lane l one pixel.  The block index is passed on its own so that the
// tile arithmetic (an integer division by tilesX) stays scalar: it is uniform per workgroup.
struct Pixel {
  int x, y;
  size_t outIdx;
  bool active;
};
__device__ __forceinline__ Pixel pixel_of(const RenderArgs &A, uint32_t blkU, int tid) {
  const int blk = (int)__builtin_amdgcn_readfirstlane(blkU);
  const int k = blk >> 4, sub = blk & 15;
  const int wave = tid >> 6, lane = tid & 63;
  const int lx = ((sub & 3) << 4) | ((wave & 1) << 3) | (lane & 7);
  const int ly = ((sub >> 2) << 4) | ((wave >> 1) << 3) | (lane >> 3);
  const int tileId = !A.tileList ? A.tileBegin + k * A.tileStride : (k < A.numTiles ? (int)scalar_word(A.tileList, (uint32_t)k) : 0);
  const int tx = tileId % A.tilesX, ty = tileId / A.tilesX;
  Pixel p;
  p.x = tx * 64 + lx;
  p.y = ty * 64 + ly;
  p.active = k < A.numTiles && p.x < A.W && p.y < A.H;
  p.outIdx = A.packed ? (size_t)k * 4096 + ly * 64 + lx : (size_t)p.x + (size_t)A.W * p.y;
  return p;
}

// Random rnd(accumID*W*H + x, y) (deviceCode.cu:288-289) and generateRay (36-49); g++
// draws the dir_dv jitter first.
__device__ __forceinline__ void gen_ray(const RenderArgs &A, int accumID, int x, int y, uint32_t &st,
                                        float &dx, float &dy, float &dz, int frame = 0) {
  st = lcg_seed((uint32_t)accumID * (uint32_t)A.W * (uint32_t)A.H + (uint32_t)x, (uint32_t)y);
  st = lcg_next(st);
  const float jv = lcg_float(st);
  st = lcg_next(st);
  const float ju = lcg_float(st);
  const float su = (float)x + .5f, sv = (float)y + .5f;
  const float a = su + ju, b = sv + jv;
  float3 d00 = A.dir00, du = A.du, dv = A.dv;
  if (A.frameCams) {  // a sequence of views: this frame's camera
    const float4 w1 = cam_word(A, frame, 1), w2 = cam_word(A, frame, 2), w3 = cam_word(A, frame, 3);
    d00 = make_float3(w1.x, w1.y, w1.z);
    du = make_float3(w2.x, w2.y, w2.z);
    dv = make_float3(w3.x, w3.y, w3.z);
  }
  dx = (d00.x + a * du.x) + b * dv.x;
  dy = (d00.y + a * du.y) + b * dv.y;
  dz = (d00.z + a * du.z) + b * dv.z;
  const float len = sqrtf(dot3(dx, dy, dz, dx, dy, dz));
  if (recip_ok(len)) {  // normalize's three quotients through one reciprocal (irt_device.h)
    const double r = recip_d(len);
    // (the bare products: one that comes out subnormal, where alone the division may round
    // otherwise, is below 1e-5 whichever neighbour it is, and the clamp below overwrites it:
    // tests/raymath_cases.py gen_ray_tie_cases)
    dx = div_product(dx, r);
    dy = div_product(dy, r);
    dz = div_product(dz, r);
  } else {
    dx = dx / len;
    dy = dy / len;
    dz = dz / len;
  }
  if (fabsf(dx) < 1e-5f) dx = 1e-5f;
  if (fabsf(dy) < 1e-5f) dy = 1e-5f;
  if (fabsf(dz) < 1e-5f) dz = 1e-5f;
}

// accumulate lerp(vec4f(color,alpha), old, 1/(accumID+1)) and write linear_to_srgb +
// make_rgba (deviceCode.cu:333-340).  Stream (nt = true): the pixel's lines are stored with
// the streaming hint -- nothing in the launch reads them again, so they should not displace
// locator lines in L2 (5-wave builds, the default: C3 -1.6 %, C4 -4.4 % with the accum
// prefetch also nt; the 4-wave A/B build keeps plain stores; profiles/r03za_nt/,
// profiles/r03zb_*).
template <bool nt = false>
__device__ __forceinline__ void write_pixel(const RenderArgs &A, size_t outIdx, float cr, float cg,
                                            float cb, float alpha, const float *s_th, float4 old) {
  const float w = A.accumW;  // 1.f / (float)(accumID + 1), on the host (the same division)
  float4 nv;
  nv.x = w * cr + (1.f - w) * old.x;
  nv.y = w * cg + (1.f - w) * old.y;
  nv.z = w * cb + (1.f - w) * old.z;
  nv.w = w * alpha + (1.f - w) * old.w;
  const uint32_t rgba = srgb_byte(s_th, nv.x) + (srgb_byte(s_th, nv.y) << 8) +
                        (srgb_byte(s_th, nv.z) << 16) + (make_8bit(nv.w) << 24);
  if constexpr (nt) {
    typedef float f4v __attribute__((ext_vector_type(4)));
    const f4v t = {nv.x, nv.y, nv.z, nv.w};
    __builtin_nontemporal_store(t, reinterpret_cast<f4v *>(&A.accum[outIdx]));
    __builtin_nontemporal_store(rgba, &A.fb[outIdx]);
  } else {
    A.accum[outIdx] = nv;
    A.fb[outIdx] = rgba;
  }
}
__device__ __forceinline__ void write_pixel(const RenderArgs &A, size_t outIdx, float cr, float cg,
                                            float cb, float alpha, const float *s_th) {
  write_pixel(A, outIdx, cr, cg, cb, alpha, s_th, A.accum[outIdx]);
}

// Chained progressive frames (RenderArgs::chain).  Workgroup (b, f) of a launch renders block
// b of frame accumID + f and lerps into accum/fb directly; the previous frame's colour of the
// same pixel must be in accum first.  The hand-off (cdna_hip_programming.md Guideline 16, R1):
// frame f - 1's wave stores its pixels write-through (sc1), drains them (vmcnt 0) and stores
// chainEpoch + f to its (block, wave) word (an sc1 store); frame f's wave polls that word
// (relaxed, agent scope: sc1 loads), then reads accum with sc1 loads (past this CU's L1).
// Every handed-off byte is stored and loaded sc1, so the hand-off does not depend on the two
// workgroups sharing an XCD (MI355X_MICROARCH.md, inter-workgroup visibility, first row of the
// sc1 table).  Frame f's wave gets there at the end of its rays, tens of microseconds after
// frame f - 1's workgroup -- dispatched numBlocks workgroups earlier -- finished, so the first
// poll normally hits.  A wait gives up after A.chainSpins polls and flags the launch
// (*A.chainFail, pinned host memory; the host returns IRT_E_CHAIN).
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ uint32_t out_pixels(const RenderArgs &A) {
  return A.packed ? (uint32_t)A.numTiles * 4096u : (uint32_t)A.W * (uint32_t)A.H;
}
__device__ __forceinline__ void chain_wait(const RenderArgs &A, uint32_t blk, int pwave, int frame) {
  uint32_t *f = A.chainFlag + (size_t)blk * 4u + (uint32_t)pwave;
  const uint32_t want = A.chainEpoch + (uint32_t)frame;  // frame - 1's publish
  for (uint32_t spins = 0;; ++spins) {
    const uint32_t v = __builtin_amdgcn_readfirstlane(__hip_atomic_load(f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    if (v == want) break;
    if (spins >= A.chainSpins) {
      if (__lane_id() == (unsigned)(__ffsll((long long)__ballot(1)) - 1))
        __hip_atomic_store(A.chainFail, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      break;
    }
    __builtin_amdgcn_s_sleep(2);
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");  // no instruction: the loads stay below
}
// the previous frame's accum pixel, past this CU's L1
__device__ __forceinline__ float4 chain_load_accum(const RenderArgs &A, size_t outIdx) {
  const __amdgpu_buffer_rsrc_t r = __builtin_amdgcn_make_buffer_rsrc((void *)A.accum, 0, (int)(out_pixels(A) * 16u), 0x00020000);
  return __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(r, (int)(outIdx * 16u), 0, 16));
}
// Which frames of a chained launch leave fb alone.  In a launch of consecutive progressive frames
// of one camera (irt_render_accumulate and its tile and tile-list forms: A.chain without
// A.frameCams) a pixel's RGBA8 is make_rgba(linear_to_srgb(accum)) of the accum its frame just
// stored, and every later frame of the launch whose ray hits the box overwrites it before anything
// reads it: only the launch's last frame converts and stores it (every frame stores accum, the
// hand-off, as before).  Everything else keeps the pixel write it had: a sequence of views
// (A.frameCams: each view is an image of its own), single-frame launches and the unchained
// sample-buffer batch (no A.chain; k_accumulate), and the split-packet and slot-table kernels
// (OPT_SPLIT, single frames only; OPT_SLOT: render_pixel_coop leaves both out at compile time).
__device__ __forceinline__ bool chain_skips_fb(const RenderArgs &A, int frame) {
  return A.chain && !A.frameCams && frame < A.numSamples - 1;
}
// ... and the frame of such a launch that writes fb for all of them: its last
__device__ __forceinline__ bool chain_last_fb(const RenderArgs &A, int frame) {
  return A.chain && !A.frameCams && frame == A.numSamples - 1;
}
// The other half of that rule, for a pixel whose ray misses the box in the launch's last frame
// (deviceCode.cu:294-295: that frame writes nothing).  When every frame wrote fb, the pixel then
// held the bytes of the latest earlier frame of the launch whose ray hit -- the conversion of the
// accum that frame stored, which no frame has touched since, so of accum as it is now.  The lane
// replays gen_ray + box_test for frames frame - 1 .. 0 of the launch (the same code on the same
// inputs as those frames' own waves: the same hit or miss), stops at the first hit and then writes
// the conversion of accum[pixel], read past L1 after the wave's chain wait (frame - 1's publish word
// covers every earlier frame's stores).  No frame of the launch hit: fb stays untouched.  Cold: a
// camera with every ray in the box never gets here.
__device__ __forceinline__ void chain_replay_fb(const RenderArgs &KA, uint32_t blk, int ptid, int frame,
                                                const float *s_th) {
  // The launch's arguments through a per-lane pointer, and the frame counter per lane: vector
  // loads and VGPRs, free at the ray's end, where the kernel has no SGPRs to spare (the accum
  // pixel by agent-scope loads, sc1 as chain_load_accum's, for the same reason: no resource words).
  const RenderArgs *vp = &KA;
  asm volatile("" : "+v"(vp));
  const RenderArgs &A = *vp;
  const Pixel p = pixel_of(A, blk, ptid);
  if (!p.active) return;
  int g = frame;
  asm volatile("" : "+v"(g));
  bool seen = false;
#pragma nounroll
  while (--g >= 0 && !seen) {
    uint32_t st;
    float dx, dy, dz, t0, t1;
    gen_ray(A, A.accumID + g, p.x, p.y, st, dx, dy, dz);
    const Ray ray = {A.org.x, A.org.y, A.org.z, 0.f, dx, dy, dz, 1e10f};
    seen = box_test(ray, A, t0, t1);
  }
  if (!seen) return;
  const float *ap = reinterpret_cast<const float *>(A.accum + p.outIdx);
  float a[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) a[k] = __hip_atomic_load(ap + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const uint32_t rgba = srgb_byte(s_th, a[0]) + (srgb_byte(s_th, a[1]) << 8) + (srgb_byte(s_th, a[2]) << 16) +
                        (make_8bit(a[3]) << 24);
  __builtin_nontemporal_store(rgba, &A.fb[p.outIdx]);
}
// write_pixel's lerp and RGBA8 with the weight of this frame; publish: write-through (sc1)
// stores that the next frame's wave reads, else streaming stores as write_pixel<true>.
// toFb (wave-uniform: a scalar branch) is false for a frame whose RGBA8 a later frame of the same
// launch overwrites before anything reads it (chain_skips_fb): accum alone is stored, no
// conversion runs.
__device__ __forceinline__ void write_pixel_chain(const RenderArgs &A, size_t outIdx, float cr, float cg, float cb,
                                                  float alpha, float w, const float *s_th, float4 old, bool publish,
                                                  bool toFb) {
  float4 nv;
  nv.x = w * cr + (1.f - w) * old.x;
  nv.y = w * cg + (1.f - w) * old.y;
  nv.z = w * cb + (1.f - w) * old.z;
  nv.w = w * alpha + (1.f - w) * old.w;
  if (!toFb) {
    if (publish) {
      const __amdgpu_buffer_rsrc_t ra =
          __builtin_amdgcn_make_buffer_rsrc((void *)A.accum, 0, (int)(out_pixels(A) * 16u), 0x00020000);
      __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, nv), ra, (int)(outIdx * 16u), 0, 16);
    } else {
      typedef float f4v __attribute__((ext_vector_type(4)));
      const f4v t = {nv.x, nv.y, nv.z, nv.w};
      __builtin_nontemporal_store(t, reinterpret_cast<f4v *>(&A.accum[outIdx]));
    }
    return;
  }
  const uint32_t rgba = srgb_byte(s_th, nv.x) + (srgb_byte(s_th, nv.y) << 8) +
                        (srgb_byte(s_th, nv.z) << 16) + (make_8bit(nv.w) << 24);
#ifdef IRT_PROBE_BUILD
  if (publish && A.probeExit == 17) {  // measurement only (17, probe build): plain stores to publish
    A.accum[outIdx] = nv;
    A.fb[outIdx] = rgba;
    return;
  }
#endif
  if (publish) {
    const uint32_t n = out_pixels(A);
    const __amdgpu_buffer_rsrc_t ra = __builtin_amdgcn_make_buffer_rsrc((void *)A.accum, 0, (int)(n * 16u), 0x00020000);
    const __amdgpu_buffer_rsrc_t rf = __builtin_amdgcn_make_buffer_rsrc((void *)A.fb, 0, (int)(n * 4u), 0x00020000);
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, nv), ra, (int)(outIdx * 16u), 0, 16);
    __builtin_amdgcn_raw_buffer_store_b32(rgba, rf, (int)(outIdx * 4u), 0, 16);
  } else {
    typedef float f4v __attribute__((ext_vector_type(4)));
    const f4v t = {nv.x, nv.y, nv.z, nv.w};
    __builtin_nontemporal_store(t, reinterpret_cast<f4v *>(&A.accum[outIdx]));
    __builtin_nontemporal_store(rgba, &A.fb[outIdx]);
  }
}

// The workgroup's event counts (LDS) out to the launch's statistics, by the workgroup's
// last wave to finish (k_render).  Default: one store of the kCnt counts per workgroup into
// wgCounts, pinned host memory the host sums when asked (irt_context.hip finish_slot): no
// statistics kernel, and no two workgroups touch the same line.  Without wgCounts:
// device-scope atomics into the counter block -- 4 096 workgroups x 5 same-line atomics per
// 1024^2 frame, ~35 us of serialised atomics.
__device__ __forceinline__ void flush_counters(const RenderArgs &A, const uint32_t *s_cnt, int lane) {
  if (A.wgCounts) {
    const size_t wg = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
    if (lane < kCnt) A.wgCounts[wg * kCnt + lane] = s_cnt[lane];
  } else if (lane < 5 && s_cnt[lane]) {
    const size_t wg = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
    unsigned long long *dst = A.counterBuckets ? A.counterBuckets + (wg % kCounterBuckets) * 8 : A.counters;
    atomicAdd(&dst[lane], (unsigned long long)s_cnt[lane]);
  }
}

// A void packet of a chained launch (RenderArgs::voidList): in every frame each of its rays passes
// boxTest and misses both spheres -- numRanges == 0, colour (0, 0, 0, 0) -- so frame g only lerps
// the zero colour into the pixel.  The packet's one wave of the launch -- in whichever grid row its
// item sits: the packet depends on nothing inside the launch, and nothing in it on the packet --
// does that for every frame, in frame order and with write_pixel_chain's expressions (the products
// and sums stay: w * 0 + -0 is +0, and NaN or inf in accum go through as they would), then stores
// accum and the RGBA8 of the final value once, with the streaming stores the launch's last frame uses.
// The wave's counts are those of the numSamples waves the plain grid runs for the packet (rays
// launched = rays in the box = active pixels, once per frame: at most 64 x 65,535 rows, within the
// per-workgroup 32-bit word), stored or added as flush_counters does; no LDS, no wait, no publish.
// An empty item (~0u, the lists' padding) stores its zero counts and returns.  The bitmap form on the
// plain grid (RenderArgs::voidBits): frame 0's wave renders, every frame's wave reports its own counts.
// lerp: this wave renders the packet (the bitmap form: frame 0's wave; a list item: unless empty);
// frames: the frames whose counts the wave reports (the bitmap form: its own, 1; a list item: all).
__device__ __forceinline__ void void_packet(const RenderArgs &KA, uint32_t blk, int pwave, bool lerp, uint32_t frames) {
  // the launch's arguments through a per-lane pointer, as chain_replay_fb reads them: vector loads
  // into VGPRs, all free here, and none of the raygen's scarce SGPRs
  const RenderArgs *vp = &KA;
  asm volatile("" : "+v"(vp));
  const RenderArgs &A = *vp;
  const int lane = (int)__lane_id();
  const Pixel px = pixel_of(A, blk, pwave * 64 + lane);
  if (lerp && px.active) {
    float4 nv = A.accum[px.outIdx];
    const float c = 0.f;
#pragma nounroll
    for (int g = 0; g < A.numSamples; ++g) {
      const float w = 1.f / (float)(A.accumID + g + 1);
      nv.x = w * c + (1.f - w) * nv.x;
      nv.y = w * c + (1.f - w) * nv.y;
      nv.z = w * c + (1.f - w) * nv.z;
      nv.w = w * c + (1.f - w) * nv.w;
    }
    const float *th = A.srgbTh;
    const uint32_t rgba = srgb_byte(th, nv.x) + (srgb_byte(th, nv.y) << 8) + (srgb_byte(th, nv.z) << 16) +
                          (make_8bit(nv.w) << 24);
    typedef float f4v __attribute__((ext_vector_type(4)));
    const f4v t = {nv.x, nv.y, nv.z, nv.w};
    __builtin_nontemporal_store(t, reinterpret_cast<f4v *>(&A.accum[px.outIdx]));
    __builtin_nontemporal_store(rgba, &A.fb[px.outIdx]);
  }
  if (A.counters) {
    const uint32_t n = (uint32_t)__popcll(__ballot(px.active)) * frames;
    const size_t wg = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
    if (A.wgCounts) {
      if (lane < kCnt) A.wgCounts[wg * kCnt + lane] = lane < 2 ? n : 0u;
    } else if (lane < 2 && n) {
      unsigned long long *dst = A.counterBuckets ? A.counterBuckets + (wg % kCounterBuckets) * 8 : A.counters;
      atomicAdd(&dst[lane], (unsigned long long)n);
    }
  }
  if (A.wgTrace && lane == 0)  // measurement only
    A.wgTrace[4 * (blockIdx.y * gridDim.x + blockIdx.x) + 1] = (uint32_t)__builtin_amdgcn_s_memrealtime();
}

// sample-buffer marker of a frame whose ray missed the box (alpha is 0 or 1 otherwise)
constexpr float kNoSample = -1.f;

// The woodcockTrackingWithAccel raygen in GRID_ACCEL_MODE (deviceCode.cu:326-328): dda3
// (DDA.h:35-136) over the 256^3 Cartesian grid, each cell handed to the woodcockFunc
// lambda (304-323) with the grid's majorant.  Written exactly as the reference's g++ CPU
// build evaluates it, including `min(reduce_min(tnext), ray.tmax)` going through
// `int min(int, int)` (dda3_min_quirk, irt_common.h).
template <int OPT>
__device__ __forceinline__ void render_grid(const RenderArgs &A, Tracer<OPT> &T, const Ray &ray,
                                            float rtmin, float rtmax, uint32_t &st, float &cr,
                                            float &cg, float &cb, float &alpha) {
  const int D = kGridDim;
  // move ray so tmin becomes 0 (DDA.h:42-46)
  const float ox = ray.ox + rtmin * ray.dx, oy = ray.oy + rtmin * ray.dy, oz = ray.oz + rtmin * ray.dz;
  const float tmax = rtmax - rtmin;
  const float rx = 1.f / ray.dx, ry = 1.f / ray.dy, rz = 1.f / ray.dz;
  const float lx = (A.bmin.x - ox) * rx, ly = (A.bmin.y - oy) * ry, lz = (A.bmin.z - oz) * rz;
  const float hx = (A.bmax.x - ox) * rx, hy = (A.bmax.y - oy) * ry, hz = (A.bmax.z - oz) * rz;
  float nx = fminf(lx, hx), ny = fminf(ly, hy), nz = fminf(lz, hz);
  const float fx = fmaxf(lx, hx), fy = fmaxf(ly, hy), fz = fmaxf(lz, hz);
  if (ray.dx == 0.f) nx = IRT_FLT_MAX;
  if (ray.dy == 0.f) ny = IRT_FLT_MAX;
  if (ray.dz == 0.f) nz = IRT_FLT_MAX;
  int cx = project_on_grid(ox, A.bmin.x, A.bmax.x, D);
  int cy = project_on_grid(oy, A.bmin.y, A.bmax.y, D);
  int cz = project_on_grid(oz, A.bmin.z, A.bmax.z, D);
  const float dx = fmaxf(0.f, (fx - nx) / (float)D), dy = fmaxf(0.f, (fy - ny) / (float)D),
              dz = fmaxf(0.f, (fz - nz) / (float)D);
  const int sx = ray.dx > 0.f ? 1 : -1, sy = ray.dy > 0.f ? 1 : -1, sz = ray.dz > 0.f ? 1 : -1;
  const int ex = ray.dx > 0.f ? D : -1, ey = ray.dy > 0.f ? D : -1, ez = ray.dz > 0.f ? D : -1;
  float tnx = ray.dx > 0.f ? nx + (float)(cx + 1) * dx : nx + (float)(D - cx) * dx;
  float tny = ray.dy > 0.f ? ny + (float)(cy + 1) * dy : ny + (float)(D - cy) * dy;
  float tnz = ray.dz > 0.f ? nz + (float)(cz + 1) * dz : nz + (float)(D - cz) * dz;
  float tc0 = 0.f;
  for (int iter = 0; iter < 4 * D + 16; ++iter) {  // a cell per step, <= 3*D steps
    const float tmn = fminf(fminf(tnx, tny), tnz);  // reduce_min (vecmath.h:512-514)
    const float tc1 = dda3_min_quirk(tmn, tmax);
    const float w0 = rtmin + tc0, w1 = rtmin + tc1;  // func(leaf, ray_tmin+t0, ray_tmin+t1)
    // every majorant of this cell's block <= 0 (k_grid_bits): woodcockTracking would return
    // at once (deviceCode.cu:161-162) -- no draw, no sample, no hit -- so only the walk goes on
    constexpr int NB = kGridDim / kGridBlock;
    const bool inGrid = (unsigned)cx < (unsigned)D && (unsigned)cy < (unsigned)D && (unsigned)cz < (unsigned)D;
    const uint32_t gb = inGrid ? ((uint32_t)(cz / kGridBlock) * NB + (uint32_t)(cy / kGridBlock)) * NB +
                                     (uint32_t)(cx / kGridBlock)
                               : 0u;
    if (!inGrid || ((T.s_gbits[gb >> 5] >> (gb & 31)) & 1u)) {
      const float maj = A.gridMaxOp[(size_t)cz * D * D + (size_t)cy * D + cx];
      float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
      const float tw = T.woodcock(ray.dx, ray.dy, ray.dz, w0, w1, st, maj, s, !(w0 == w1));
      if (tw > w0 && tw < w1) {
        cr = s.x * A.amb.x * A.ambRad;
        cg = s.y * A.amb.y * A.ambRad;
        cb = s.z * A.amb.z * A.ambRad;
        alpha = s.w > 0.f ? 1.f : 0.f;
        return;
      }
    }
    if (tnx == tmn) {
      tnx += dx;
      cx += sx;
      if (cx == ex) return;
    }
    if (tny == tmn) {
      tny += dy;
      cy += sy;
      if (cy == ey) return;
    }
    if (tnz == tmn) {
      tnz += dz;
      cz += sz;
      if (cz == ez) return;
    }
    tc0 = tc1;
  }
}

// ------------------------------------------------------------------ the full raygen
// One pixel of woodcockTrackingWithAccel / woodcockTrackingAE, every range and leaf.
template <int OPT>
__device__ __forceinline__ void render_pixel(const RenderArgs &A, Tracer<OPT> &T, const Pixel &px,
                                             const float *s_th, int4 *s_dda, float4 *s_entry,
                                             int tid, int accumID, float4 *sampleOut) {
  uint32_t st;
  float dx, dy, dz;
  gen_ray(A, accumID, px.x, px.y, st, dx, dy, dz);
  const Ray ray = {A.org.x, A.org.y, A.org.z, 0.f, dx, dy, dz, 1e10f};
  float t0, t1;
  if (!box_test(ray, A, t0, t1)) {  // deviceCode.cu:294-295: pixel untouched
    if (sampleOut) *sampleOut = make_float4(0.f, 0.f, 0.f, kNoSample);
    return;
  }
  T.count(1);
  float cr = 0.f, cg = 0.f, cb = 0.f, alpha = 0.f;
  const bool ae = A.raygen == 1;
  // The ranges the raygen tracks.  woodcockTrackingAE (deviceCode.cu:239-275): the box
  // interval, majorant 1, one leaf.  woodcockTrackingWithAccel: sdda (ShellAccel.h:82-229)
  // over the shell's (at most two) sphere ranges (94-111), each a sequence of macrocell
  // leaves handed to the woodcockFunc lambda (deviceCode.cu:304-323).
  float rlo0 = t0, rhi0 = t1, rlo1 = __builtin_inff(), rhi1 = -__builtin_inff();
  int numRanges = 1;
  if (!ae) {
    float st1 = 0.f, st2 = 0.f, st3 = 0.f, st4 = 0.f;
    const bool s1 = intersect_sphere(ray, A.sbHi.x, st1, st4);
    const bool s2 = intersect_sphere(ray, A.sbLo.x, st2, st3);
    numRanges = 0;
    if ((s1 || s2) && !(st4 < t0)) {  // ray.tmin == t0 here
      numRanges = 2;
      if (s1 && !s2) {
        rlo0 = st1; rhi0 = st4;
      } else if (t0 < st2) {
        rlo0 = st1; rhi0 = st2;
        rlo1 = st3; rhi1 = st4;
      } else {
        rlo0 = st3; rhi0 = st4;
      }
    }
  }
  if constexpr ((OPT & OPT_GRID) != 0) {
    if (!ae) {
      render_grid(A, T, ray, t0, t1, st, cr, cg, cb, alpha);
      numRanges = 0;
    }
  }
  const float sceneEPS = A.sbLo.x * 1e-6f;
  for (int i = 0; i < numRanges; ++i) {
    const float lower = i ? rlo1 : rlo0, upper = i ? rhi1 : rhi0;
    if (upper <= lower) break;  // box1f::empty (vecmath.h:981)
    const bool lastRange = ae || i == 1 || rhi1 <= rlo1;
    // cellID of the entry point (ShellAccel.h:121-124)
    int cx = 0, cy = 0, cz = 0;
    if (!ae) {
      const float e1 = lower + sceneEPS;
      float r1, la1, lo1;
      to_spherical(ray.ox + ray.dx * e1, ray.oy + ray.dy * e1, ray.oz + ray.dz * e1, r1, la1, lo1);
      cx = project_axis(r1, A.sbLo.x, A.sbHi.x, A.dims.x);
      cy = project_axis(la1, A.sbLo.y, A.sbHi.y, A.dims.y);
      cz = project_axis(lo1, A.sbLo.z, A.sbHi.z, A.dims.z);
      if (!lastRange) lds_st16(&s_entry[tid], make_float4(r1, la1, lo1, 0.f));  // for step (125-127)
    }
    // The lat/lon "planes" (ShellAccel.h:147-160, 183-200) are built from
    // toCartesian(vec3f(0.f, ...)) -- radius 0 -- so N = 0, w = 0 and every evalPlane(...)
    // is exactly +-0: tnext = {upper, 0, 0} throughout, and the sign of those zeros never
    // changes a comparison.  (radius/sphereT1, 136-146, is dead.)  So only a range's FIRST
    // leaf can have positive length: every later one is [t_c, t_c] with t_c = min(upper, 0),
    // where woodcockTracking can only consume draws (its tw <= tmax == tmin never passes
    // deviceCode.cu:316).  Those leaves matter only through the RNG state, i.e. only when
    // another range follows -- and only then are the exit point, step and stop needed.
    const float tnx = upper, tny = 0.f, tnz = 0.f;
    float t = lower;
    for (int iter = 0; iter < (1 << 22); ++iter) {
      float tt1 = IRT_FLT_MAX;
      if (ae) {
        tt1 = upper;
      } else {
        if (tnx < tt1 && tnx >= t) tt1 = tnx;
        if (tny < tt1 && tny >= t) tt1 = tny;
        if (tnz < tt1 && tnz >= t) tt1 = tnz;
      }
      const bool zeroLen = tt1 == t;
      if (zeroLen && lastRange) break;
      if constexpr ((OPT & OPT_STATS) != 0) T.cnt.deg += zeroLen ? 1u : 0u;
      float maj = 1.f;
      if (!ae) {
        const uint32_t leaf = (uint32_t)wrap_coord(cz, A.dims.z) * (uint32_t)A.dims.x * (uint32_t)A.dims.y +
                              (uint32_t)wrap_coord(cy, A.dims.y) * (uint32_t)A.dims.x +
                              (uint32_t)wrap_coord(cx, A.dims.x);
        maj = A.maxOp[leaf];
      }
      bool fast = false;
      if (zeroLen) {
        const float q = maj / A.unitDistance;
        const uint32_t nx = lcg_next(st);
        if (!(maj > 0.f)) {
          fast = true;  // woodcockTracking returns at once (deviceCode.cu:161-162)
        } else if (q > 0.f && q <= 1e30f && (nx & 0x00FFFFFFu) != 0u) {
          st = nx;  // one draw: logf(1-xi) < 0 puts t past tmax (165-166)
          fast = true;
        }
      }
      if (!fast) {  // woodcockFunc(leafID, t, tt1)
        float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
        const bool counted = !zeroLen;
        const float tw = T.woodcock(ray.dx, ray.dy, ray.dz, t, tt1, st, maj, s, counted);
        if (!zeroLen && (ae || (tw > t && tw < tt1))) {
          // AE: colour/alpha from the last accepted sample, zero if none (239-275)
          cr = s.x * A.amb.x * A.ambRad;
          cg = s.y * A.amb.y * A.ambRad;
          cb = s.z * A.amb.z * A.ambRad;
          alpha = s.w > 0.f ? 1.f : 0.f;
          i = 2;  // done: no further ranges
          break;
        }
      }
      if (lastRange) break;  // every later leaf of the last range is zero-length
      int4 dd;               // {packed steps, ex, ey, ez}
      if (iter == 0) {
        // exit point, step and stop (ShellAccel.h:125-132), first needed now
        const float e2 = upper - sceneEPS;
        float r2, la2, lo2;
        to_spherical(ray.ox + ray.dx * e2, ray.oy + ray.dy * e2, ray.oz + ray.dz * e2, r2, la2, lo2);
        const float4 en = lds_ld16(&s_entry[tid]);
        const float r1 = en.x, la1 = en.y, lo1 = en.z;
        const int sx = r1 < r2 ? 1 : -1, sy = la1 < la2 ? 1 : -1, sz = lo1 < lo2 ? 1 : -1;
        dd.x = (sx > 0 ? 1 : 0) | (sy > 0 ? 2 : 0) | (sz > 0 ? 4 : 0);
        dd.y = (int)((uint32_t)project_axis(r2, A.sbLo.x, A.sbHi.x, A.dims.x) + (uint32_t)sx);
        dd.z = (int)((uint32_t)project_axis(la2, A.sbLo.y, A.sbHi.y, A.dims.y) + (uint32_t)sy);
        dd.w = (int)((uint32_t)project_axis(lo2, A.sbLo.z, A.sbHi.z, A.dims.z) + (uint32_t)sz);
        s_dda[tid] = dd;
      } else {
        dd = s_dda[tid];
      }
      const float t_closest = fminf(fminf(tnx, tny), tnz);
      if (tnx == t_closest) {
        cx += (dd.x & 1) ? 1 : -1;
        if (cx == dd.y) break;
      }
      if (tny == t_closest) {
        cy += (dd.x & 2) ? 1 : -1;
        if (cy == dd.z) break;
      }
      if (tnz == t_closest) {
        cz += (dd.x & 4) ? 1 : -1;
        if (cz == dd.w) break;
      }
      t = t_closest;
    }
  }
  if (sampleOut)
    *sampleOut = make_float4(cr, cg, cb, alpha);
  else
    write_pixel(A, px.outIdx, cr, cg, cb, alpha, s_th);
}

// toSpherical (ICONGrid.h:36-42) of an sdda entry or exit point with the certified fast
// lat/lon (irt_device.h): r exactly, lat/lon within kLatErr/kLonErr of glibc's, and the
// point's shell-grid cells (ShellAccel.h:121-124, 128-130).  Returns false when a cell is
// not certified (the caller takes the glibc-exact path, to_spherical).
__device__ __forceinline__ bool spherical_fast(const RenderArgs &A, float x, float y, float z, float &r, float &la,
                                               float &lo, int &cy, int &cz) {
  r = sqrtf(dot3(x, y, z, x, y, z));
  la = fast_asin(z / r);  // z / r rounds as toSpherical's
  const bool okLon = fast_atan2(y, x, lo);
  const bool okY = cell_certified(la, kLatErr, A.sbLo.y, A.invSb[1], A.dims.y, cy);
  const bool okZ = cell_certified(lo, kLonErr, A.sbLo.z, A.invSb[2], A.dims.z, cz);
  return okY && okZ && okLon;
}

// render_pixel restated as a per-lane state machine whose one Woodcock call site is reached
// by the whole wave together (Tracer::woodcock_wave): each lane runs its ranges and sdda
// leaves on its own until it needs a woodcockFunc on a leaf (kWait) or is finished
// (kDone); then the wave tracks every waiting lane's leaf at once, and each lane resumes
// with the leaf's outcome.  Every lane of the wave calls it (those without a pixel start
// finished).  Same ranges, leaves, draws and results as render_pixel, step for step.

template <int OPT>
__device__ __forceinline__ void render_pixel_coop(const RenderArgs &A, Tracer<OPT> &T, const Pixel &px,
                                                  const float *s_th, int4 *s_dda, float4 *s_entry,
                                                  float4 *s_acc, CoopWave &W, ScanWave *SW, const uint2 *jmp,
                                                  int tid, int accumID, uint32_t blk, int pwave, int frame,
                                                  int partSel = -1, uint32_t interior = 0u) {
  // At 5+ waves/SIMD the pixel's output addresses are recomputed where they are used (from the
  // workgroup's uniform block index), not held in VGPRs through the rounds: a progressive
  // batch's sample slot (k_accumulate reads it) and the frame index.  (At 4 waves there is
  // room for them, and recomputing costs 1 %: profiles/r03u_waves/.)
  constexpr bool kRecompute = ((OPT >> 8) & 15) >= 5;
  // the pixel's thread index within its 256-pixel block: the packet's wave pwave (uniform) of
  // the block, and the lane (tid is the LDS index within this workgroup: a persistent launch's
  // wave renders any packet; OPT_WAVEWG has four one-wave workgroups per block)
  const int ptid = pwave * 64 + (tid & 63);
  // ... and so is the thread index itself after the rounds: the wave's base (uniform, an SGPR)
  // plus the lane id, instead of tid and the pixel's in-block coordinates held in scratch
  // across the rounds (24 B per lane of spill stores and reloads at 5 waves)
  const int wbase = __builtin_amdgcn_readfirstlane(tid) & ~63;
  auto tid_late = [&]() { return kRecompute ? (opaque_u(wbase) | (int)__lane_id()) : tid; };
  auto ptid_late = [&]() {
    if constexpr (!kRecompute) return ptid;
    int lane = (int)__lane_id();
    asm volatile("" : "+v"(lane));  // not CSE'd with the pixel's coordinates at the ray's start
    if (partSel >= 0) {  // a split packet's part (k_render): pn rays from ray part * pn
      const int ps = opaque_u(partSel), pn = 64 >> (ps & 255);
      lane = ((ps >> 8) * pn) | (lane & (pn - 1));
    }
    return (opaque_u(pwave) << 6) | lane;
  };
  const bool toSample = A.numSamples > 1 && !A.chain;
  // chained frames: frame f > 0 of the launch reads its accum pixel at the end, once frame
  // f - 1's wave has published it (chain_wait); frame 0 prefetches it as a single frame does
  const bool chainLate = A.chain && frame > 0;
  // ... unless frame f - 1's wave has published by the time this wave's rays are set up (a
  // large frame's previous-frame workgroup ran numBlocks workgroups earlier): its publish word,
  // loaded now, compared after the box test, and then the accum pixel prefetched (sc1) as frame 0
  uint32_t chainSeen = 0u;
  if (chainLate)
    chainSeen = __hip_atomic_load(A.chainFlag + (size_t)blk * 4u + (uint32_t)pwave, __ATOMIC_RELAXED,
                                  __HIP_MEMORY_SCOPE_AGENT);
  float4 *const slot0 = kRecompute || !toSample
                            ? nullptr
                            : A.sampleBuf + (size_t)frame * A.numTiles * 4096u + (size_t)blk * 256u + (size_t)ptid;
  auto sample_slot = [&]() {
    if constexpr (!kRecompute) return slot0;
    return A.sampleBuf + (size_t)opaque_u(frame) * opaque_u(A.numTiles) * 4096u + (size_t)opaque_u((int)blk) * 256u +
           (size_t)ptid_late();
  };
  enum : int { kRange, kLeaf, kWait, kDone, kGrid, kGridNext };
  constexpr bool kFastSph = (OPT & OPT_FASTSPH) != 0;
  constexpr bool grid = (OPT & OPT_GRID) != 0;
  const bool ae = A.raygen == 1;
  uint32_t st = 0;
  float dx = 1.f, dy = 1.f, dz = 1.f;
  float rlo0 = 0.f, rhi0 = 0.f, rlo1 = __builtin_inff(), rhi1 = -__builtin_inff();
  int numRanges = 0, phase = kDone;
  bool inBox = false;
  float t0box = 0.f, t1box = 0.f;
  if (px.active) {
    gen_ray(A, accumID, px.x, px.y, st, dx, dy, dz, frame);
    const float3 O = cam_org(A, frame);
    const Ray ray = {O.x, O.y, O.z, 0.f, dx, dy, dz, 1e10f};
    // Interior packets (host/irt_void.cpp section 4; the OPT_VOID kernels): every
    // ray of the packet passes boxTest, hits both spheres and takes the front-and-back ranges, so
    // the wave -- one scalar branch the compiler cannot see through -- skips the box test, the
    // d < 0 exits, the range selection and the fallback divisions.  The ranges are those the
    // general path below gives such a ray, bit for bit; both paths join before the state machine.
    bool setUp = false;
    if constexpr ((OPT & OPT_VOID) != 0) {
      uint32_t iu = __builtin_amdgcn_readfirstlane(interior);
      if constexpr ((OPT & OPT_VLIST) == 0) {
        // the bitmap form: the packet's bit of the second bitmap, behind the first one's 2 numTiles words
        const RenderArgs &BA = fresh_args();
        const uint32_t pkt = (uint32_t)opaque_u((int)blk) * 4u + (uint32_t)opaque_u(pwave);
        iu = BA.voidBits && BA.interior
                 ? (scalar_word(BA.voidBits, 2u * (uint32_t)BA.numTiles + (pkt >> 5)) >> (pkt & 31u)) & 1u
                 : 0u;
        iu = __builtin_amdgcn_readfirstlane(iu);
      }
      asm volatile("" : "+s"(iu));
      if (iu) {
        setUp = true;
        inBox = true;
        phase = kRange;
        if (!toSample && !chainLate && (OPT & OPT_LEAN) == 0)
          __builtin_amdgcn_global_load_lds((const void *)(A.accum + px.outIdx),
                                           (__attribute__((address_space(3))) void *)(s_acc + (tid & ~63)),
                                           16, 0, kRecompute ? 2 : 0);
        const RenderArgs &IA = fresh_args();
        float st1, st2, st3, st4;
        intersect_spheres_interior(ray, IA.sbHi.x, IA.sbLo.x, st1, st4, st2, st3);
        rlo0 = st1; rhi0 = st2;
        rlo1 = st3; rhi1 = st4;
        numRanges = 2;
      }
    }
    if (!setUp) {
    float t0, t1;
    const bool boxHit = box_test(ray, A, t0, t1);
#ifdef IRT_PROBE_BUILD
    // measurement only (30): 200 extra VALU instructions per wave in the ray setup -- is the
    // frame's time sensitive to VALU work at all?
    if (A.probeExit == 30) {
#pragma nounroll
      for (int k = 0; k < 50; ++k) asm volatile("v_nop\n v_nop\n v_nop\n v_nop" ::: "memory");
    }
#endif
    if (A.probeExit == 3) {  // measurement only: ray generation and boxTest, nothing written
      if (boxHit && t0 == -1.2345f) A.fb[0] = 0u;  // keeps the work live
      return;
    }
    if (boxHit) {
      inBox = true;  // counted at the ray's end: an LDS add here would wait for the prologue's LDS-DMA
      phase = kRange;
      t0box = t0;
      t1box = t1;
      // the accum pixel the lerp reads at the end, fetched now straight into LDS (no VGPRs
      // held through the Woodcock rounds; its latency hides behind them)
      if (!toSample && !chainLate && (OPT & OPT_LEAN) == 0)
        __builtin_amdgcn_global_load_lds((const void *)(A.accum + px.outIdx),
                                         (__attribute__((address_space(3))) void *)(s_acc + (tid & ~63)),
                                         16, 0, kRecompute ? 2 : 0);  // 2: nt (write_pixel)
      rlo0 = t0;
      rhi0 = t1;
      numRanges = 1;
      if (!ae) {  // the shell's sphere ranges, as render_pixel
        float st1 = 0.f, st2 = 0.f, st3 = 0.f, st4 = 0.f;
        bool s1, s2;
        intersect_spheres(ray, A.sbHi.x, A.sbLo.x, s1, st1, st4, s2, st2, st3);
        numRanges = 0;
        if ((s1 || s2) && !(st4 < t0)) {
          numRanges = 2;
          if (s1 && !s2) {
            rlo0 = st1; rhi0 = st4;
          } else if (t0 < st2) {
            rlo0 = st1; rhi0 = st2;
            rlo1 = st3; rhi1 = st4;
          } else {
            rlo0 = st3; rhi0 = st4;
          }
        }
      }
    } else if (toSample) {
      *sample_slot() = make_float4(0.f, 0.f, 0.f, kNoSample);  // deviceCode.cu:294-295
    }
    }  // !setUp
  }
  const bool chainReady = !chainLate || __builtin_amdgcn_readfirstlane(chainSeen) == A.chainEpoch + (uint32_t)frame;
  if ((OPT & OPT_LEAN) == 0 && chainLate && chainReady && inBox)
    __builtin_amdgcn_global_load_lds((const void *)(A.accum + px.outIdx),
                                     (__attribute__((address_space(3))) void *)(s_acc + (tid & ~63)), 16, 0, 16);  // sc1
  // GRID_ACCEL_MODE (deviceCode.cu:326-328): dda3 (DDA.h:35-136) over the 256^3 grid as
  // render_grid walks it, each cell's woodcockFunc one of the wave's cooperative requests
  int gcx = 0, gcy = 0, gcz = 0, gsteps = 0, gdirs = 0;
  float gtnx = 0.f, gtny = 0.f, gtnz = 0.f, gdx = 0.f, gdy = 0.f, gdz = 0.f, gtmax = 0.f, grtmin = 0.f,
        gtc0 = 0.f, gtc1 = 0.f;
  if constexpr (grid) {
    if (phase == kRange && !ae) {
      const float rtmin = t0box, rtmax = t1box;  // the box interval [t0, t1]
      const int D = kGridDim;
      const float3 O = cam_org(A, frame);
      const float ox = O.x + rtmin * dx, oy = O.y + rtmin * dy, oz = O.z + rtmin * dz;
      gtmax = rtmax - rtmin;
      grtmin = rtmin;
      const float rx = 1.f / dx, ry = 1.f / dy, rz = 1.f / dz;
      const float lx = (A.bmin.x - ox) * rx, ly = (A.bmin.y - oy) * ry, lz = (A.bmin.z - oz) * rz;
      const float hx = (A.bmax.x - ox) * rx, hy = (A.bmax.y - oy) * ry, hz = (A.bmax.z - oz) * rz;
      float nx = fminf(lx, hx), ny = fminf(ly, hy), nz = fminf(lz, hz);
      const float fx = fmaxf(lx, hx), fy = fmaxf(ly, hy), fz = fmaxf(lz, hz);
      if (dx == 0.f) nx = IRT_FLT_MAX;
      if (dy == 0.f) ny = IRT_FLT_MAX;
      if (dz == 0.f) nz = IRT_FLT_MAX;
      gcx = project_on_grid(ox, A.bmin.x, A.bmax.x, D);
      gcy = project_on_grid(oy, A.bmin.y, A.bmax.y, D);
      gcz = project_on_grid(oz, A.bmin.z, A.bmax.z, D);
      gdx = fmaxf(0.f, (fx - nx) / (float)D);
      gdy = fmaxf(0.f, (fy - ny) / (float)D);
      gdz = fmaxf(0.f, (fz - nz) / (float)D);
      gdirs = (dx > 0.f ? 1 : 0) | (dy > 0.f ? 2 : 0) | (dz > 0.f ? 4 : 0);
      gtnx = dx > 0.f ? nx + (float)(gcx + 1) * gdx : nx + (float)(D - gcx) * gdx;
      gtny = dy > 0.f ? ny + (float)(gcy + 1) * gdy : ny + (float)(D - gcy) * gdy;
      gtnz = dz > 0.f ? nz + (float)(gcz + 1) * gdz : nz + (float)(D - gcz) * gdz;
      phase = kGrid;
    }
  }
  // sceneEPS (ShellAccel.h:121-127), recomputed where it is used (a VALU product the
  // compiler would otherwise hold in a VGPR through every loop)
  auto sceneEPS = [&]() {
    const RenderArgs &SA = fresh_args();
    return opaque_u(SA.sbLo.x) * 1e-6f;
  };
  int i = 0, iter = 0, cx = 0, cy = 0, cz = 0;
  float t = 0.f, upper = 0.f, tt1 = 0.f, maj = 0.f;
  bool lastRange = true, zeroLen = false, hit = false;
  bool miss = false;  // the cooperative loop's speculation mode, carried from leaf to leaf
  bool first = true;  // OPT_TIMING
  // after a leaf without a hit: the next leaf of the range, or the next range
  // (render_pixel's loop tail, ShellAccel.h:201-226)
  auto next_leaf = [&]() {
    const RenderArgs &SA = fresh_args();
    if (lastRange) {  // every later leaf of the last range is zero-length
      ++i;
      phase = kRange;
      return;
    }
    const float tnx = upper, tny = 0.f, tnz = 0.f;
    int4 dd;
    if (iter == 0) {
      // exit point, step and stop (ShellAccel.h:125-132); the entry's (r1, la1, lo1, lower)
      // wait in s_entry.  OPT_FASTSPH: the certified fast lat/lon (spherical_fast).
      const float e2 = upper - sceneEPS();
      float r2, la2, lo2;
      int cy2 = 0, cz2 = 0;
      bool ok2 = false;
      const float3 O = cam_org(SA, frame);
      if constexpr (kFastSph)
        ok2 = spherical_fast(A, O.x + dx * e2, O.y + dy * e2, O.z + dz * e2, r2, la2, lo2, cy2, cz2);
      else
        to_spherical(O.x + dx * e2, O.y + dy * e2, O.z + dz * e2, r2, la2, lo2);
      const float4 en = lds_ld16(&s_entry[tid_late()]);
      const float r1 = en.x;
      const int sx = r1 < r2 ? 1 : -1;
      int sy, sz;
      if constexpr (!kFastSph) {
        sy = en.y < la2 ? 1 : -1;
        sz = en.z < lo2 ? 1 : -1;
        cy2 = project_axis_inv(la2, SA.sbLo.y, SA.invSb[1], SA.dims.y);
        cz2 = project_axis_inv(lo2, SA.sbLo.z, SA.invSb[2], SA.dims.z);
      } else {
        sy = sign_certified(en.y, la2, kLatErr);
        sz = sign_certified(en.z, lo2, kLonErr);
      }
      if (kFastSph && (!ok2 || sy == 0 || sz == 0)) {  // not certified (rare): both points glibc-exact
        float la1 = 0.f, lo1 = 0.f;
#pragma nounroll
        for (int k = 0; k < 2; ++k) {  // the entry, then the exit point (one inlined copy)
          const float e = k == 0 ? en.w + sceneEPS() : upper - sceneEPS();
          float rr, la, lo;
          to_spherical(O.x + dx * e, O.y + dy * e, O.z + dz * e, rr, la, lo);
          if (k == 0) {
            la1 = la;
            lo1 = lo;
          } else {
            la2 = la;
            lo2 = lo;
          }
        }
        sy = la1 < la2 ? 1 : -1;
        sz = lo1 < lo2 ? 1 : -1;
        cy2 = project_axis_inv(la2, SA.sbLo.y, SA.invSb[1], SA.dims.y);
        cz2 = project_axis_inv(lo2, SA.sbLo.z, SA.invSb[2], SA.dims.z);
      }
      dd.x = (sx > 0 ? 1 : 0) | (sy > 0 ? 2 : 0) | (sz > 0 ? 4 : 0);
      dd.y = (int)((uint32_t)project_axis_inv(r2, SA.sbLo.x, SA.invSb[0], SA.dims.x) + (uint32_t)sx);
      dd.z = (int)((uint32_t)cy2 + (uint32_t)sy);
      dd.w = (int)((uint32_t)cz2 + (uint32_t)sz);
      lds_st16(&s_entry[tid_late()], __builtin_bit_cast(float4, dd));  // the entry point is not needed again
    } else {
      dd = __builtin_bit_cast(int4, lds_ld16(&s_entry[tid_late()]));
    }
    const float t_closest = fminf(fminf(tnx, tny), tnz);
    bool stop = false;
    if (tnx == t_closest) {
      cx += (dd.x & 1) ? 1 : -1;
      stop = cx == dd.y;
    }
    if (!stop && tny == t_closest) {
      cy += (dd.x & 2) ? 1 : -1;
      stop = cy == dd.z;
    }
    if (!stop && tnz == t_closest) {
      cz += (dd.x & 4) ? 1 : -1;
      stop = cz == dd.w;
    }
    t = t_closest;
    if (stop || ++iter >= (1 << 22)) {
      ++i;
      phase = kRange;
    } else {
      phase = kLeaf;
    }
  };
  while (true) {
    if constexpr (grid) {
      // this lane's dda3 cells, on its own: up to the next one whose woodcockFunc can act
      const int D = kGridDim;
      constexpr int NB = kGridDim / kGridBlock;
      while (phase == kGrid || phase == kGridNext) {
        if (phase == kGridNext) {  // the step to the next cell (render_grid)
          const float tmn = fminf(fminf(gtnx, gtny), gtnz);
          bool out = false;
          if (gtnx == tmn) {
            gtnx += gdx;
            gcx += (gdirs & 1) ? 1 : -1;
            out = gcx == ((gdirs & 1) ? D : -1);
          }
          if (!out && gtny == tmn) {
            gtny += gdy;
            gcy += (gdirs & 2) ? 1 : -1;
            out = gcy == ((gdirs & 2) ? D : -1);
          }
          if (!out && gtnz == tmn) {
            gtnz += gdz;
            gcz += (gdirs & 4) ? 1 : -1;
            out = gcz == ((gdirs & 4) ? D : -1);
          }
          gtc0 = gtc1;
          if (out || ++gsteps >= 4 * D + 16) {
            phase = kDone;
            break;
          }
          phase = kGrid;
        }
        const float tmn = fminf(fminf(gtnx, gtny), gtnz);  // reduce_min (vecmath.h:512-514)
        gtc1 = dda3_min_quirk(tmn, gtmax);
        // a cell whose block holds no majorant above 0 (k_grid_bits), or whose own majorant
        // is <= 0: woodcockTracking returns at once (deviceCode.cu:161-162), nothing to do
        const bool inGrid = (unsigned)gcx < (unsigned)D && (unsigned)gcy < (unsigned)D && (unsigned)gcz < (unsigned)D;
        const uint32_t gb = inGrid ? ((uint32_t)(gcz / kGridBlock) * NB + (uint32_t)(gcy / kGridBlock)) * NB +
                                         (uint32_t)(gcx / kGridBlock)
                                   : 0u;
        if (!inGrid || ((T.s_gbits[gb >> 5] >> (gb & 31)) & 1u)) {
          maj = A.gridMaxOp[(size_t)gcz * D * D + (size_t)gcy * D + gcx];
          if (!(maj <= 0.f)) {
            t = grtmin + gtc0;  // woodcockFunc(leaf, ray_tmin + t0, ray_tmin + t1)
            tt1 = grtmin + gtc1;
            zeroLen = t == tt1;  // counted = !(w0 == w1)
            phase = kWait;
            break;
          }
        }
        phase = kGridNext;
      }
    }
    // this lane, on its own: up to its next woodcockFunc, or to the end
    while (phase == kRange || phase == kLeaf) {
      const RenderArgs &SA = fresh_args();
      if (phase == kRange) {
        if (i >= numRanges) {
          phase = kDone;
          break;
        }
        const float lower = i ? rlo1 : rlo0;
        upper = i ? rhi1 : rhi0;
        if (upper <= lower) {  // box1f::empty (vecmath.h:981)
          phase = kDone;
          break;
        }
        lastRange = ae || i == 1 || rhi1 <= rlo1;
        cx = cy = cz = 0;
        if (!ae) {  // cellID of the entry point (ShellAccel.h:121-124)
          const float e1 = lower + sceneEPS();
          const float3 O = cam_org(SA, frame);
          const float x1 = O.x + dx * e1, y1 = O.y + dy * e1, z1 = O.z + dz * e1;
          float r1, la1, lo1;
          // OPT_FASTSPH: the certified fast lat/lon, glibc-exact when not certified
          if (!(kFastSph && spherical_fast(A, x1, y1, z1, r1, la1, lo1, cy, cz))) {
            to_spherical(x1, y1, z1, r1, la1, lo1);
            cy = project_axis_inv(la1, SA.sbLo.y, SA.invSb[1], SA.dims.y);
            cz = project_axis_inv(lo1, SA.sbLo.z, SA.invSb[2], SA.dims.z);
          }
          cx = project_axis_inv(r1, SA.sbLo.x, SA.invSb[0], SA.dims.x);
          // for the exit's step (sign_certified) and its exact fallback (`lower`)
          if (!lastRange) lds_st16(&s_entry[tid_late()], make_float4(r1, la1, lo1, lower));
        }
        t = lower;
        iter = 0;
        phase = kLeaf;
      }
      // the leaf [t, tt1] (tnext = {upper, 0, 0}: render_pixel)
      tt1 = IRT_FLT_MAX;
      if (ae) {
        tt1 = upper;
      } else {
        if (upper < tt1 && upper >= t) tt1 = upper;
        if (0.f < tt1 && 0.f >= t) tt1 = 0.f;
      }
      zeroLen = tt1 == t;
      if (zeroLen && lastRange) {
        ++i;
        phase = kRange;
        continue;
      }
      if (!ae && zeroLen && iter >= 1 && upper > 0.f) {
        // The zero-length leaves after a non-last range's first leaf (see render_pixel): with
        // upper > 0 the walk steps cy and cz together (tnext = {upper, 0, 0}, t = 0) until one reaches its
        // stop, and each leaf only reads its majorant and, if positive, consumes one draw
        // (deviceCode.cu:161-166, the fast path above).  The leaves are known in advance, so
        // their majorants are gathered kWalk at a time (independent loads, one round trip)
        // instead of one dependent gather per leaf; the draws are then applied in order, and
        // a leaf that needs the full woodcockFunc (its draw's low 24 bits zero, or q out of
        // range) is handed to the single-leaf path below.  Same leaves, draws and state.
        const int4 dd = __builtin_bit_cast(int4, lds_ld16(&s_entry[tid_late()]));
        const int sy = (dd.x & 2) ? 1 : -1, sz = (dd.x & 4) ? 1 : -1;
        const int ky = (dd.z - cy) * sy, kz = (dd.w - cz) * sz;  // leaves left: min(ky, kz)
        if (ky >= 1 && kz >= 1 && iter + min(ky, kz) < (1 << 22)) {
          constexpr int kWalk = 8;
          const int n = min(min(ky, kz), kWalk);
          const int dimx = opaque_u(SA.dims.x), dimy = opaque_u(SA.dims.y);
          const uint32_t wx = (uint32_t)wrap_coord(cx, dimx);
          float mj[kWalk];
#pragma unroll
          for (int j = 0; j < kWalk; ++j) {
            mj[j] = 0.f;
            if (j < n) {
              const uint32_t leaf = (uint32_t)wrap_coord(cz + j * sz, SA.dims.z) * (uint32_t)dimx * (uint32_t)dimy +
                                    (uint32_t)wrap_coord(cy + j * sy, dimy) * (uint32_t)dimx + wx;
              mj[j] = SA.maxOp[leaf];
            }
          }
          int done = n;  // leaves taken by the fast path
#pragma unroll
          for (int j = 0; j < kWalk; ++j) {
            if (j < done) {
              const float q = mj[j] / SA.unitDistance;
              const uint32_t nx = lcg_next(st);
              if (!(mj[j] > 0.f)) {
              } else if (q > 0.f && q <= 1e30f && (nx & 0x00FFFFFFu) != 0u) {
                st = nx;
              } else {
                done = j;  // this leaf needs woodcockFunc: the single-leaf path takes it
              }
            }
          }
          if constexpr ((OPT & OPT_STATS) != 0) T.cnt.deg += (uint32_t)done;
          cy += done * sy;
          cz += done * sz;
          iter += done;
          if (done == min(ky, kz)) {  // the walk's stop (render_pixel's loop tail)
            ++i;
            phase = kRange;
            continue;
          }
          if (done == n) continue;  // the next batch
        }
      }
      if constexpr ((OPT & OPT_STATS) != 0) T.cnt.deg += zeroLen ? 1u : 0u;
      maj = 1.f;
      if (!ae) {
        const uint32_t leaf = (uint32_t)wrap_coord(cz, SA.dims.z) * (uint32_t)SA.dims.x * (uint32_t)SA.dims.y +
                              (uint32_t)wrap_coord(cy, SA.dims.y) * (uint32_t)SA.dims.x +
                              (uint32_t)wrap_coord(cx, SA.dims.x);
        maj = SA.maxOp[leaf];
      }
      bool fast = false;
      if (zeroLen) {
        const float q = maj / SA.unitDistance;
        const uint32_t nx = lcg_next(st);
        if (!(maj > 0.f)) {
          fast = true;
        } else if (q > 0.f && q <= 1e30f && (nx & 0x00FFFFFFu) != 0u) {
          st = nx;
          fast = true;
        }
      }
      if (!fast) {
        phase = kWait;
        break;
      }
      next_leaf();
    }
    // the wave, together: woodcockFunc(leafID, t, tt1) of every waiting lane
    const bool req = phase == kWait;
    if (__ballot(req) == 0ull) break;
    if (A.probeExit == 4) break;  // measurement only: ray setup up to the first woodcockFunc
    float tw = t;
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
    if constexpr ((OPT & OPT_TIMING) != 0) {
      if (first) {
        T.tmark(1);  // ray setup up to the first woodcockFunc
        first = false;
      }
    }
    T.woodcock_wave(req, dx, dy, dz, tw, tt1, st, maj, !zeroLen, s, miss, W, SW, jmp);
    if (A.probeExit == 5) break;  // measurement only: the first woodcockFunc of every lane
#ifdef IRT_PROBE_BUILD
    if (A.probeExit >= 8 && A.probeExit < 16) break;  // (IRT_ROUND_PROBE)
#endif
    if (grid && req && phase == kWait && !ae) {
      if (tw > t && tw < tt1) {  // render_grid's hit test (deviceCode.cu:316)
        lds_st16(&s_entry[tid_late()], make_float4(s.x * A.amb.x * A.ambRad, s.y * A.amb.y * A.ambRad,
                                   s.z * A.amb.z * A.ambRad, s.w > 0.f ? 1.f : 0.f));
        hit = true;
        phase = kDone;
      } else {
        phase = kGridNext;
      }
    } else if (req) {
      if (!zeroLen && (ae || (tw > t && tw < tt1))) {
        // the colour waits in the lane's s_entry slot (free once it is finished)
        lds_st16(&s_entry[tid_late()], make_float4(s.x * A.amb.x * A.ambRad, s.y * A.amb.y * A.ambRad,
                                   s.z * A.amb.z * A.ambRad, s.w > 0.f ? 1.f : 0.f));
        hit = true;
        phase = kDone;
      } else {
        next_leaf();
      }
    }
  }
  // chained frames: every wave of frame f > 0 waits for frame f - 1's wave of its pixels -- also
  // a wave none of whose rays hit the box, so that the publish words advance in frame order and
  // frame f - 1's word covers every earlier frame's stores
  const RenderArgs &TA = fresh_args();  // the ray's end: chain wait, pixel write
  if (chainLate && !chainReady) chain_wait(TA, blk, pwave, frame);
  {
    const uint64_t ib = __ballot(inBox);  // rays in the box (T.count(1) at the box test)
    if (ib && __lane_id() == (unsigned)__builtin_ctzll(ib)) atomicAdd(&T.s_cnt[1], (uint32_t)__popcll(ib));
  }
  // the pixel write decides here which launch forms skip a non-final frame's RGBA8 (chain_skips_fb:
  // chained progressive frames of one camera); the split-packet kernels keep their code as it was,
  // and so do the slot-table kernels, which write fb in every frame: with the skip and the replay
  // their hole-free form spilled 69 SGPRs instead of 63 and ran 0.4 % slower one launch per frame
  // at C3s and C5, with nothing gained chained (profiles/r07a_fbskip/)
  constexpr bool kFbSkip = (OPT & (OPT_SPLIT | OPT_SLOT)) == 0;
  if (!inBox) {
    if constexpr (kFbSkip) {
      // the launch's last frame, earlier ones having skipped fb: what an earlier hit left there
      if (chain_last_fb(TA, frame))
        chain_replay_fb(TA, (uint32_t)opaque_u((int)blk), ptid_late(), frame, s_th);
    }
    return;
  }
  const int tl = tid_late();
  const float4 c = hit ? lds_ld16(&s_entry[tl]) : make_float4(0.f, 0.f, 0.f, 0.f);
  if (toSample) {
    *sample_slot() = c;
  } else {
    const size_t outIdx = kRecompute ? pixel_of(TA, (uint32_t)opaque_u((int)blk), ptid_late()).outIdx : px.outIdx;
    if (TA.chain) {
      float4 old;
      if (chainLate && (!chainReady || (OPT & OPT_LEAN) != 0)) {
        old = chain_load_accum(TA, outIdx);
      } else if constexpr ((OPT & OPT_LEAN) != 0) {
        old = TA.accum[outIdx];
      } else {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the accum prefetch has landed
        old = lds_ld16(&s_acc[tl]);
      }
      // 1.f / (float)(accumID + 1) of this frame, correctly rounded as the host's TA.accumW
      write_pixel_chain(TA, outIdx, c.x, c.y, c.z, c.w, 1.f / (float)(accumID + 1), s_th, old,
                        frame < TA.numSamples - 1, !(kFbSkip && chain_skips_fb(TA, frame)));
    } else if constexpr ((OPT & OPT_LEAN) != 0) {
#ifdef IRT_PROBE_BUILD
      if (TA.probeExit == 6) {  // measurement only (probe build): the lerp without its accum read
        write_pixel(TA, outIdx, c.x, c.y, c.z, c.w, s_th, make_float4(0.f, 0.f, 0.f, 0.f));
        return;
      }
      if (TA.probeExit == 7) return;  // measurement only (probe build): no accum read, no pixel stores
#endif
      write_pixel(TA, outIdx, c.x, c.y, c.z, c.w, s_th);
    } else {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the accum prefetch has landed
      write_pixel<kRecompute>(TA, outIdx, c.x, c.y, c.z, c.w, s_th, lds_ld16(&s_acc[tl]));
    }
  }
}

}  // namespace irt
