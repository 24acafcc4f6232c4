// irt_tracer.h -- the raygen's sampling half, included by irt_raygen.h (one translation unit,
// irt_render.hip): the cube-map cell of a point (cubemap_cell_fast), the per-wave LDS records
// of the cooperative loop, the LDS-vector and DPP prefix helpers, the kernel-argument reads
// (fresh_args, the per-frame camera words) and Tracer<OPT> -- sampleVolume over each locator
// (locate, locate_wave, locate_wedge, locate_tri), classification, and woodcockTracking one lane
// per ray (woodcock) or for the whole wave together (woodcock_wave).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "irt_device.h"

namespace irt {

// cube-map cell of a sample point, and its sub-cell (irt_build.h).  The lists are
// rasterised with 1e-5 padding in face coordinates, so the hardware reciprocal (1 ulp) is
// exact enough: any (sub-)cell it picks lists every record that can contain the point.
// The kSubCells-times finer index is exact scaling by a power of two: its cell is the
// coarse grid's cell.
__device__ __forceinline__ uint32_t cubemap_cell_fast(float px, float py, float pz, int G,
                                                      uint32_t &sub) {
  const float ax = __builtin_fabsf(px), ay = __builtin_fabsf(py), az = __builtin_fabsf(pz);
  uint32_t face;
  float num0, num1, den;
  if (ax >= ay && ax >= az) {
    face = px >= 0.f ? 0u : 1u;
    num0 = py;
    num1 = pz;
    den = ax;
  } else if (ay >= az) {
    face = py >= 0.f ? 2u : 3u;
    num0 = px;
    num1 = pz;
    den = ay;
  } else {
    face = pz >= 0.f ? 4u : 5u;
    num0 = px;
    num1 = py;
    den = az;
  }
  const float inv = __builtin_amdgcn_rcpf(den);
  const int GS = opaque_u(G) * kSubCells;
  const float fg = 0.5f * (float)GS;
  int i = (int)((num0 * inv + 1.f) * fg);
  int j = (int)((num1 * inv + 1.f) * fg);
  i = i < 0 ? 0 : (i >= GS ? GS - 1 : i);
  j = j < 0 ? 0 : (j >= GS ? GS - 1 : j);
  sub = (uint32_t)((j & (kSubCells - 1)) * kSubCells + (i & (kSubCells - 1)));
  return face * (uint32_t)G * (uint32_t)G + (uint32_t)(j / kSubCells) * (uint32_t)G +
         (uint32_t)(i / kSubCells);
}
__device__ __forceinline__ uint32_t cubemap_cell_fast(float px, float py, float pz, int G) {
  uint32_t sub;
  return cubemap_cell_fast(px, py, pz, G, sub);
}

// Per-wave LDS of the cooperative Woodcock loop (Tracer::woodcock_wave).
struct CoopWave {
  float4 req[64];   // the request of the rank-r ray: {t, tmax, q = majorant/unitDistance, majorant}
  float4 ray[64];   // {dx, dy, dz, RNG state bits}
  float step[64];   // lane l's Woodcock step log(1 - xi)/q this round
  uint32_t cnt[64]; // the request is counted (a positive-length leaf)
};
// Per-wave LDS of Tracer::locate_wave's candidate scan
struct ScanWave {
  float4 pt[64];    // lane l's sample {point, r}
  uint4 lst[64];    // its candidate list {first entry, sub-cell mask, next position, record limit}
};

// t0 - d[0] - d[1] - ... - d[k], subtracted one at a time as woodcockTracking's `t -=`
// (deviceCode.cu:165) does: the same roundings as k+1 iterations of the serial loop.
typedef float fvec2 __attribute__((ext_vector_type(2)));
typedef float fvec4 __attribute__((ext_vector_type(4)));
// 16-byte LDS slots read and written as one ds_read_b128 / ds_write_b128: HIP's float4 and
// uint4 copy member-wise in IR, and with the IR load/store vectorizer off for this file
// (Makefile RENDER_FLAGS) they would split into b32 pairs.
template <class T>
__device__ __forceinline__ T lds_ld16(const T *p) {
  static_assert(sizeof(T) == 16, "16-byte slot");
  return __builtin_bit_cast(T, *reinterpret_cast<const fvec4 *>(p));
}
typedef uint32_t uvec2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint2 lds_ld8(const uint2 *p) {
  return __builtin_bit_cast(uint2, *reinterpret_cast<const uvec2 *>(p));
}
template <class T>
__device__ __forceinline__ void lds_st16(T *p, T v) {
  static_assert(sizeof(T) == 16, "16-byte slot");
  *reinterpret_cast<fvec4 *>(p) = __builtin_bit_cast(fvec4, v);
}
// The group's steps are read as explicit 4- / 2-float LDS vectors (the group base is a
// multiple of G floats), independent of the IR load/store vectorizer (off for this file).
template <int G>
__device__ __forceinline__ float coop_prefix(float t0, const float *d, int k) {
  float t = t0;
  if constexpr (G == 2) {
    const fvec2 v = *static_cast<const fvec2 *>(__builtin_assume_aligned(d, 8));
    t = t - v.x;
    t = k >= 1 ? t - v.y : t;
  } else {
#pragma unroll
    for (int c = 0; c < G / 4; ++c) {
      const fvec4 v = static_cast<const fvec4 *>(__builtin_assume_aligned(d, 16))[c];
      t = 4 * c <= k ? t - v.x : t;
      t = 4 * c + 1 <= k ? t - v.y : t;
      t = 4 * c + 2 <= k ? t - v.z : t;
      t = 4 * c + 3 <= k ? t - v.w : t;
    }
  }
  return t;
}

// The same prefix by DPP steps across the lanes of groups of G = 2, 4, 16 or 64 (OPT_DPPSCAN):
// lane k starts at t0 - d_k (final for k = 0), and step s sets y_k = y_{k-1} - d_k, so that after
// step s the lanes k <= s hold ((t0 - d0) - d1) - ... - dk, subtracted in the serial loop's order.
// A group's first lane reads itself (quad_perm) or has no source lane (row_shr / wave_shr with
// bound_ctrl off: the old value) and subtracts +0, which leaves every float as it is.
template <int G>
__device__ __forceinline__ float dpp_prefix(float t0, float dk, int k) {
  static_assert(G == 2 || G == 4 || G == 16 || G == 64, "DPP prefix: groups of 2, 4, 16, 64");
  constexpr int ctrl = G == 2 ? 0xA0 : G == 4 ? 0x90 : G == 16 ? 0x111 : 0x138;  // quad_perm [0,0,2,2] /
                                                                                // [0,0,1,2], row_shr:1,
                                                                                // wave_shr:1
  const float e = k == 0 ? 0.f : dk;
  float y = t0 - dk;
#pragma unroll
  for (int s = 1; s < G; ++s) {
    const float prev = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, y),
                                                                             __builtin_bit_cast(int, y), ctrl, 0xf,
                                                                             0xf, false));
    y = prev - e;
  }
  return y;
}

// Measurement only, the probe build (profiles/build_probe_lib.sh, -DIRT_PROBE_BUILD):
// IRT_PROBE_EXIT 8..13 end the first
// woodcockFunc call inside its first round -- 8 after the samples' positions, 9 after the
// header and bin, 10 after the first candidate test, 11 after the dealt-out candidates, 12 after
// locate_wave (getValue included), 13 at the round's end -- so that the SQ counters of runs
// with each exit give the instructions of every piece of a round (profiles/r06m_gpu.sh)
#ifdef IRT_PROBE_BUILD
#define IRT_ROUND_PROBE(n, ...) \
  if (A.probeExit == (n)) return __VA_ARGS__;
#else
#define IRT_ROUND_PROBE(n, ...)
#endif

// OPT_TIMING's per-wave region clocks (Tracer::tmark); empty in every other kernel
struct TimeAccOff {};
struct TimeAccOn {
  static constexpr int kTimeRegions = 9;
  uint64_t tLast = 0, tAcc[kTimeRegions] = {};
};

// The camera of frame `frame` of a launch: the launch's own, or in a sequence of views
// (RenderArgs::frameCams, irt_render_sequence) that frame's words, read through the constant
// address space (scalar loads: uniform values, written by the host before the launch).
typedef const __attribute__((address_space(4))) fvec4 *CamWords;
// a uniform word of a host-written table (tile lists, block orders) through the scalar unit: a
// vector load's wait would also wait for every vector load before it (the counter retires in
// order), the prologue's LDS-DMA table loads included
typedef const __attribute__((address_space(4))) uint32_t *ScalarWords;
__device__ __forceinline__ uint32_t scalar_word(const void *table, uint32_t i) {
  return ((ScalarWords)table)[i];
}
__device__ __forceinline__ float4 cam_word(const RenderArgs &A, int frame, int k) {
  return __builtin_bit_cast(float4, ((CamWords)A.frameCams)[4 * frame + k]);
}
__device__ __forceinline__ float3 cam_org(const RenderArgs &A, int frame) {
  if (A.frameCams) {
    const float4 w = cam_word(A, frame, 0);
    return make_float3(w.x, w.y, w.z);
  }
  return A.org;
}
// the frame's accumID (deviceCode.cu:288-289): accumID + frame in a progressive batch
__device__ __forceinline__ int cam_accum_id(const RenderArgs &A, int frame) {
  if (A.frameCams) return (int)__float_as_uint(cam_word(A, frame, 0).w);
  return A.accumID + frame;
}

// The ray's per-lane state machine reads RenderArgs through fresh_args(): k_render's only
// argument reached through a pointer the compiler cannot follow, so the fields it uses are
// loaded (scalar loads, scalar-cache hits) where it uses them instead of held in SGPRs -- or
// spilled to VGPR lanes -- through the Woodcock rounds; so does the ray's end (chain wait, pixel
// write).  108 -> 65 spilled SGPRs on flat grids, 120 -> 87 and no scratch over terrain; C3
// -1.5 %, C3t -2.4 % (one launch per frame -4.3 %), C3s -0.6 %, C5 even (profiles/r06s/, r06t/).
// The Tracer's late reads (classify_alpha, record_value, sphere_at, the sphere test) too: 62 and
// 73 spilled SGPRs, C3t -1.2 %, C5 -0.9 %, C3 and C3s even (profiles/r06v/).
__device__ __forceinline__ const RenderArgs &fresh_args() {
  typedef const __attribute__((address_space(4))) RenderArgs *KArgs;
  KArgs kp = (KArgs)__builtin_amdgcn_kernarg_segment_ptr();
  asm volatile("" : "+s"(kp));
  return *(const RenderArgs *)kp;
}

template <int OPT>
struct Tracer : std::conditional_t<(OPT & OPT_TIMING) != 0, TimeAccOn, TimeAccOff> {
  const RenderArgs &A;
  const LogfTab *s_logf;
  const uint32_t *s_sph;
  uint32_t *s_cnt;  // [0] launched [1] inBox [2] locate [3] found [4] candidates
  Counts cnt;       // per-lane statistics (OPT_STATS)
  uint32_t specCand = 0;  // candidate tests of this lane's sample in a cooperative round
  const uint32_t *s_gbits = nullptr;  // OPT_GRID: the grid's empty-space bitmap in LDS
  // the cooperative loop's statistics, per lane (samples taken, their locates / found /
  // candidate tests), added into s_cnt at the end by flush_coop
  uint32_t nLocate = 0, nFound = 0, nCand = 0;
  int frame = 0;  // the launch's frame this wave renders (its camera: cam_org)
  const RenderArgs *Ap = &A;  // the arguments its methods read
  // OPT_TIMING: shader clocks per region (wave-uniform), in the TimeAcc base
  __device__ __forceinline__ void tmark(int region) {
    if constexpr ((OPT & OPT_TIMING) != 0) {
      const uint64_t now = __builtin_amdgcn_s_memtime();
      this->tAcc[region] += now - this->tLast;
      this->tLast = now;
    }
  }

  // wave sum of a per-lane count: the DPP prefix sum's last lane (wave_incl_sum)
  __device__ __forceinline__ static uint32_t wave_sum(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_readlane((int)wave_incl_sum(v), 63);
  }
  // inclusive prefix sum over the wave's 64 lanes in six DPP adds (row shifts within rows of
  // 16, then the row broadcasts), no LDS round trips
  __device__ __forceinline__ static uint32_t wave_incl_sum(uint32_t v) {
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, false);  // row_shr:1
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, false);  // row_shr:2
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, false);  // row_shr:4
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, false);  // row_shr:8
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, false);  // row_bcast:15
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xc, 0xf, false);  // row_bcast:31
    return v;
  }
  __device__ __forceinline__ void flush_coop() {
    const uint32_t a = wave_sum(nLocate), b = wave_sum(nFound), c = wave_sum(nCand);
    if (__lane_id() == 0) {
      if (a) atomicAdd(&s_cnt[2], a);
      if (b) atomicAdd(&s_cnt[3], b);
      if (c) atomicAdd(&s_cnt[4], c);
    }
  }

  // the cooperative Woodcock loop (woodcock_wave) runs in every kernel (any sampler, either
  // accelerator) but the OPT_SERIAL comparison one
  static constexpr bool kCoop = (OPT & OPT_SERIAL) == 0;
  // the miss mode of woodcock_wave: after a sample outside every cell, a ray's next round
  // places its samples as if none were located, until one is.  Misses come in runs wherever
  // the volume has holes: the unstructured samplers' gaps, the grid accel's empty cells, and
  // in the user-geometry sampler the voids convert_icon leaves under land (a column's first
  // record starts at R + HSURF, convert_icon.cpp:361: nothing covers [R, R + HSURF)) -- at C3t a
  // third of the samples miss, in runs of up to ~280 draws, and without the miss mode every
  // miss cost its ray a round (single-frame launches 1.07 ms against 0.09 ms at C3, a few
  // waves running ~1 ms: profiles/r05d_missmode/).  Flat grids almost never miss (C3: 707 of 1.01 M
  // samples).  The kernels with misses everywhere (wedges, grid) start with whole-wave groups.
  static constexpr bool kMiss = kCoop && (OPT & OPT_NOMISS) == 0;
  // the void walk of woodcock_wave's solo miss-mode lanes (the user-geometry sampler from headers)
  static constexpr bool kVoidRun =
      kMiss && (OPT & (OPT_WEDGE | OPT_GRID | OPT_SCAN1 | OPT_SLOT | OPT_NOHOLESKIP | OPT_NOVOIDRUN)) == 0;
  static constexpr int kVoidRunMax = 32;  // samples one lane walks before the round goes on
  static constexpr bool kWideStart = (OPT & (OPT_WEDGE | OPT_GRID)) != 0;

  // one wave-aggregated LDS add per event site
  __device__ __forceinline__ void count(int k) {
    const unsigned long long m = __ballot(1);
    if (__lane_id() == (unsigned)(__ffsll((long long)m) - 1)) atomicAdd(&s_cnt[k], (uint32_t)__popcll(m));
  }

  // findHeight (ICONGrid.h:117-145) literally, over a record's blocks; getValue (147-164)
  __device__ __forceinline__ float find_value_literal(const float4 *B, int nl, float r) {
    const float *Bf = reinterpret_cast<const float *>(B);
    int first = 0, count = nl;
    while (count > 0) {
      const int stp = count / 2, it = first + stp;
      if (!(r <= Bf[blk_height_pos(it + 1)])) {
        first = it + 1;
        count -= stp + 1;
      } else {
        count = stp;
      }
    }
    return Bf[blk_value_pos(first)];
  }

  // sample()'s point test (ICONGrid.h:184, 197-203) on one fat entry {p0, p1, p2, m}:
  // the radial range and the three ccw side planes
  __device__ __forceinline__ bool pass_fat(const float4 &p0, const float4 &p1, const float4 &p2,
                                           const float4 &m, float px, float py, float pz, float r) {
    if constexpr (kCoop)
      ++specCand;  // counted only if the sample is one the reference takes (woodcock_wave)
    else
      count(4);
    if (r < m.x || r > m.y) return false;                                 // ICONGrid.h:184
    if (dot3(px, py, pz, p0.x, p0.y, p0.z) - p0.w > 0.f) return false;  // ICONGrid.h:201
    if (dot3(px, py, pz, p1.x, p1.y, p1.z) - p1.w > 0.f) return false;  // 202
    if (dot3(px, py, pz, p2.x, p2.y, p2.z) - p2.w > 0.f) return false;  // 203
    return true;
  }

  // The record a point test found: index and its getValue path at the sample's radius
  // (irt_common.h record_path: numLayers, which 64-B block, or the literal search).
  struct Found {
    uint32_t rec, path;
  };

  // First entry of fat entries [q, qe) whose point test passes, among records < limit:
  // of the first kMaskCand entries only those whose bit is set in `mask` (the candidates
  // that can reach the sample's sub-cell, irt_build.h), then every later one.  Only the
  // point test runs in the (lane-divergent) loop; getValue's gathers come after.
  __device__ __forceinline__ bool scan_fat(uint32_t q, uint32_t qe, uint32_t mask, uint32_t limit,
                                           float px, float py, float pz, float r, Found &f) {
    const uint32_t n = qe - q;
    for (uint32_t j = 0;; ++j) {
      if (j < (uint32_t)kMaskCand) {
        const uint32_t m = mask >> j;
        j = m ? j + (uint32_t)__builtin_ctz(m) : (uint32_t)kMaskCand;
      }
      if (j >= n) break;
      const float4 *F = (*Ap).fat + (size_t)(q + j) * kFatStride4;
      const float4 a0 = F[0], a1 = F[1], a2 = F[2], am = F[3];
      if (__float_as_uint(am.z) >= limit) return false;
      if (pass_fat(a0, a1, a2, am, px, py, pz, r)) {
        f = {__float_as_uint(am.z), record_path(__float_as_uint(am.w), am.x, am.y, r)};
        return true;
      }
    }
    return false;
  }

  // getValue (ICONGrid.h:147-164) of the found record at radius r: sorted heights take the
  // 64-B height/value block the quantised keys pick (one gather; r within a unit of a key:
  // the exact keys from the record's lines first), others the literal binary search
  __device__ __forceinline__ float record_value(const Found &f, float r) {
    const RenderArgs &LA = fresh_args();  // read where used
    const int nl = (int)(f.path & 31u);
    const float4 *B = LA.blocks + (size_t)f.rec * kBlk4;
    if (f.path & kPathBlock) {
      int b = (int)((f.path >> 5) & 3u);
      if (f.path & kPathExactKeys) {
        const float *Bf = reinterpret_cast<const float *>(B);
        b = rec_coarse_block(Bf[blk_height_pos(7)], Bf[blk_height_pos(15)], Bf[blk_height_pos(23)],
                             __builtin_inff(), nl, r);  // height[31] = hN >= r never counts
      }
      const float4 *Q = B + 4 * b;
      const float4 h0 = Q[0], h1 = Q[1], v0 = Q[2], v1 = Q[3];
      const int k = rec_block_index(h0.x, h0.y, h0.z, h0.w, h1.x, h1.y, h1.z, b, nl, r);
      return select8(k, v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w);
    }
    return find_value_literal(B, nl, r);
  }

  // A zero-thickness record at exactly radius r (a sphere, host/irt_scene.cpp), if any:
  // the lowest such record and its getValue.
  __device__ __forceinline__ bool sphere_at(float r, float &value, uint32_t &rec) {
    const RenderArgs &LA = fresh_args();  // read where used
    uint32_t lo = 0, hi = LA.numSph;
    while (lo < hi) {
      const uint32_t mid = (lo + hi) >> 1;
      if (LA.sphR[mid] < r) lo = mid + 1;
      else hi = mid;
    }
    if (lo >= LA.numSph || !(LA.sphR[lo] == r)) return false;
    const uint2 q = LA.sphRec[LA.sphOff[lo]];
    value = find_value_literal(LA.blocks + (size_t)q.x * kBlk4, (int)q.y, r);
    rec = q.x;
    return true;
  }

  // sampleVolume (deviceCode.cu:58-125) over the binned lists (irt_common.h): the first
  // record in index order passing sample() -- the reference's linear scan's answer
  // (116-123).
  // CUBQL_MODE sampleVolume (deviceCode.cu:90-115) over the wedge locator: the first wedge
  // in (record, layer) order whose primBounds (hostCode.cu:534-552) contain the point and
  // whose intersectWedgeEXT (UElems.h:214-311) accepts it.  Wedges are rebuilt in
  // registers from the record's corner trig and heights exactly as buildCuBQLAccel makes
  // them (hostCode.cu:557-590); a record's union box rejects it first.
  __device__ __forceinline__ bool locate_wedge(float px, float py, float pz, float &value) {
    const uint32_t cell = cubemap_cell_fast(px, py, pz, (*Ap).wG);
    const uint32_t qe = (*Ap).wOff[cell + 1];
    for (uint32_t q = (*Ap).wOff[cell]; q < qe; ++q) {
      const uint32_t rec = (*Ap).wRec[q];
      const float4 lo = (*Ap).wBox[2 * (size_t)rec], hi = (*Ap).wBox[2 * (size_t)rec + 1];
      if (!(lo.x <= px && px <= hi.x && lo.y <= py && py <= hi.y && lo.z <= pz && pz <= hi.z))
        continue;
      const int nl = (int)__float_as_uint(lo.w);
      const float4 t0 = (*Ap).wTrig[3 * (size_t)rec], t1 = (*Ap).wTrig[3 * (size_t)rec + 1],
                   t2 = (*Ap).wTrig[3 * (size_t)rec + 2];
      const float4 *B = (*Ap).blocks + (size_t)rec * kBlk4;
      const float *Bf = reinterpret_cast<const float *>(B);
      for (int h = 0; h < nl; ++h) {
        const float hb = Bf[blk_height_pos(h)], ht = Bf[blk_height_pos(h + 1)];
        WV4 V[6];
        V[0] = {(hb * t0.x) * t0.z, (hb * t0.x) * t0.w, hb * t0.y, 0.f};
        V[1] = {(hb * t1.x) * t1.z, (hb * t1.x) * t1.w, hb * t1.y, 0.f};
        V[2] = {(hb * t2.x) * t2.z, (hb * t2.x) * t2.w, hb * t2.y, 0.f};
        V[3] = {(ht * t0.x) * t0.z, (ht * t0.x) * t0.w, ht * t0.y, 0.f};
        V[4] = {(ht * t1.x) * t1.z, (ht * t1.x) * t1.w, ht * t1.y, 0.f};
        V[5] = {(ht * t2.x) * t2.z, (ht * t2.x) * t2.w, ht * t2.y, 0.f};
        float bl[3] = {1e31f, 1e31f, 1e31f}, bu[3] = {-1e31f, -1e31f, -1e31f};
#pragma unroll
        for (int k = 0; k < 6; ++k) {
          bl[0] = fminf(bl[0], V[k].x);
          bl[1] = fminf(bl[1], V[k].y);
          bl[2] = fminf(bl[2], V[k].z);
          bu[0] = fmaxf(bu[0], V[k].x);
          bu[1] = fmaxf(bu[1], V[k].y);
          bu[2] = fmaxf(bu[2], V[k].z);
        }
        if (!(bl[0] <= px && px <= bu[0] && bl[1] <= py && py <= bu[1] && bl[2] <= pz && pz <= bu[2]))
          continue;
        // the per-layer scalar (hostCode.cu:571-572) on all six vertices (`#if 1`, 574-577)
        const float bv = h == 0 ? find_value_literal(B, nl, hb)
                                : (find_value_literal(B, nl, Bf[blk_height_pos(h - 1)]) +
                                   find_value_literal(B, nl, hb)) * 0.5f;
#pragma unroll
        for (int k = 0; k < 6; ++k) V[k].w = bv;
        if (intersect_wedge(value, px, py, pz, V)) return true;
      }
    }
    return false;
  }

  // TRIANGLE_MODE sampleVolume (deviceCode.cu:61-76): the ray from the sample toward the
  // Earth's centre against the listed records' bottom triangles (hostCode.cu:445-450),
  // closest front-face hit (ray_triangle, irt_common.h), then its radial range and getValue.
  __device__ __forceinline__ bool locate_tri(float px, float py, float pz, float &value) {
    const float len = sqrtf(dot3(px, py, pz, px, py, pz));
    const float dx = -(px / len), dy = -(py / len), dz = -(pz / len);
    const uint32_t cell = cubemap_cell_fast(px, py, pz, (*Ap).wG);
    const uint32_t qe = (*Ap).wOff[cell + 1];
    float best = __builtin_inff();
    uint32_t hit = 0xFFFFFFFFu;
    for (uint32_t q = (*Ap).wOff[cell]; q < qe; ++q) {
      const uint32_t rec = (*Ap).wRec[q];
      const float4 t0 = (*Ap).wTrig[3 * (size_t)rec], t1 = (*Ap).wTrig[3 * (size_t)rec + 1],
                   t2 = (*Ap).wTrig[3 * (size_t)rec + 2];
      const float h0 = reinterpret_cast<const float *>((*Ap).blocks + (size_t)rec * kBlk4)[blk_height_pos(0)];
      const float v0[3] = {(h0 * t0.x) * t0.z, (h0 * t0.x) * t0.w, h0 * t0.y};
      const float v1[3] = {(h0 * t1.x) * t1.z, (h0 * t1.x) * t1.w, h0 * t1.y};
      const float v2[3] = {(h0 * t2.x) * t2.z, (h0 * t2.x) * t2.w, h0 * t2.y};
      float t;
      if (ray_triangle(px, py, pz, dx, dy, dz, v0, v1, v2, t) && t < best) {
        best = t;
        hit = rec;
      }
    }
    if (hit == 0xFFFFFFFFu) return false;
    const float4 *B = (*Ap).blocks + (size_t)hit * kBlk4;
    const float *Bf = reinterpret_cast<const float *>(B);
    const int nl = (int)__float_as_uint((*Ap).wBox[2 * (size_t)hit].w);
    if (len < Bf[blk_height_pos(0)] || len > Bf[blk_height_pos(nl)]) return false;
    value = find_value_literal(B, nl, len);
    return true;
  }

  __device__ __forceinline__ bool locate(float px, float py, float pz, float &value) {
    if ((*Ap).numCells == 0) return false;
    if constexpr ((OPT & OPT_WEDGE) != 0) {
      if ((*Ap).sampler == IRT_MODE_TRIANGLES) return locate_tri(px, py, pz, value);
      return locate_wedge(px, py, pz, value);
    }
    const float r = sqrtf(dot3(px, py, pz, px, py, pz));  // toSpherical(pos).x
    uint32_t sub;
    const uint32_t cell = cubemap_cell_fast(px, py, pz, (*Ap).G, sub);
    // the cell header's words 0..7 and the sub-cell's mask word: one 128-B line
    const uint4 *Hc = (*Ap).binHdr + (size_t)cell * (kBinHdrWords / 4);
    const uint4 H0 = Hc[0], H1 = Hc[1];
    const uint32_t M = reinterpret_cast<const uint32_t *>(Hc)[8 + sub];
    return locate_hdr(px, py, pz, r, H0, H1, M, value);
  }

  __device__ __forceinline__ bool locate_hdr(float px, float py, float pz, float r, const uint4 &H0,
                                             const uint4 &H1, uint32_t M, float &value) {
    const float e0 = __uint_as_float(H0.x), e1 = __uint_as_float(H0.y), e2 = __uint_as_float(H0.z);
    const int b = bin_of(r, e0, e1, e2);
    // bin b's [beg, end) from the cumulative ends, and its upper edge, selected with masks
    // (a select chain on b becomes a scratch lookup table otherwise)
    const uint32_t m1 = b > 0 ? ~0u : 0u, m2 = b > 1 ? ~0u : 0u, m3 = b > 2 ? ~0u : 0u;
    const uint32_t beg = (m1 & H1.x) + (m2 & (H1.y - H1.x)) + (m3 & (H1.z - H1.y));
    const uint32_t end = H1.x + (m1 & (H1.y - H1.x)) + (m2 & (H1.z - H1.y)) + (m3 & (H1.w - H1.z));
    const uint32_t end2 = H1.y + (m1 & (H1.z - H1.y)) + (m2 & (H1.w - H1.z));
    // r exactly on the bin's upper edge: records starting at that edge sit in the next
    // bin, so a second pass scans it for a lower record (one scan site, two passes)
    const float eb = __uint_as_float(H0.x ^ (m1 & (H0.x ^ H0.y)) ^ (m2 & (H0.y ^ H0.z)));
    const bool onEdge = b < kMaxEdges && r == eb;
    Found f = {0xFFFFFFFFu, 0u};
    bool hit = false;
    uint32_t qb = H0.w + beg, qe = H0.w + end;
    for (int pass = 0; pass < 2; ++pass) {
      Found g;
      if (scan_fat(qb, qe, (M >> (8 * (b + pass))) & 0xFFu, f.rec, px, py, pz, r, g)) {
        f = g;
        hit = true;
      }
      if (!onEdge) break;
      qb = qe;
      qe = H0.w + end2;
    }
    if ((*Ap).numSph) {
      const uint32_t h = sph_hash(r);
      if ((s_sph[h >> 5] >> (h & 31)) & 1u) {
        float v2;
        uint32_t rec2;
        if (sphere_at(r, v2, rec2) && (!hit || rec2 < f.rec)) {
          value = v2;
          return true;
        }
      }
    }
    if (hit) value = record_value(f, r);
    return hit;
  }

  // sampleVolume for every lane of the wave with `want` set (the cooperative loop's locate;
  // all lanes call it).  The same answer as locate: the first candidate of the sample's bin
  // and sub-cell, in record order, passing sample().  But the candidate scan is spread over
  // the wave: every lane first tests its list's first candidate (a quarter of C3's samples
  // fail it: 916,920 / 270,995 / 30,517 samples take 1 / 2 / >=3 tests), then the wave's
  // remaining candidates are dealt out one per lane and tested together, so a round waits
  // for two entry gathers instead of the longest lane's chain (2.96 per round at C3).  The
  // lowest passing candidate of each list wins, as in the serial scan.  Samples exactly on a
  // radial bin edge (the two-bin scan) take locate_hdr's serial path.
  static constexpr bool kWaveScan = kCoop && (OPT & (OPT_WEDGE | OPT_GRID | OPT_SCAN1)) == 0;
  __device__ __forceinline__ static bool entry_passes(const float4 &a0, const float4 &a1, const float4 &a2,
                                                     const float4 &am, float px, float py, float pz, float r) {
    return !(r < am.x || r > am.y) && !(dot3(px, py, pz, a0.x, a0.y, a0.z) - a0.w > 0.f) &&
           !(dot3(px, py, pz, a1.x, a1.y, a1.z) - a1.w > 0.f) && !(dot3(px, py, pz, a2.x, a2.y, a2.z) - a2.w > 0.f);
  }
  __device__ __forceinline__ bool pass_entry(const float4 *F, float px, float py, float pz, float r,
                                             Found &f) {
    const float4 a0 = F[0], a1 = F[1], a2 = F[2], am = F[3];
    f = {__float_as_uint(am.z), record_path(__float_as_uint(am.w), am.x, am.y, r)};
    if (r < am.x || r > am.y) return false;                               // ICONGrid.h:184
    if (dot3(px, py, pz, a0.x, a0.y, a0.z) - a0.w > 0.f) return false;  // ICONGrid.h:201
    if (dot3(px, py, pz, a1.x, a1.y, a1.z) - a1.w > 0.f) return false;  // 202
    if (dot3(px, py, pz, a2.x, a2.y, a2.z) - a2.w > 0.f) return false;  // 203
    return true;
  }
  // position p of a candidate list {set bits of m8, ascending} ++ {8, 9, ...} -> entry offset
  __device__ __forceinline__ static uint32_t list_entry(uint32_t m8, uint32_t p) {
    const uint32_t nm = (uint32_t)__popc(m8);
    if (p >= nm) return (uint32_t)kMaskCand + (p - nm);
    for (uint32_t k = 0; k < p; ++k) m8 &= m8 - 1u;
    return (uint32_t)__builtin_ctz(m8);
  }
  __device__ __forceinline__ bool locate_wave(bool want, float px, float py, float pz, float &value,
                                              CoopWave &CW, ScanWave &W) {
    want = want && (*Ap).numCells != 0;
    const int lane = (int)__lane_id();
    // The scan's state lives in the wave's LDS (fewer live VGPRs across it):
    //   W.pt[l]  the sample {point, r} of lane l
    //   W.lst[l] its list {first entry, sub-cell mask, next list position, record limit}
    //   frm[l]   the record found so far: {record, getValue path} (in the round's request
    //            slots CW.ray, free once the round has read them)
    //   W.own[s] the lane whose tasks start at s (W.step, free after the round's prefix)
    uint32_t *own = reinterpret_cast<uint32_t *>(CW.step);
    uint2 *frm = reinterpret_cast<uint2 *>(CW.ray);
    uint32_t c = 0u;
    uint32_t fe = 0u, flim = 0xFFFFFFFFu;  // the pass's first candidate entry, record limit
    float fr = 0.f;                        // the sample's r
    bool hit = false, edge = false;
    uint4 H0 = make_uint4(0u, 0u, 0u, 0u), H1 = H0;
    uint32_t M = 0u, cell = 0u, sub = 0u;
    constexpr bool kSlot = (OPT & OPT_SLOT) != 0;
    // the quad-bound miss test: scenes with holes (the miss-mode kernels) that start from headers
    constexpr bool kHoleSkip = kMiss && !kSlot && (OPT & OPT_NOHOLESKIP) == 0;
    float4 s0 = make_float4(0.f, 0.f, 0.f, 0.f), s1 = s0, s2 = s0, sm = s0;  // OPT_SLOT: the first candidate
    bool slotCopy = false;  // OPT_SLOT: the slot's copy is this sample's first admitted candidate
    if (kSlot && want) {
      // the slot of the sample's (cell, sub-cell, bin): the bins from the scene's shared edges
      const float r = sqrtf(dot3(px, py, pz, px, py, pz));  // toSpherical(pos).x
      cell = cubemap_cell_fast(px, py, pz, (*Ap).G, sub);
      const float e0 = (*Ap).slotEdge[0], e1 = (*Ap).slotEdge[1], e2 = (*Ap).slotEdge[2];
      const int b = bin_of(r, e0, e1, e2);
      const int subs = (*Ap).slotSubs;
      const uint32_t unit = slot_unit(sub, subs);
      const float4 *S = (*Ap).slots + ((size_t)(cell * ((uint32_t)(kSubCells * kSubCells) >> (subs >> 1)) + unit) * (uint32_t)(*Ap).slotBins + (uint32_t)b) * kSlot4;
      s0 = S[0];
      s1 = S[1];
      s2 = S[2];
      sm = S[3];
      const uint4 info = reinterpret_cast<const uint4 *>(S)[4];
      edge = r == __uint_as_float(info.w);  // the cell's own bin edge (+inf: none)
      // this sub-cell's mask and first admitted candidate; the slot's copy is that candidate when
      // its list position is the unit's first (j_U), otherwise it is gathered from the list
      const uint32_t m8 = (info.z >> (8 * slot_sub(sub, subs))) & 0xFFu;
      const uint32_t j = m8 ? (uint32_t)__builtin_ctz(m8) : (uint32_t)kMaskCand;
      c = (uint32_t)__popc(m8) + (info.x & 0xFFFFFFu);
      slotCopy = j == (info.x >> 24);
      fe = info.y + j;
      lds_st16(&W.pt[lane], make_float4(px, py, pz, r));
      lds_st16(&W.lst[lane], make_uint4(info.y, m8, 0u, 0xFFFFFFFFu));
      fr = r;
    } else if (want) {
      const float r = sqrtf(dot3(px, py, pz, px, py, pz));  // toSpherical(pos).x
      cell = cubemap_cell_fast(px, py, pz, (*Ap).G, sub);
      const uint4 *Hc = (*Ap).binHdr + (size_t)cell * (kBinHdrWords / 4);
      H0 = Hc[0];
      H1 = Hc[1];
      M = reinterpret_cast<const uint32_t *>(Hc)[8 + sub];
      const int b = bin_of(r, __uint_as_float(H0.x), __uint_as_float(H0.y), __uint_as_float(H0.z));
      const uint32_t m1 = b > 0 ? ~0u : 0u, m2 = b > 1 ? ~0u : 0u, m3 = b > 2 ? ~0u : 0u;
      const uint32_t beg = (m1 & H1.x) + (m2 & (H1.y - H1.x)) + (m3 & (H1.z - H1.y));
      const uint32_t end = H1.x + (m1 & (H1.y - H1.x)) + (m2 & (H1.z - H1.y)) + (m3 & (H1.w - H1.z));
      // r exactly on the bin's upper edge: records starting at that edge sit in the next
      // bin, whose list is scanned in a second pass for a lower record (locate_hdr)
      const float eb = __uint_as_float(H0.x ^ (m1 & (H0.x ^ H0.y)) ^ (m2 & (H0.y ^ H0.z)));
      edge = b < kMaxEdges && r == eb;
      const uint32_t n = end - beg;
      const uint32_t m8 = (M >> (8 * b)) & 0xFFu & (n < 8u ? (1u << n) - 1u : 0xFFu);
      c = (uint32_t)__popc(m8) + (n > (uint32_t)kMaskCand ? n - (uint32_t)kMaskCand : 0u);
      if constexpr (kHoleSkip) {
        // the sample's quad's radial range (header words kBoundWord..): outside it no listed
        // record passes the radial test (ICONGrid.h:184), so the scan would test every candidate
        // and find none -- a void of the volume (convert_icon's land columns), decided from the
        // header line alone
        const uint2 bd = reinterpret_cast<const uint2 *>((*Ap).binHdr + (size_t)cell * (kBinHdrWords / 4))
            [kBoundWord / 2 + quad_of(sub)];
        if (r > __uint_as_float(bd.x) || r < __uint_as_float(bd.y)) {
          c = 0u;
          edge = false;
        }
      }
      lds_st16(&W.pt[lane], make_float4(px, py, pz, r));
      lds_st16(&W.lst[lane], make_uint4(H0.w + beg, m8, 0u, 0xFFFFFFFFu));
      fe = H0.w + beg + (m8 ? (uint32_t)__builtin_ctz(m8) : (uint32_t)kMaskCand);
      fr = r;
    }
    IRT_ROUND_PROBE(9, false)
    for (int pass = 0;; ++pass) {
      // every lane: its list's first candidate
      uint32_t rem = 0u;
      if (c > 0u) {  // (from registers: no LDS round trip before the gather)
        Found f;
        bool ok;
        if (kSlot && pass == 0) {  // the slot's copy
          f = {__float_as_uint(sm.z), record_path(__float_as_uint(sm.w), sm.x, sm.y, fr)};
          ok = entry_passes(s0, s1, s2, sm, px, py, pz, fr);
        } else {
          ok = pass_entry((*Ap).fat + (size_t)fe * kFatStride4, px, py, pz, fr, f);
        }
        if (kSlot && pass == 0 && !slotCopy) {
          // the unit's first candidate is not one this sub-cell admits (a slot unit of several
          // sub-cells): it cannot hold the sample, and the sample's own candidates, its first
          // included, go to the dealt-out step -- no gather of its own on the round's chain
          rem = c;
        } else if (f.rec < flim) {  // scan_fat stops, uncounted, at the first record >= the limit
          ++specCand;
          if (ok) {
            hit = true;
            frm[lane] = make_uint2(f.rec, f.path);
          } else {
            rem = c - 1u;
            W.lst[lane].z = 1u;
          }
        }
      }
      tmark(3);  // header, first candidate
      IRT_ROUND_PROBE(10, false)
      bool need = rem > 0u;
      for (uint64_t nm = __ballot(need); nm != 0ull; nm = __ballot(need)) {
        // deal the owners' untested candidates out to the lanes: exclusive prefix of rem
        const uint32_t incl = wave_incl_sum(need ? rem : 0u);
        const uint32_t total = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
        const uint32_t start = incl - (need ? rem : 0u);
        const bool owns = need && start < 64u;
        own[lane] = 0xFFFFFFFFu;
        __builtin_amdgcn_wave_barrier();
        if (owns) own[start] = (uint32_t)lane;
        __builtin_amdgcn_wave_barrier();
        const uint64_t sm = __ballot(own[lane] != 0xFFFFFFFFu);  // bit s: an owner's tasks start at s
        // lane t: task t - s0 of the owner whose tasks start at the highest s0 <= t
        const uint32_t t = (uint32_t)lane;
        const bool task = t < total;
        const uint32_t s0 = task ? 63u - (uint32_t)__builtin_clzll(sm & (~0ull >> (63u - t))) : 0u;
        const uint32_t o = own[s0];
        bool tp = false, tl = false;
        Found g;
        if (task) {
          const float4 po = lds_ld16(&W.pt[o]);
          const uint4 d = lds_ld16(&W.lst[o]);
          tp = pass_entry((*Ap).fat + (size_t)(d.x + list_entry(d.y, d.z + (t - s0))) * kFatStride4, po.x, po.y,
                          po.z, po.w, g);
          tl = g.rec >= d.w;  // past the limit: the serial scan stops there
          tp = tp && !tl;
        }
        const uint64_t pm = __ballot(tp), lm = __ballot(tl);
        // the lowest event of each owner's tasks: a passing record (it hands it over) or the limit
        const uint64_t below = t ? (~0ull >> (64u - t)) : 0ull;  // tasks < t
        if (tp && ((pm | lm) & below & (~0ull << s0)) == 0ull) frm[o] = make_uint2(g.rec, g.path);
        __builtin_amdgcn_wave_barrier();
        if (owns) {
          const uint32_t k = min(rem, 64u - start);  // this owner's tasks in this batch
          const uint64_t ev = (pm | lm) & ((k >= 64u ? ~0ull : ((1ull << k) - 1ull)) << start);
          if (ev) {
            const uint32_t e = (uint32_t)__builtin_ctzll(ev) - start;
            const bool ps = (pm >> (start + e)) & 1ull;
            specCand += e + (ps ? 1u : 0u);
            hit = hit || ps;
            need = false;
          } else {
            specCand += k;
            rem -= k;
            W.lst[lane].z += k;
            need = rem > 0u;
          }
        }
        __builtin_amdgcn_wave_barrier();
      }
      tmark(4);  // the dealt-out candidates
      IRT_ROUND_PROBE(11, false)
      // the second pass: bin-edge samples, the next bin's list below the record found
      if (pass == 1 || __ballot(edge) == 0ull) break;
      c = 0u;
      if (edge) {
        const float4 p = lds_ld16(&W.pt[lane]);
        uint32_t sub;
        const uint32_t cell = cubemap_cell_fast(p.x, p.y, p.z, (*Ap).G, sub);
        const uint4 *Hc = (*Ap).binHdr + (size_t)cell * (kBinHdrWords / 4);
        const uint4 H0 = Hc[0], H1 = Hc[1];
        const uint32_t M = reinterpret_cast<const uint32_t *>(Hc)[8 + sub];
        const int b = bin_of(p.w, __uint_as_float(H0.x), __uint_as_float(H0.y), __uint_as_float(H0.z)) + 1;
        const uint32_t m1 = b > 0 ? ~0u : 0u, m2 = b > 1 ? ~0u : 0u, m3 = b > 2 ? ~0u : 0u;
        const uint32_t beg = (m1 & H1.x) + (m2 & (H1.y - H1.x)) + (m3 & (H1.z - H1.y));
        const uint32_t end = H1.x + (m1 & (H1.y - H1.x)) + (m2 & (H1.z - H1.y)) + (m3 & (H1.w - H1.z));
        const uint32_t n = end - beg;
        const uint32_t m8 = (M >> (8 * b)) & 0xFFu & (n < 8u ? (1u << n) - 1u : 0xFFu);
        c = (uint32_t)__popc(m8) + (n > (uint32_t)kMaskCand ? n - (uint32_t)kMaskCand : 0u);
        flim = hit ? frm[lane].x : 0xFFFFFFFFu;
        lds_st16(&W.lst[lane], make_uint4(H0.w + beg, m8, 0u, flim));
        fe = H0.w + beg + (m8 ? (uint32_t)__builtin_ctz(m8) : (uint32_t)kMaskCand);
      }
    }
    if (!want) return false;
    const float r = W.pt[lane].w;
    Found f = {0xFFFFFFFFu, 0u};
    if (hit) {
      const uint2 rm = frm[lane];
      f = {rm.x, rm.y};
    }
    if ((*Ap).numSph) {
      const uint32_t h = sph_hash(r);
      if ((s_sph[h >> 5] >> (h & 31)) & 1u) {
        float v2;
        uint32_t rec2;
        if (sphere_at(r, v2, rec2) && (!hit || rec2 < f.rec)) {
          value = v2;
          return true;
        }
      }
    }
    if (hit) value = record_value(f, r);
    return hit;
  }

  // postClassify's alpha only (the acceptance test needs nothing else); the colour comes
  // from post_classify on acceptance
  __device__ __forceinline__ float classify_alpha(float v) {
    const RenderArgs &LA = fresh_args();  // read where used
    v = div_uniform(v - LA.tfLo, LA.invTf, LA.tfHi - LA.tfLo);  // (v - tfLo) / (tfHi - tfLo), as the division rounds it
    const int size = opaque_u(LA.lutSize);
    const int idx = f2i_x86(v * (float)size);
    const float frac = (v * (float)size) - (float)idx;
    const int i1 = idx < 0 ? 0 : (idx > size - 1 ? size - 1 : idx);
    const int idx2 = (int)((uint32_t)idx + 1u);
    const int i2 = idx2 < 0 ? 0 : (idx2 > size - 1 ? size - 1 : idx2);
    const float a = LA.lut[i1].w, b = LA.lut[i2].w;
    return a * frac + b * (1.f - frac) * LA.opacityScale;
  }

  // postClassify (deviceCode.cu:127-135): weights reversed, opacityScale on 2nd term only
  __device__ __forceinline__ float4 post_classify(float v) {
    const RenderArgs &LA = fresh_args();  // read where used
    v = div_uniform(v - LA.tfLo, LA.invTf, LA.tfHi - LA.tfLo);  // (v - tfLo) / (tfHi - tfLo), as the division rounds it
    const int size = opaque_u(LA.lutSize);
    const int idx = f2i_x86(v * (float)size);
    const float frac = (v * (float)size) - (float)idx;
    const int i1 = idx < 0 ? 0 : (idx > size - 1 ? size - 1 : idx);
    const int idx2 = (int)((uint32_t)idx + 1u);
    const int i2 = idx2 < 0 ? 0 : (idx2 > size - 1 ? size - 1 : idx2);
    const float4 a = LA.lut[i1], b = LA.lut[i2];
    const float om = 1.f - frac;
    float4 o;
    o.x = a.x * frac + b.x * om * 1.f;
    o.y = a.y * frac + b.y * om * 1.f;
    o.z = a.z * frac + b.z * om * 1.f;
    o.w = a.w * frac + b.w * om * LA.opacityScale;
    return o;
  }

  // woodcockTracking (deviceCode.cu:149-186) over [tmin, tmax].  `counted` is false in
  // zero-length sdda leaves, whose sampleVolume calls the statistics leave out.
  __device__ __forceinline__ float woodcock(float dx, float dy, float dz, float tmin, float tmax,
                                            uint32_t &st, float majorant, float4 &sampleOut,
                                            bool counted) {
    float t = tmin;
    if (majorant <= 0.f) return fminf(t, tmax);
    const float q = majorant / (*Ap).unitDistance;  // the same value every iteration (165)
    while (true) {
      if constexpr ((OPT & OPT_STATS) != 0) ++cnt.steps;
      st = lcg_next(st);
      t -= (woodcock_log(st, s_logf) / q);
      if (t > tmax) break;
      const float3 O = cam_org((*Ap), frame);
      const float px = O.x + dx * t, py = O.y + dy * t, pz = O.z + dz * t;
      float value = 0.f;
      if (counted) count(2);
      if (!locate(px, py, pz, value)) continue;
      if (counted) count(3);
      const float sw = classify_alpha(value);  // postClassify(value).w
      st = lcg_next(st);
      const float u = lcg_float(st);
      if (sw >= u * majorant) {
        sampleOut = post_classify(value);
        break;
      }
    }
    return fminf(t, tmax);
  }

  // woodcockTracking (deviceCode.cu:149-186) for every lane of the wave with `req` set,
  // evaluated together.  A ray's sample positions depend on nothing but its RNG: sample k
  // (k = 0, 1, ...) of a ray whose earlier samples were all located and rejected lies at
  // t - d_0 - ... - d_k with d_j from the state 2j+1 draws ahead, and is accepted against
  // the state 2k+2 draws ahead.  So each round the wave's R undecided rays get G = 64/R
  // (a power of two) lanes each; lane k of a group takes sample k of its ray -- independent
  // gathers in parallel instead of a chain -- and the ray's first event among its G samples
  // (past tmax / not located / accepted) decides it exactly as the serial loop would; the
  // samples after the event are discarded.  A not-located sample consumes only its step
  // draw, so the ray resumes from there next round -- in miss mode: its samples are then
  // placed as if none were located (sample k from the state k+1 draws ahead) until one is,
  // which switches back (samples outside every cell come in runs: grid-accel cells and
  // wedge gaps).  Statistics count only the samples
  // the reference takes.  Returns in t the woodcockTracking return value.
  __device__ __forceinline__ void woodcock_wave(bool req, float dx, float dy, float dz, float &t,
                                                float tmax, uint32_t &st, float majorant,
                                                bool counted, float4 &sampleOut, bool &miss,
                                                CoopWave &W, ScanWave *SW, const uint2 *jmp) {
    Ap = &A;  // the arguments this call's methods read
    const int lane = (int)__lane_id();
    const uint64_t below = (1ull << lane) - 1ull;
    const float q = majorant / (*Ap).unitDistance;
    bool active = req && !(majorant <= 0.f);  // majorant <= 0: return at once (161-162)
    // speculation ramps up: a ray gets at most 2^lgCap lanes this round, and lgCap grows
    // each round it stays undecided.  Most chains end within a few samples (default TF:
    // 3 draws), and the lines of samples past the event are wasted gathers; long chains
    // (sparse TFs) reach whole-wave groups after six rounds.  The miss-mode kernels (wedge
    // samplers, grid accel) keep whole-wave groups from the start: their misses come in
    // runs that wide groups cross in one round (2 % faster there, profiles/r02e_coop_cap).
    int lgCap = kWideStart ? 6 : (*Ap).coopMaxLg;
    tmark(6);  // between woodcockFunc calls (sdda leaves, ranges)
    for (;; lgCap = min(lgCap + (*Ap).coopRamp, 6)) {
      const uint64_t am = __ballot(active);
      if (am == 0ull) break;
      if constexpr ((OPT & OPT_STATS) != 0) ++cnt.rounds;
      const int R = __popcll(am);
      const int lg = min(lgCap, R > 32 ? 0 : R > 16 ? 1 : R > 8 ? 2 : R > 4 ? 3 : R > 2 ? 4 : R > 1 ? 5 : 6);
      const int G = 1 << lg;
      // solo round (G = 1): every ray on its own lane, nothing exchanged
      const bool solo = lg == 0;
      const int rank = __popcll(am & below);
      int grp, k;
      bool used, cntd, mm;
      float4 rq, ry;
      if (solo) {
        grp = lane;
        k = 0;
        used = active;
        cntd = counted;
        mm = kMiss && miss;
        rq = make_float4(t, tmax, q, majorant);
        ry = make_float4(dx, dy, dz, __uint_as_float(st));
      } else {
        if (active) {
          lds_st16(&W.req[rank], make_float4(t, tmax, q, majorant));
          lds_st16(&W.ray[rank], make_float4(dx, dy, dz, __uint_as_float(st)));
          W.cnt[rank] = (counted ? 1u : 0u) | (miss ? 2u : 0u);
        }
        __builtin_amdgcn_wave_barrier();
        grp = lane >> lg;
        k = lane & (G - 1);
        used = grp < R;
        const int g = used ? grp : 0;
        rq = lds_ld16(&W.req[g]);
        ry = lds_ld16(&W.ray[g]);
        const uint32_t cf = W.cnt[g];
        cntd = cf & 1u;
        mm = kMiss && (cf & 2u);
      }
      const uint32_t s0 = __float_as_uint(ry.w);
      // sample k's step draw: 2k+1 draws ahead if every earlier sample is located (and
      // rejected), k+1 if none is (miss mode)
      const int jk = mm ? k + 1 : 2 * k + 1;
      uint32_t sk;
      if (solo) {
        sk = lcg_next(s0);
      } else {
        const uint2 j = lds_ld8(&jmp[jk]);  // {mul, add}: one 8-byte LDS read
        sk = j.x * s0 + j.y;
      }
      const float dk = woodcock_log(sk, s_logf) / rq.z;
      float tk;
      constexpr bool dppScan = (OPT & OPT_DPPSCAN) != 0;
      if (solo) {
        tk = rq.x - dk;
      } else if (dppScan && (lg == 1 || lg == 2 || lg == 4 || lg == 6)) {
        tk = lg == 1 ? dpp_prefix<2>(rq.x, dk, k)
                     : lg == 2 ? dpp_prefix<4>(rq.x, dk, k) : lg == 4 ? dpp_prefix<16>(rq.x, dk, k) : dpp_prefix<64>(rq.x, dk, k);
      } else {
        W.step[lane] = dk;
        __builtin_amdgcn_wave_barrier();
        const float *dg = &W.step[grp << lg];
        switch (lg) {
          case 1: tk = coop_prefix<2>(rq.x, dg, k); break;
          case 2: tk = coop_prefix<4>(rq.x, dg, k); break;
          case 3: tk = coop_prefix<8>(rq.x, dg, k); break;
          case 4: tk = coop_prefix<16>(rq.x, dg, k); break;
          case 5: tk = coop_prefix<32>(rq.x, dg, k); break;
          default: tk = coop_prefix<64>(rq.x, dg, k); break;
        }
      }
      bool past = used && tk > rq.y;
      if constexpr (kVoidRun) {
        // A solo lane in miss mode walks the void its ray is in on its own: while its sample lies
        // outside the radial range of every record that can reach the sample's quad (the cell
        // header's bounds, the quad-bound test of locate_wave), the sample is outside every cell
        // -- sampleVolume finds nothing and woodcockTracking takes its next step after one draw
        // (deviceCode.cu:165-173) -- so the lane takes that step here, with no candidate test (the
        // header's bound word, an L1 hit while the walk stays in one cell).  The round then scans the first sample
        // that may be located.  convert_icon's voids (over and under every land column) are
        // crossed in one round instead of one round per sample.
        constexpr bool kVoidLoc = (OPT & OPT_VOIDLOC) != 0;
        if (solo && used && !past && (mm || kVoidLoc)) {
          const float3 O = cam_org((*Ap), frame);
#pragma nounroll
          for (int it = 0; it < kVoidRunMax; ++it) {
            const float px = O.x + ry.x * tk, py = O.y + ry.y * tk, pz = O.z + ry.z * tk;
            const float r = sqrtf(dot3(px, py, pz, px, py, pz));  // toSpherical(pos).x
            uint32_t sub;
            const uint32_t cell = cubemap_cell_fast(px, py, pz, (*Ap).G, sub);
            // (the same header line as the last sample's while the walk stays in one cell: an L1 hit)
            const uint2 bd = reinterpret_cast<const uint2 *>((*Ap).binHdr + (size_t)cell * (kBinHdrWords / 4))
                [kBoundWord / 2 + quad_of(sub)];
            if (!(r > __uint_as_float(bd.x) || r < __uint_as_float(bd.y))) break;  // may be located: the round's scan decides
            if ((*Ap).numSph) {  // a zero-thickness record at exactly r is not in the lists
              const uint32_t h = sph_hash(r);
              if ((s_sph[h >> 5] >> (h & 31)) & 1u) break;
            }
            // outside every cell: the sample is taken (a sampleVolume call), one draw.  In
            // located mode (OPT_VOIDLOC) this miss breaks the round's assumption: a solo lane's
            // sample 0 takes its step draw first in either mode, so the ray switches to miss
            // mode here and walks on
            if (kVoidLoc && !mm) {
              mm = true;
              miss = true;
            }
            if (cntd) ++nLocate;
            if constexpr ((OPT & OPT_STATS) != 0) ++cnt.steps;
            rq.x = tk;
            sk = lcg_next(sk);
            tk = rq.x - woodcock_log(sk, s_logf) / rq.z;
            if (tk > rq.y) {
              past = true;
              break;
            }
          }
        }
      }
      IRT_ROUND_PROBE(8)
      bool found = false, acc = false;
      float value = 0.f;
      tmark(2);  // round start: exchange, jumps, logf, prefix
#ifdef IRT_PROBE_BUILD
      // measurement only (31): 100 extra VALU instructions per Woodcock round
      if ((*Ap).probeExit == 31) {
#pragma nounroll
        for (int k = 0; k < 25; ++k) asm volatile("v_nop\n v_nop\n v_nop\n v_nop" ::: "memory");
      }
#endif
      if constexpr (kWaveScan) {
        const float3 O = cam_org((*Ap), frame);
        found = locate_wave(used && !past, O.x + ry.x * tk, O.y + ry.y * tk, O.z + ry.z * tk,
                            value, W, *SW);
      } else if (used && !past) {
        const float3 O = cam_org((*Ap), frame);
        found = locate(O.x + ry.x * tk, O.y + ry.y * tk, O.z + ry.z * tk, value);
      }
      tmark(5);  // locate's tail: sphere, getValue
#ifdef IRT_PROBE_BUILD
      if ((*Ap).probeExit >= 9 && (*Ap).probeExit <= 12) return;
#endif
      if (found) {
        const float sw = classify_alpha(value);  // postClassify(value).w
        acc = sw >= lcg_float(lcg_next(sk)) * rq.w;
      }
      // the first sample that breaks the round's assumption, or ends the ray's leaf
      const bool ev = used && (past || acc || (mm ? found : !found));
      // the lane's group: its first event, G if none; the samples up to it are taken
      int first;
      uint64_t em = 0ull;
      if (solo) {
        first = ev ? 0 : 1;
      } else {
        em = __ballot(ev);
        const uint64_t gm = lg == 6 ? ~0ull : (((1ull << G) - 1ull) << (grp << lg));
        first = (em & gm) ? (int)__builtin_ctzll(em & gm) - (grp << lg) : G;
      }
      if (used && k <= first) {
        if (cntd) {
          nLocate += past ? 0u : 1u;
          nFound += found ? 1u : 0u;
        }
        nCand += specCand;
      }
      if constexpr ((OPT & OPT_STATS) != 0) {
        const bool loc = used && !past;
        uint32_t m = loc ? specCand : 0u;
        for (int off = 32; off > 0; off >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, off, 64));
        cnt.hops += m;
        cnt.locRounds += __ballot(loc) ? 1u : 0u;
        if (loc) ++cnt.candHist[specCand < 3u ? specCand : 3u];
      }
      specCand = 0u;
      // the rays' owners take their group's outcome
      int of;
      float tsrc, vsrc;
      bool pastS, accS, foundS;
      if (solo) {
        of = first;
        tsrc = tk;
        vsrc = value;
        pastS = past;
        accS = acc;
        foundS = found;
      } else {
        const uint64_t pastM = __ballot(past), accM = __ballot(acc), foundM = kMiss ? __ballot(found) : 0ull;
        const int ob = active ? rank << lg : 0;  // < 64 for an owner
        const uint64_t om = lg == 6 ? ~0ull : (((1ull << G) - 1ull) << ob);
        of = (active && (em & om)) ? (int)__builtin_ctzll(em & om) - ob : G;
        const int src = active ? ob + (of < G ? of : G - 1) : lane;
        tsrc = __shfl(tk, src, 64);
        vsrc = __shfl(value, src, 64);
        pastS = (pastM >> src) & 1ull;
        accS = (accM >> src) & 1ull;
        foundS = (foundM >> src) & 1ull;
      }
      if (active) {
        if constexpr ((OPT & OPT_STATS) != 0) cnt.steps += of < G ? (uint32_t)of + 1u : (uint32_t)G;
        t = tsrc;
        // draws taken: two per located sample, one per miss (and the one past tmax)
        const int n = (kMiss && miss) ? (of == G ? G : (foundS ? of + 2 : of + 1))
                           : (of == G ? 2 * G : (accS ? 2 * of + 2 : 2 * of + 1));
        if (solo) {
          st = n == 1 ? sk : lcg_next(sk);  // the draws this round made
        } else {
          const uint2 j = lds_ld8(&jmp[n]);
          st = j.x * st + j.y;
        }
        if (of < G && (pastS || accS)) {
          active = false;
          if (accS) sampleOut = post_classify(vsrc);
        } else if (kMiss && of < G) {
          miss = !miss;  // the assumption broke: a miss, or (miss mode) a located sample
        }
      }
      IRT_ROUND_PROBE(13)
    }
    if (req) t = fminf(t, tmax);
    tmark(7);  // the rounds' classify, LUT, ballots, outcomes
  }
};

}  // namespace irt
