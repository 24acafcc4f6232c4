// irt_debug.cpp -- host-only inspection entry points (include/icon_rt_hip_debug.h).

#include <math.h>
#include <vector>
#include <string.h>

#include "icon_rt_hip_debug.h"
#include "irt_internal.h"

using namespace irt;

struct irt_debug_scene {
  HostScene s;
  std::vector<irt_icon_cell> cells;  // kept for the CUBQL_MODE wedge queries
  WedgeScene w;
};

struct irt_debug_void_cache {
  VoidCache c;
};

extern "C" {

float irt_debug_asinf(float x) { return glibc_asinf(x); }
float irt_debug_atan2f(float y, float x) { return glibc_atan2f(y, x); }
int irt_debug_f2i(float x) { return f2i_x86(x); }
void irt_debug_lcg_jump(uint32_t n, uint32_t *mul, uint32_t *add) { lcg_jump(n, *mul, *add); }

float irt_debug_logf_entry(uint32_t k) { return logf_table()[k & 0x00FFFFFFu]; }

void irt_debug_srgb_thresholds(float *out256) { srgb_thresholds(out256); }

void irt_debug_host_woodcock_log(float *out) {
  for (uint32_t k = 0; k < (1u << 24); ++k) out[k] = logf(1.f - (float)k / (float)0x01000000);
}

uint32_t irt_debug_logf_mismatches(void) {
  // glibc_logf_unit (irt_common.h) vs the host glibc logf over the Woodcock domain
  uint32_t bad = 0;
  for (uint32_t k = 0; k < (1u << 24); ++k) {
    const float x = 1.f - (float)k / (float)0x01000000;
    if (f2u(glibc_logf_unit(x, kLogfTab)) != f2u(logf(x))) ++bad;
  }
  return bad;
}

int irt_debug_scene_build(const irt_icon_cell *cells, size_t n, irt_debug_scene **out) {
  if (!out || (n && !cells)) {
    set_error("irt_debug_scene_build: null argument");
    return IRT_E_INVALID;
  }
  irt_debug_scene *d = new irt_debug_scene();
  int rc = build_scene(cells, n, d->s);
  if (rc) {
    delete d;
    return rc;
  }
  *out = d;
  return IRT_OK;
}

int irt_debug_scene_info(const irt_debug_scene *s, irt_volume_info *info) {
  if (!s || !info) return IRT_E_INVALID;
  *info = s->s.info;
  return IRT_OK;
}

int irt_debug_scene_locate(const irt_debug_scene *s, irt_vec3f p, float *value,
                           uint32_t *record) {
  if (!s || !value) return IRT_E_INVALID;
  float v = 0.f;
  uint32_t r = 0;
  int hit = locate_host(s->s, p.x, p.y, p.z, v, &r);
  if (hit) {
    *value = v;
    if (record) *record = r;
  }
  return hit;
}

int irt_debug_scene_locate_binned(const irt_debug_scene *s, irt_vec3f p, float *value,
                                  uint32_t *record, uint32_t *tested) {
  if (!s || !value) return IRT_E_INVALID;
  float v = 0.f;
  uint32_t r = 0;
  int hit = locate_bins_host(s->s, p.x, p.y, p.z, v, &r, tested);
  if (hit) {
    *value = v;
    if (record) *record = r;
  }
  return hit;
}

int irt_debug_scene_values(const irt_debug_scene *s, uint32_t rec, float r, float *out2) {
  if (!s || !out2 || rec >= s->s.n) return IRT_E_INVALID;
  const float *hv = &s->s.hv[(size_t)rec * kHV];
  int32_t nl;
  memcpy(&nl, hv + 63, 4);
  out2[0] = hv[32 + find_height(hv, nl, r)];
  // the kernel's path (irt_render.hip record_value): the quantised coarse keys pick one
  // 64-B block for sorted heights (exact keys near a key), else the literal binary search
  out2[1] = record_value_host(s->s, rec,
                              record_path(s->s.meta[rec], s->s.rng[2 * (size_t)rec],
                                          s->s.rng[2 * (size_t)rec + 1], r), r);
  return IRT_OK;
}

int irt_debug_scene_candidates(const irt_debug_scene *s, irt_vec3f p, uint32_t *records,
                               int capacity) {
  if (!s || s->s.G == 0) return 0;
  const uint32_t cell = cubemap_cell(p.x, p.y, p.z, s->s.G);
  const uint32_t b = s->s.offsets[cell], e = s->s.offsets[cell + 1];
  int k = 0;
  for (uint32_t i = b; i < e; ++i, ++k)
    if (records && k < capacity) records[k] = s->s.entryRec[i];
  return k;
}

int irt_debug_scene_planes(const irt_debug_scene *s, uint32_t record, float *out12) {
  if (!s || !out12 || record >= s->s.n) return IRT_E_INVALID;
  memcpy(out12, &s->s.planes[12 * (size_t)record], 12 * sizeof(float));
  return IRT_OK;
}

void irt_debug_scene_free(irt_debug_scene *s) { delete s; }

int irt_debug_scene_array(const irt_debug_scene *s, int which, void *dst, size_t capacity,
                          size_t *bytes) {
  if (!s || !bytes) {
    set_error("irt_debug_scene_array: null argument");
    return IRT_E_INVALID;
  }
  const HostScene &S = s->s;
  std::vector<uint32_t> rec;
  const void *src = nullptr;
  size_t n = 0;
  switch (which) {
    case IRT_DEBUG_ARRAY_BIN_HDR: src = S.binHdr.data(); n = S.binHdr.size() * 4; break;
    case IRT_DEBUG_ARRAY_FAT: src = S.fat.data(); n = S.fat.size() * 4; break;
    case IRT_DEBUG_ARRAY_BLOCKS: src = S.blocks.data(); n = S.blocks.size() * 4; break;
    case IRT_DEBUG_ARRAY_SPH_R: src = S.sphR.data(); n = S.sphR.size() * 4; break;
    case IRT_DEBUG_ARRAY_SPH_OFF: src = S.sphOff.data(); n = S.sphOff.size() * 4; break;
    case IRT_DEBUG_ARRAY_SPH_REC:
      for (uint32_t r : S.sphRec) {
        int32_t nl;
        memcpy(&nl, &S.hv[(size_t)r * kHV + 63], 4);
        rec.push_back(r);
        rec.push_back((uint32_t)nl);
      }
      src = rec.data();
      n = rec.size() * 4;
      break;
    case IRT_DEBUG_ARRAY_SPH_BITS: src = S.sphBits.data(); n = S.sphBits.size() * 4; break;
    default:
      set_error("irt_debug_scene_array: unknown array %d", which);
      return IRT_E_INVALID;
  }
  *bytes = n;
  if (dst && capacity >= n && n) memcpy(dst, src, n);
  return IRT_OK;
}

int irt_debug_scene_locate_wedge(irt_debug_scene *s, irt_vec3f p, float *value) {
  if (!s || !value) return IRT_E_INVALID;
  if (s->w.G == 0) {
    set_error("irt_debug_scene_locate_wedge: call irt_debug_scene_build_wedges first");
    return IRT_E_INVALID;
  }
  return wedge_locate_host(s->w, s->cells.data(), p.x, p.y, p.z, *value) ? 1 : 0;
}

int irt_debug_scene_build_wedges(irt_debug_scene *s, const irt_icon_cell *cells, size_t n) {
  if (!s || (n && !cells) || n != s->s.n) {
    set_error("irt_debug_scene_build_wedges: cells do not match the scene");
    return IRT_E_INVALID;
  }
  s->cells.assign(cells, cells + n);
  return build_wedges(cells, n, s->w);
}

int irt_debug_scene_locate_triangle(irt_debug_scene *s, irt_vec3f p, float *value,
                                    uint32_t *record) {
  if (!s || !value) return IRT_E_INVALID;
  if (s->w.G == 0) {
    set_error("irt_debug_scene_locate_triangle: call irt_debug_scene_build_wedges first");
    return IRT_E_INVALID;
  }
  return triangle_locate_host(s->w, s->cells.data(), p.x, p.y, p.z, *value, record) ? 1 : 0;
}

int irt_debug_intersect_wedge(const float *v24, irt_vec3f p, float *value) {
  WV4 V[6];
  memcpy(V, v24, sizeof(V));
  float v = 0.f;
  const bool hit = intersect_wedge(v, p.x, p.y, p.z, V);
  if (hit) *value = v;
  return hit ? 1 : 0;
}

int irt_debug_sched_order(const uint32_t *cost, int numBlocks, int tilesX, int tileStride, int policy,
                          int splitLg, float splitFactor, int numCU, int wavewg, size_t capacity,
                          uint32_t maxSplit, uint32_t *out, uint32_t *numSplit) {
  if (!cost || !out || !numSplit || numBlocks < 0 || numBlocks % 16 || (size_t)numBlocks > capacity ||
      splitLg < 0 || splitLg > 3 || maxSplit % 8) {
    set_error("irt_debug_sched_order: bad argument");
    return IRT_E_INVALID;
  }
  *numSplit = sched_order(cost, numBlocks, tilesX, tileStride, policy, splitLg, splitFactor, numCU,
                          wavewg != 0, capacity, maxSplit, out);
  return IRT_OK;
}

irt_debug_void_cache *irt_debug_void_cache_create(void) { return new irt_debug_void_cache(); }
void irt_debug_void_cache_free(irt_debug_void_cache *cache) { delete cache; }

int irt_debug_void_packets(irt_debug_void_cache *cache, const irt_launch_params *lp, const irt_volume_info *info,
                           int W, int H, int tileBegin, int tileStride, const int32_t *tileList, int listCount,
                           uint32_t *bits, size_t capacity, uint32_t *numVoid, long long *computations) {
  if (!lp || !info || !numVoid || W <= 0 || H <= 0 || tileBegin < 0 || tileStride <= 0 || listCount < 0) {
    set_error("irt_debug_void_packets: bad argument");
    return IRT_E_INVALID;
  }
  const int total = ((W + 63) / 64) * ((H + 63) / 64);
  const int numTiles = tileList ? listCount : tileBegin < total ? (total - tileBegin + tileStride - 1) / tileStride : 0;
  for (int k = 0; tileList && k < listCount; ++k)
    if (tileList[k] < 0 || tileList[k] >= total) {
      set_error("irt_debug_void_packets: tile id %d at %d outside [0, %d)", tileList[k], k, total);
      return IRT_E_INVALID;
    }
  if (void_words(numTiles) > capacity || (!bits && capacity)) {
    set_error("irt_debug_void_packets: %zu words needed", void_words(numTiles));
    return IRT_E_INVALID;
  }
  const VoidRequest q = void_request(*lp, *info, W, H, tileBegin, tileStride, numTiles, tileList);
  VoidCache local;
  VoidCache &vc = cache ? cache->c : local;
  vc.lookup(q);
  if (void_words(numTiles)) memcpy(bits, vc.bits.data(), void_words(numTiles) * sizeof(uint32_t));
  *numVoid = vc.count;
  if (computations) *computations = vc.generation;
  return IRT_OK;
}

int irt_debug_interior_packets(irt_debug_void_cache *cache, const irt_launch_params *lp, const irt_volume_info *info,
                               int W, int H, int tileBegin, int tileStride, const int32_t *tileList, int listCount,
                               uint32_t *bits, size_t capacity, uint32_t *numInterior, long long *computations) {
  if (!lp || !info || !numInterior || W <= 0 || H <= 0 || tileBegin < 0 || tileStride <= 0 || listCount < 0) {
    set_error("irt_debug_interior_packets: bad argument");
    return IRT_E_INVALID;
  }
  const int total = ((W + 63) / 64) * ((H + 63) / 64);
  const int numTiles = tileList ? listCount : tileBegin < total ? (total - tileBegin + tileStride - 1) / tileStride : 0;
  for (int k = 0; tileList && k < listCount; ++k)
    if (tileList[k] < 0 || tileList[k] >= total) {
      set_error("irt_debug_interior_packets: tile id %d at %d outside [0, %d)", tileList[k], k, total);
      return IRT_E_INVALID;
    }
  if (void_words(numTiles) > capacity || (!bits && capacity)) {
    set_error("irt_debug_interior_packets: %zu words needed", void_words(numTiles));
    return IRT_E_INVALID;
  }
  const VoidRequest q = void_request(*lp, *info, W, H, tileBegin, tileStride, numTiles, tileList);
  VoidCache local;
  VoidCache &vc = cache ? cache->c : local;
  vc.lookup(q);
  if (void_words(numTiles)) memcpy(bits, vc.interior.data(), void_words(numTiles) * sizeof(uint32_t));
  *numInterior = vc.interiorCount;
  if (computations) *computations = vc.generation;
  return IRT_OK;
}

int irt_debug_void_lists(irt_debug_void_cache *cache, const irt_launch_params *lp, const irt_volume_info *info,
                         int W, int H, int tileBegin, int tileStride, const int32_t *tileList, int listCount,
                         int numFrames, uint32_t *items, size_t capacity, uint32_t *numLive, uint32_t *voidPerRow,
                         uint32_t *numVoid) {
  if (!lp || !info || !numLive || !voidPerRow || !numVoid || W <= 0 || H <= 0 || tileBegin < 0 || tileStride <= 0 ||
      listCount < 0 || numFrames < 1) {
    set_error("irt_debug_void_lists: bad argument");
    return IRT_E_INVALID;
  }
  const int total = ((W + 63) / 64) * ((H + 63) / 64);
  const int numTiles = tileList ? listCount : tileBegin < total ? (total - tileBegin + tileStride - 1) / tileStride : 0;
  for (int k = 0; tileList && k < listCount; ++k)
    if (tileList[k] < 0 || tileList[k] >= total) {
      set_error("irt_debug_void_lists: tile id %d at %d outside [0, %d)", tileList[k], k, total);
      return IRT_E_INVALID;
    }
  const VoidRequest q = void_request(*lp, *info, W, H, tileBegin, tileStride, numTiles, tileList);
  VoidCache local;
  VoidCache &vc = cache ? cache->c : local;
  vc.lookup(q);
  const VoidLists &vl = vc.lists;
  *numLive = vl.live;
  *numVoid = vl.count;
  *voidPerRow = vl.count ? void_row(vl.count, numFrames) : 0u;
  if (!items) return IRT_OK;
  const size_t need = (size_t)vl.live + (size_t)numFrames * *voidPerRow;
  if (need > capacity) {
    set_error("irt_debug_void_lists: %zu words needed", need);
    return IRT_E_INVALID;
  }
  // the rows' void parts as k_render's workgroups read them: item y * voidPerRow + k, empty past the last
  std::copy(vl.items.begin(), vl.items.begin() + vl.live, items);
  for (size_t j = 0; j < (size_t)numFrames * *voidPerRow; ++j)
    items[vl.live + j] = j < vl.count ? vl.items[vl.live + j] : kVoidEmpty;
  return IRT_OK;
}

}  // extern "C"
