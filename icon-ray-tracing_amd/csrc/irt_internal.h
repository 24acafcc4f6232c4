// irt_internal.h -- C++ internals shared by the host build (host/*.cpp, g++) and the HIP
// runtime layer (csrc/*.hip, hipcc).  No HIP types here.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "icon_rt_hip.h"
#include "irt_common.h"

namespace irt {

void set_error(const char *fmt, ...) __attribute__((format(printf, 1, 2)));
void clear_error();


// The scene build's arrays (irt_build.h), restated on the host: the device build
// (irt_build.hip) produces the same bytes.
struct HostScene {
  size_t n = 0;
  irt_volume_info info{};
  std::vector<float> hv;          // n * kHV floats (see irt_common.h), for host checks
  std::vector<float> trig;        // n * 12: per corner {cosf lat, sinf lat, cosf lon, sinf lon}
  std::vector<float> planes;      // n * 12: the side planes of sample() (ICONGrid.h:197-199)
  std::vector<float> rng;         // n * 2: {height[0], height[numLayers]}
  std::vector<uint32_t> meta;     // n: record_meta (numLayers, coarse flag, quantised keys)
  std::vector<float> blocks;      // n * kBlk4 * 4: height/value blocks
  int G = 0;                      // cube-map cells per face edge
  std::vector<uint32_t> offsets;  // 6*G*G + 1 CSR offsets
  std::vector<uint32_t> entryRec; // candidate lists (each sorted by record index) ...
  std::vector<uint32_t> entrySub; // ... and each entry's sub-cell mask
  // the product locator (irt_build.h)
  std::vector<uint32_t> binHdr;   // 6*G*G * kBinHdrWords
  std::vector<float> fat;         // binEntries * kFatStride4 * 4
  size_t binEntries = 0;
  // zero-thickness records (spheres): distinct radii, CSR into record indices (ascending),
  // and a hash bitmap of the radii (irt_common.h sph_hash) the kernel keeps in LDS
  std::vector<float> sphR;
  std::vector<uint32_t> sphOff, sphRec, sphBits;
};

// Build the binned locator (binHdr, fat) from the CSR lists; build_scene calls it.
int build_bins(HostScene &S, int threads);
// Cube-map resolution for a scene with numRuns columns (IRT_LOCATOR_SCALE / _G override).
int locator_resolution(size_t numRuns);
// Point location over the binned locator, as the kernel does it (host restatement).
// getValue of record rec at radius r along its record_path (the kernel's record_value)
float record_value_host(const HostScene &s, uint32_t rec, uint32_t path, float r);
int locate_bins_host(const HostScene &s, float px, float py, float pz, float &value,
                     uint32_t *record, uint32_t *tested);

// Validate, compute volume facts, per-record planes/heights, and the locator.
int build_scene(const irt_icon_cell *cells, size_t n, HostScene &out, int threads = 0);


// Volume facts only (hostCode.cu:792-808, 838-840).
void compute_volume_info(const irt_icon_cell *cells, size_t n, irt_volume_info &info);
// ... as a fold over records in order, for chunked input: per record the corner trig
// (glibc cosf/sinf) and getBounds (ICONGrid.h:78-115), then volume_acc_add in record order.
struct VolumeAcc {
  float vlo[3], vhi[3], slo[3], shi[3], dlo, dhi;
  size_t n;
};
void corner_trig(const irt_icon_cell &c, float *t12);
void cell_bounds(const irt_icon_cell &c, const float *t12, float lo[3], float hi[3]);
void volume_acc_init(VolumeAcc &a);
void volume_acc_add(VolumeAcc &a, const irt_icon_cell &c, const float blo[3], const float bhi[3]);
void volume_acc_merge(VolumeAcc &a, const VolumeAcc &b);  // a's records, then b's
void volume_acc_finish(const VolumeAcc &a, irt_volume_info &info);

// glibc logf(1 - k/2^24) for k in [0, 2^24): the only arguments woodcockTracking's
// `logf(1.f - rnd())` (deviceCode.cu:165) can ever see.
const std::vector<float> &logf_table();

// th[b] (b = 1..255) = smallest float x with make_8bit(linear_to_srgb(x)) >= b, under the
// host glibc powf (dvr_course-common-both.h:30-35, 89-92); th[0] = smallest float x >= 1 whose
// byte is 0 again: int(s * 256) overflows there (cvttss2si: INT_MIN), +inf included.
void srgb_thresholds(float th[256]);

// Host restatement of the scalar reference functions the kernels rely on, for checks.
int sample_host(const HostScene &s, uint32_t rec, float px, float py, float pz, float &value);
// Reference-semantics point location over the locator (host side, for CPU tests).
int locate_host(const HostScene &s, float px, float py, float pz, float &value,
                uint32_t *record);

// The unstructured-element locator of CUBQL_MODE (Params.h:31; deviceCode.cu:90-115) and
// TRIANGLE_MODE (61-76), the replacement of buildCuBQLAccel's cuBQL BVH and
// buildTriangleAccel's OptiX BVH (hostCode.cu:557-649, 440-484): per record the glibc corner
// trig and the union box of its wedges' primBounds and its bottom triangle, and a gnomonic
// cube map listing, per cell, every record whose box can hold a point of that direction
// (sorted by index).
struct WedgeScene {
  int G = 0;
  std::vector<float> trig;       // n * 12: per corner {cosf lat, sinf lat, cosf lon, sinf lon}
  std::vector<float> box;        // n * 8: lo.xyz, numLayers (int bits), hi.xyz, 0
  std::vector<uint32_t> offsets; // 6*G*G + 1
  std::vector<uint32_t> recs;    // record indices
};
int build_wedges(const irt_icon_cell *cells, size_t n, WedgeScene &W, int threads = 0);
// CUBQL_MODE sampleVolume over the wedge locator, as the kernel does it (host check).
bool wedge_locate_host(const WedgeScene &W, const irt_icon_cell *cells, float px, float py,
                       float pz, float &value);
// TRIANGLE_MODE sampleVolume over the same locator, as the kernel does it (host check).
bool triangle_locate_host(const WedgeScene &W, const irt_icon_cell *cells, float px, float py,
                          float pz, float &value, uint32_t *record);

int default_threads();

// irt_update_values*: records [first, first + n) lie inside a context of numCells records
// (first + n without wrapping)
inline bool update_range_ok(size_t first, size_t n, size_t numCells) {
  return first <= numCells && n <= numCells - first;
}

// Resampling (host/irt_latlon.cpp; csrc/irt_sample.hip): the most points of one call (2^30 one-wave
// workgroups: 32 rows of one grid, irt_sample.hip sample_grid), the lat/lon grid's trig rows {cosf, sinf} per
// latitude and per longitude from the host's glibc, and the grid calls' argument check
constexpr uint64_t kSampleMaxPoints = uint64_t(1) << 36;
void latlon_trig(const float *lat, int numLat, const float *lon, int numLon, float *latCS, float *lonCS);
int latlon_args(const char *what, const float *lat, int numLat, const float *lon, int numLon,
                const float *radius, int numLevels, size_t *total);

// Level surfaces (host/irt_level_order.cpp; csrc/irt_levels.hip): the check of the radii
// (numLevels in [1, IRT_MAX_LEVELS], every radius finite and positive), and the near order of the
// hit slots -- sorted[h] = radius[index[h]], descending, ties by ascending index
int levels_args(const char *what, const float *radius, int numLevels);
void levels_order(const float *radius, int numLevels, float *sorted, int32_t *index);

// Column products (host/irt_column.cpp; csrc/irt_column.hip): the check of the weights (NULL, or
// numLevels finite floats), and irt_render_column's check of its levels (numLevels >= 1, every
// radius finite and positive, then the weights).  The reduction itself is csrc/irt_column.h.
int column_weights(const char *what, const float *weight, int numLevels);
int column_levels_args(const char *what, const float *radius, const float *weight, int numLevels);

// Sections (host/irt_section.cpp; csrc/irt_section.hip): the columns' trig table, {cosf lat, sinf lat,
// cosf lon, sinf lon} per (lat, lon) pair from the host's glibc, and the check irt_section and
// irt_section_points share (negative counts, more than kSampleMaxPoints points, a NULL array with
// points to sample); *total = numColumns * numLevels
constexpr size_t kSectionTrigSplit = 1 << 14;  // columns from which section_trig uses default_threads()
void section_trig(const float *lat, const float *lon, int numColumns, float *tab);
int section_args(const char *what, const float *lat, const float *lon, int numColumns, const float *radius,
                 int numLevels, size_t *total);

// Field statistics (host/irt_histogram.cpp; csrc/irt_histogram.hip): the check irt_histogram and
// irt_histogram_cells share -- the bin and band counts, the value range, the weighting, the band edges.
// The definition itself is csrc/irt_histogram.h.
int hist_args(const char *what, irt_box1f valueRange, int numBins, int weighting, const float *bandEdges,
              int numBands);

// Measured-cost scheduling (host/irt_sched.cpp): the words of one order buffer from the measured
// costs of a frame's packets (cost: 4 per 256-pixel block, 64 per 64x64 tile).  out holds
//   [0, cap)                    the block order: tiles, or bands of max(1, tilesX / tileStride)
//                               tiles (policy 2), by descending summed cost (stable; policy 3:
//                               reversed index order), each tile's 16 blocks together and ascending;
//   [cap, cap + maxSplit)       the split work items, (packet << 8) | (part << 4) | splitLg, the
//                               parts of one packet 8 items apart, ~0u for an empty item;
//   (4 cap + 31) / 32 more      the bitmap of the split packets.
// A packet is split when its cost exceeds splitFactor x the frame's ideal span (the costs' sum over
// 20 numCU resident waves) -- costliest first, at most a tenth of the packets and maxSplit items,
// only with one-wave workgroups (wavewg) and splitLg > 0.  cap >= numBlocks, a multiple of 16.
// Returns the number of work items (a multiple of 8).
uint32_t sched_order(const uint32_t *cost, int numBlocks, int tilesX, int tileStride, int policy,
                     int splitLg, float splitFactor, int numCU, bool wavewg, size_t cap,
                     uint32_t maxSplit, uint32_t *out);

// Void packets (host/irt_void.cpp): the 8x8 packets of a launch all of whose rays, whatever the
// jitter, pass boxTest and miss the shell's outer sphere -- colour zero in every frame.  Bit
// 4 * block + wave of the launch's blocks (16 per launch tile k: frame tile tileList[k], or
// tileBegin + k * tileStride), as the chain's publish words are indexed; a packet's inactive pixels
// (x >= W or y >= H) are not looked at, one without active pixels is never flagged.  Nothing is
// flagged for another raygen, accel mode or sampler, or for a camera the float error bound does not
// cover (see the file's head).  Every member is 4 bytes wide and the pointer comes last: no padding,
// so a request compares bytewise.
struct VoidRequest {
  float cam[12];  // org, dir_00, dir_du, dir_dv
  float bmin[3], bmax[3];
  float rOuter, rInner;
  int W, H, tileBegin, tileStride, numTiles;
  int raygen, accelMode, mode;
  const int32_t *tileList;  // numTiles ids, or null
};
// the request of a launch with these parameters over a scene with these facts
inline VoidRequest void_request(const irt_launch_params &lp, const irt_volume_info &info, int W, int H, int tileBegin,
                                int tileStride, int numTiles, const int32_t *tileList) {
  VoidRequest q;
  const irt_vec3f *cam[4] = {&lp.org, &lp.dir_00, &lp.dir_du, &lp.dir_dv};
  for (int k = 0; k < 4; ++k) {
    q.cam[3 * k] = cam[k]->x;
    q.cam[3 * k + 1] = cam[k]->y;
    q.cam[3 * k + 2] = cam[k]->z;
  }
  q.bmin[0] = info.bounds.lower.x, q.bmin[1] = info.bounds.lower.y, q.bmin[2] = info.bounds.lower.z;
  q.bmax[0] = info.bounds.upper.x, q.bmax[1] = info.bounds.upper.y, q.bmax[2] = info.bounds.upper.z;
  q.rOuter = info.sphericalBounds.upper.x;
  q.rInner = info.sphericalBounds.lower.x;
  q.W = W, q.H = H, q.tileBegin = tileBegin, q.tileStride = tileStride, q.numTiles = numTiles;
  q.raygen = lp.raygen, q.accelMode = lp.accelMode, q.mode = lp.mode;
  q.tileList = tileList;
  return q;
}
inline size_t void_words(int numTiles) { return ((size_t)(numTiles > 0 ? numTiles : 0) * 64 + 31) / 32; }
// The work-item list of a launch that renders its void packets once (RenderArgs::voidList, k_render's
// OPT_VOID forms), built in the classifier's pass; a packet is 4 * block + wave, as the bitmap numbers them.
//   items[0 .. live)             the live part, the same for every frame (grid row) of the launch: the
//                                packets with an active pixel that are not void.  Block b's packets sit
//                                at indices = b mod 8, consecutive within that residue and blocks in
//                                ascending order -- the hardware deals workgroup i to XCD i mod 8, so a
//                                block's packets share one XCD's L2, as on the plain grid --; the
//                                residues are padded to one length with empty items (~0u): live % 8 == 0.
//   items[live .. live + count)  the void packets, ascending.  A launch of F frames deals them over its
//                                rows, void_row(count, F) to a row: row y's item k is void packet
//                                y * void_row + k, empty past the last.
// Packets without an active pixel are in neither part: no workgroup is dispatched for them.
// Empty (live == count == 0) when nothing is flagged: such a launch runs the plain grid.
struct VoidLists {
  std::vector<uint32_t> items;
  uint32_t live = 0, count = 0;
};
constexpr uint32_t kVoidEmpty = ~0u;
// void workgroups per grid row of a launch of F frames over `count` void packets: a multiple of 8, so
// that with `live` every row starts on XCD 0
inline uint32_t void_row(uint32_t count, int F) {
  return (uint32_t)((((uint64_t)count + (uint64_t)F - 1) / (uint64_t)F + 7) & ~(uint64_t)7);
}
// bits: void_words(numTiles) words; returns the number of packets flagged.  lists (may be null): see above
// interior (may be null): void_words(numTiles) words, the packets every ray of which passes boxTest, hits
// both spheres and takes the front-and-back ranges with every fast division's guard holding
// (host/irt_void.cpp section 4), *numInterior their number; never one of the void packets
uint32_t void_packets(const VoidRequest &q, uint32_t *bits, VoidLists *lists = nullptr, uint32_t *interior = nullptr,
                      uint32_t *numInterior = nullptr);
// ... and the last request's bitmap, kept while the request stays the same (tile lists by content)
struct VoidCache {
  std::vector<unsigned char> key;
  std::vector<uint32_t> bits;
  VoidLists lists;                      // of the same request and generation as bits
  uint32_t count = 0;                   // packets flagged (0 while the bitmap is not computed)
  std::vector<uint32_t> interior;       // the interior packets' bitmap, of the same request and generation
  uint32_t interiorCount = 0;
  bool keyed = false, valid = false;    // a request was seen; its bitmap is computed
  long long generation = 0;             // bitmaps computed so far
  // true: computed anew.  defer: a new request is only noted, and computed when it comes again
  bool lookup(const VoidRequest &q, bool defer = false);
};

// Synthetic RnBk grid generator (host/irt_synth.cpp): open once, fill any record range.
int synth_open(int rootN, int bisections, int levels, float topHeight, float noise, uint32_t seed,
               float terrainHeight,
               void **gen, size_t *total);
void synth_fill(const void *gen, size_t first, size_t count, irt_icon_cell *out);
void synth_close(void *gen);

}  // namespace irt
