// irt_kernels.h -- kernel argument block and launchers (HIP translation units only).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "icon_rt_hip.h"

namespace irt {

// Everything k_render reads: the per-frame LaunchParams (Params.h:92-119) plus the
// context-owned HBM arrays.  Passed by value (kernarg segment).
struct RenderArgs {
  // camera / frame (Params.h:100-118)
  float3 org, dir00, du, dv;
  int accumID;
  float accumW;          // 1.f / (float)(accumID + 1), the single frame's lerp weight
  float3 amb;
  float ambRad;
  float unitDistance;
  int raygen;
  // volume (Params.h:62-74)
  float3 bmin, bmax;     // Volume::bounds
  int3 dims;             // ShellAccel::dims
  float3 sbLo, sbHi;     // ShellAccel::sphericalBounds
  const float *maxOp;    // ShellAccel::maxOpacities
  int accelMode;         // Volume::accelMode (Params.h:33-34): 0 sphere (sdda), 1 grid (dda3)
  const float *gridMaxOp;  // Grid::maxOpacities, kGridDim^3 over bmin..bmax (Params.h:44-49)
  const uint32_t *gridBits;  // per kGridBlock^3 block: any majorant not <= 0 (k_grid_bits)
  int sampler;           // Volume::mode (Params.h:60): 0 cell sample() scan, 2 CUBQL wedges
  int wG;                // CUBQL_MODE wedge locator (host/irt_scene.cpp build_wedges)
  const uint32_t *wOff, *wRec;
  const float4 *wBox;    // per record: {lo.xyz, numLayers bits}, {hi.xyz, 0}
  const float4 *wTrig;   // per record: 3 corners {cosf lat, sinf lat, cosf lon, sinf lon}
  // transfer function (Params.h:77-82)
  float tfLo, tfHi, opacityScale;
  // 1 / (double)(tfHi - tfLo) and 1 / (double)(sbHi - sbLo) per axis (the float differences):
  // quotients by these per-launch divisors as one double product (div_uniform, irt_device.h)
  double invTf;
  double invSb[3];
  const float4 *lut;
  int lutSize;
  // locator
  uint32_t numCells;
  int G;
  // sRGB byte thresholds (256 entries, host/irt_host.cpp)
  const float *srgbTh;
  // output
  int W, H;
  uint32_t *fb;
  float4 *accum;
  int packed;            // 0: linear x + W*y; 1: packed 64x64 tiles
  int tileBegin, tileStride, numTiles, tilesX;
  const int32_t *tileList;  // explicit tile ids (irt_render_tile_list); null: tileBegin + k*tileStride
  unsigned long long *counters;  // [0] launched [1] inBox [2] locate [3] found [4] candidates
  // the device-atomic fallback of the per-workgroup counts (a launch past wgCountsMax
  // workgroups): kCounterBuckets x 8 counters, workgroup w adding into bucket w % 64 (one line
  // would serialise every workgroup's adds), summed into counters[0..4] by k_stats_out
  unsigned long long *counterBuckets;
  // The binned locator (irt_common.h): per cube-map cell a 32-B header, fat entries,
  // per-record height/value blocks.
  const uint4 *binHdr;
  const float4 *fat;
  const float4 *blocks;
  // zero-thickness records (spheres, host/irt_scene.cpp): sorted distinct radii, CSR into
  // (record, numLayers) pairs, and the radius hash bitmap (kSphBitWords words)
  uint32_t numSph;
  const float *sphR;
  const uint32_t *sphOff;
  const uint2 *sphRec;
  const uint32_t *sphBits;
  // per-workgroup event counts (kCnt u32 per workgroup, in pinned host memory, summed by
  // the host); null: device-scope atomics into `counters`
  uint32_t *wgCounts;
  // progressive batch (irt_render_accumulate): frames accumID .. accumID+numSamples-1;
  // for numSamples > 1 each frame's colour goes to sampleBuf[frame][lane] first
  int numSamples;
  // measured-cost workgroup scheduling of the one-kernel raygen (irt_context.hip): the
  // block order to render (null: identity) and this launch's per-block durations
  const uint32_t *schedOrder;
  uint32_t *schedCost;
  float4 *sampleBuf;
  // cooperative Woodcock loop: at most 2^coopMaxLg lanes (samples) per ray in the first
  // round of a woodcock_wave call, coopRamp powers of two more per later round (any
  // setting gives the same frame)
  int coopMaxLg;
  int coopRamp;
  // measurement only (IRT_PROBE_EXIT, profiles/): 1 = every workgroup returns at once,
  // 2 = after the prologue, 3 = after ray generation and boxTest (no pixel written), 4 = at
  // the first woodcockFunc, 5 = after it
  int probeExit;
  // persistent launch (the thread pool's queue, common/thread_pool.h:146-161, per wave):
  // non-null: kQueueWords u32 of per-XCD packet counters and a done count -- every wave pulls
  // 8x8-pixel packets (packet p: block p >> 2 over the launch's frames, the block's wave p & 3)
  // until none is left; the launch's last wave resets the counters for the next launch
  uint32_t *queue;
  uint32_t numPackets;
  // chained progressive frames (numSamples > 1, irt_render_accumulate & co.): workgroup (b, f)
  // of the launch renders block b of frame accumID + f and lerps straight into accum/fb, after
  // waiting for (b, f - 1)'s wave to publish the same pixels -- chainFlag[4 b + wave] = chainEpoch
  // + f after its write-through (sc1) stores -- instead of the sample buffer + k_accumulate.
  // The hand-off is cdna_hip_programming.md Guideline 16's R1 form (sc1 payload stores drained
  // by the storing wave, an sc1 flag store; sc1 polls and sc1 loads of every handed-off byte),
  // so it holds whichever XCD the two workgroups run on.  A frame's workgroups wait on the
  // previous frame's, which the linear dispatch order starts earlier; a wait gives up after
  // chainSpins polls and sets *chainFail (pinned host memory, one word per launch slot): the
  // frames are then unordered and the host reports IRT_E_CHAIN.
  int chain;
  // a sequence of views (irt_render_sequence; null otherwise): frame f's camera and accumID
  // as 4 float4 {org, accumID bits} {dir_00} {dir_du} {dir_dv}, uploaded before the launch and
  // read by the scalar unit in place of org/dir00/du/dv and accumID + f
  const float4 *frameCams;
  uint32_t chainEpoch;
  uint32_t *chainFlag;
  uint32_t *chainFail;
  uint32_t chainSpins;   // polls before a wait gives up (kChainSpinsDefault; tests lower it)
  int chainWithhold;     // test hook (irt_debug_set_chain_fault): this frame's waves never publish

  // measurement only (irt_debug_set_wg_trace, profiles/wg_trace.py): non-null: workgroup b
  // writes {start, end} (s_memrealtime, 100 MHz, low 32 bits), HW_ID and XCC_ID to
  // wgTrace[4b..4b+3] -- when the machine is idle at a launch's ramp and tail
  uint32_t *wgTrace;
  // a single frame's costliest packets first (one-wave workgroups, measured-cost scheduling:
  // irt_context.hip sched_prepare): numSplit work items (a multiple of 8; 0: none), item i =
  // (packet << 8) | (part << 4) | lg -- part `part` of 2^lg of packet 4 block + wave, 64 >> lg rays
  // -- rendered by the launch's workgroup i (~0u: nothing); splitMask bit p marks the listed
  // packets (their regular workgroups render nothing)
  const uint32_t *splitList;
  const uint32_t *splitMask;
  uint32_t numSplit;
  // the slot table (irt_common.h kSlot4; null: none -- the cells' radial edges are more than
  // three values in all, the headers fit the last-level cache, or IRT_SLOTS=0): slotEdge = the
  // table's edges (+inf past slotBins - 1), slotBins = table bins per slot unit, slotSubs =
  // sub-cells per slot unit (1, 2 or 4).
  // Launches with a table run the default kernels' OPT_SLOT form (VariantForms::slot).
  const float4 *slots;
  float slotEdge[3];
  int slotBins;
  int slotSubs;
  // Void packets of a chained launch of progressive frames of one camera (host/irt_void.cpp; null:
  // not in use): every ray of such a packet, whatever the jitter, passes boxTest and misses the outer
  // sphere, so each frame only scales the pixel: nv = w_f 0 + (1 - w_f) old.  One wave per launch
  // applies all numSamples lerps in order and stores accum and fb once (irt_raygen.h void_packet);
  // no other workgroup is dispatched for the packet -- no hand-off, its publish words keep an
  // earlier launch's epoch, which nothing waits for.  Such a launch runs a grid of numSamples rows
  // of voidLive + voidRow workgroups that read their packet (4 block + wave; ~0u: nothing) from
  // voidList (irt_internal.h VoidLists): workgroup x < voidLive of row y renders frame y of packet
  // voidList[x], as the plain grid's workgroup of that packet does; workgroup voidLive + k of row y
  // renders void packet j = y voidRow + k, voidList[voidLive + j], if j < voidCount.
  // (voidBits keeps its place: every other field's offset is the one the kernels without a void form
  // were compiled with before the list came)
  // The launches without a list (OPT_VLIST: the terrain kernels, and rows no shorter than the plain
  // grid's) keep the plain grid and test the packet's bit, 4 block + wave: frame 0's wave of a void
  // packet renders it, the later frames' waves return at once.
  const uint32_t *voidBits;
  const uint32_t *voidList;
  uint32_t voidLive, voidRow, voidCount;
  // Interior packets of such a launch (host/irt_void.cpp section 4; 0: none flagged): every ray passes
  // boxTest, hits both spheres and takes the front-and-back ranges, so the OPT_VOID kernels -- all
  // four, within the registers, spills and LDS they had -- set the ray up
  // without the box test, the range selection and the fallback divisions.  The list carries the class in the live item's top bit (kItemInterior); the
  // bitmap form in a second bitmap behind the first, at voidBits + 2 numTiles.  (In the struct's tail
  // padding: no other field moves, and the kernels without OPT_VOID are the parent's byte for byte.)
  uint32_t interior;
};
// a live work item of an interior packet, as the device copy of the work-item list carries it (the
// host's list, VoidLists::items, keeps plain packet numbers; ~0u stays the empty item)
constexpr uint32_t kItemInterior = 1u << 31;
// a persistent launch's queue words (irt_render.hip queue_take): 8 per-XCD counters and the
// done count, each on its own 128-B line
constexpr int kQueueLine = 32;
// polls of a chained wait (an L2 round trip + s_sleep 2 each: ~1 s in all) before it gives up
constexpr uint32_t kChainSpinsDefault = 1u << 20;
constexpr int kQueueWords = 9 * kQueueLine;

// Event counts kept per workgroup: [0] launched [1] inBox [2] locate [3] found [4] candidates
constexpr int kCnt = 8;

// Render-kernel variants: a bit set of these OPT_* flags (bits 8-11: minimum waves per SIMD).
// All give identical results.  (A/B): compiled only into the A/B library, make VARIANTS=all.
// The switches that were measured, lost and removed are listed in DESIGN.md section 5.
enum : int {
  OPT_WEDGE = 16384,  // CUBQL / TRIANGLE samplers (locate_wedge, locate_tri); kept out of
                      // the default kernels
  OPT_GRID = 8192,    // GRID_ACCEL_MODE traversal (render_grid); likewise
  OPT_STATS = 32768,  // per-wave statistics into counters[5..15] (measurement only; with the
                      // cooperative loop [7] entry hops, [8] locate rounds, [12..15] samples by
                      // candidates tested 0/1/2/>=3)
  OPT_SERIAL = 65536, // one lane per ray through the Woodcock loop (render_pixel), for A/B:
                      // the default user-geometry/sphere kernel is render_pixel_coop
  OPT_SCAN1 = 131072, // the cooperative loop with each lane's candidate scan on its own
                      // (locate), for A/B against Tracer::locate_wave
  OPT_TIMING = 524288,  // measurement only: per-wave shader-clock time by region into
                        // counters[5..15] (Tracer::tmark)
  OPT_WAVEWG = 4194304,   // (with OPT_LEAN) one wave per workgroup: a wave's LDS is freed as
                          // soon as it finishes, instead of when its workgroup's last wave does
  OPT_LEAN = 2097152,   // less LDS per workgroup (31.0 -> 24 KB), so that more workgroups
                        // fit a CU while finished waves wait for their workgroup's last one:
                        // the sRGB thresholds and the sphere hash read from global memory
                        // (L1/L2), the accum pixel loaded at the end instead of prefetched
  OPT_QUEUE = 16777216,  // the persistent launch (RenderArgs::queue): every resident wave pulls
                        // 8x8-pixel packets from the launch's counter; its own instantiation
                        // of the default kernel (k_render's grid launch is unchanged)
  OPT_FASTSPH = 33554432,  // (A/B) the sdda entry/exit cells from the certified fast lat/lon
                           // (irt_device.h spherical_fast, glibc-exact fallback near cell edges):
                           // no gain at C3, C5 3 % slower (profiles/r04b/) -- the setup waits on
                           // the majorant gather, not on asinf/atan2f
  OPT_SPLIT = 8,  // measured-cost work items (RenderArgs::splitList): the launches of a single frame
                  // that split packets run this instantiation of the default kernels (VariantForms::split)
  OPT_DPPSCAN = 32,  // groups of 2, 4, 16 and 64 lanes take the round's prefix t0 - d0 - ... - dk
                     // by DPP steps across lanes (woodcock_wave), not each lane from LDS
  OPT_DMATAB = 67108864,  // one-wave workgroups: the LCG jump and logf tables loaded into
                          // LDS by LDS-DMA, not waited for in the prologue (k_render)
  OPT_NOMISS = 262144,  // the user-geometry cooperative loop without its miss mode:
                        // every sample outside all cells ends its ray's round (round 4's
                        // default); convert_icon terrain leaves voids under land, where such runs
                        // cost one round per miss
  OPT_VOIDLOC = 1073741824,  // the solo lanes' void walk also in located mode: a certain miss at
                             // the round's sample switches the ray to miss mode there, not a round
                             // later; scenes with holes run it since round 6 (scene_variant:
                             // profiles/r06zg/ C3t chained -1.7 %, single frames even)
  OPT_NOVOIDRUN = 2,   // (A/B) the miss-mode kernels without the solo lanes' void walk (woodcock_wave)
  OPT_NOHOLESKIP = 4,  // (A/B) the miss-mode kernels without the quad-bound miss test (Tracer::locate_wave:
                       // a sample outside its quad's radial range is outside every cell, no
                       // candidate tested)
  OPT_SLOT = 128,  // the wave-wide scan starts from the slot table (RenderArgs::slots, irt_common.h
                   // kSlot4): the first admitted candidate and the list's position in one gather,
                   // instead of the header, then the entry; launches on a scene with a table run
                   // this instantiation of the default kernels (VariantForms::slot)
  OPT_VOID = 16,  // the default kernels' form for chained launches that carry a void-packet bitmap
                  // (RenderArgs::voidList; plan_render): the workgroup's packet is read from the list at
                  // the kernel's top.  Every other launch runs the kernels without it, as before
  OPT_VLIST = 64,  // with OPT_VOID: the launch runs rows of work items (RenderArgs::voidList) instead
                   // of the plain grid with the bitmap; the flat kernel only (the terrain kernels'
                   // list form needs scratch), and only where the rows are shorter than the plain grid's
  // bits 8-11: minimum waves per SIMD asked of the register allocator (0: none)
};
// OPT_MONO is kept in the numbering of round 1 (the one-kernel raygen; the setup -> march ->
// continuation pipeline it distinguished from was removed): every listed variant sets it, and
// make_forms (irt_render.hip) masks it off.
// 5376 (the default until round 4): four-wave workgroups at 5 waves/SIMD, 96 VGPRs, the few spills
// in the prologue and epilogue only; 5120: the same kernel at 4 waves/SIMD (117 VGPRs).  70656 =
// 5120 | OPT_SERIAL: the one-lane-per-ray Woodcock loop, against the cooperative loop.  2102272 =
// 5120 | OPT_LEAN (24 KB of LDS per workgroup), 2102528 the same at 5 waves/SIMD; 6296576 /
// 6296832 = 2102272 / 2102528 | OPT_WAVEWG (one-wave workgroups); 73405696 = 6296832 | OPT_DMATAB,
// 73405728 = 73405696 | OPT_DPPSCAN (the default since round 5), 73667872 its hole-free form (|
// OPT_NOMISS), 1147147552 its form for scenes with holes (| OPT_VOIDLOC).  73930016 / 74192160: the
// default / its hole-free form with OPT_TIMING (per-region shader clocks, profiles/probe.py;
// s_memtime slows them ~17x).
constexpr int OPT_MONO = 4096;
// one kernel per frame, 5 waves/SIMD (96 VGPRs; spills only in the prologue/epilogue): against
// 4 waves C3 -1.8 %, C4 -4.9 %, comb TF -9 %, C5 +1.9 % (profiles/r03u_waves/)
// Round 4: one-wave workgroups with the leaner LDS (OPT_WAVEWG | OPT_LEAN, 5 waves/SIMD): a
// finished wave frees its slot at once instead of when its 256-pixel block's slowest wave does;
// against 5376 (four-wave workgroups) with chained frames C3 -1.7 %, C3s -5.8 %, C4 -1.1 %, C5
// -2.3 %, a single C3 frame -1.1 % (profiles/r04p_ab/)
// Round 5: + OPT_DMATAB (67108864: the prologue's LCG-jump and logf tables by LDS-DMA, with no
// wait before the ray generation): against 6296832 C3 -1.2 %, one frame per launch -1.7 %, C5
// -2.5 %, C3t -1.2 %, C3s -0.3 % (profiles/r05k_dmatab/); + OPT_DPPSCAN (32: the round's prefix
// by DPP steps across lanes): C3t -1.1 %, comb TF -1.3 %, C3 -0.3 % (profiles/r05p_ab/)
constexpr int kDefaultVariant = 73405728;
// Round 5: the raygen's miss mode (woodcock_wave) is on in the default variant; a scene
// without holes (every column starting at the same radius, no gaps inside columns) runs it
// without (bit 262144, OPT_NOMISS): C3 -2.3 %, while convert_icon terrain (voids under land)
// runs 2.25x faster with it (profiles/r05d/)
constexpr int kNoMissBit = OPT_NOMISS;
// measured-cost scheduling (irt_context.hip sched_prepare): at most this many work items run first
// in a single frame (RenderArgs::splitList), a multiple of 8
constexpr uint32_t kMaxSplit = 4096;
// Round 6: a scene with holes also walks a certain miss in located mode (bit 1073741824,
// OPT_VOIDLOC: a solo lane whose sample is outside its quad's records switches its ray to the miss
// mode in the same round and walks on): C3t 8 chained frames -1.7 %, one per launch even
// (profiles/r06zg/)
constexpr int kVoidLocBit = OPT_VOIDLOC;
// The Tracer instantiation of VariantForms::wedge, the kernel of the unstructured samplers'
// sphere-accel launches (256-thread workgroups, full LDS, no waves-per-SIMD floor), which
// k_debug_locate_sampler runs too
constexpr int kSamplerVariant = ((kDefaultVariant & ~OPT_MONO) & ~(0xF00 | OPT_WAVEWG | OPT_LEAN)) | OPT_WEDGE;
inline int scene_variant(bool holes) { return holes ? kDefaultVariant | kVoidLocBit : kDefaultVariant | kNoMissBit; }

// The launcher (irt_render.hip, "variants / launcher").  A variant's kernels, one per launch form:
// fn null where the variant has no such form, id the kernel's template argument (k_render<id>),
// threads its workgroup size.
typedef void (*RenderKernel)(RenderArgs);
struct KernelForm {
  RenderKernel fn;
  int id;
  int threads;
};
struct VariantForms {
  int variant;
  // the user-geometry sphere path: the plain grid; a single frame's measured-cost work items first
  // (RenderArgs::splitList); the scan from the slot table (RenderArgs::slots), and both; chained
  // frames with the void-packet bitmap (RenderArgs::voidBits) or rows of work items
  // (RenderArgs::voidList); the persistent launch (RenderArgs::queue)
  KernelForm plain, split, slot, slotSplit, voidBits, voidList, queue;
  // the grid accelerator; the unstructured samplers over the shell's spheres and over the grid
  KernelForm grid, wedge, wedgeGrid;
};
const VariantForms *forms_of(int variant);  // null: not compiled
// ... and for a variant that is not compiled the default's forms
inline const VariantForms &render_forms(int variant) {
  const VariantForms *f = forms_of(variant);
  return f ? *f : *forms_of(kDefaultVariant);
}
int render_variants(int *out, int cap);  // the compiled variants (count; the first cap into out)
bool render_queue_compiled();  // some variant has a persistent form: the A/B library (make VARIANTS=all) only

// What a launch may put into its arguments is read from the table: the forms below exist on the
// user-geometry sphere path only (the grid accelerator and the samplers have one kernel each).
inline bool render_sphere_path(const RenderArgs &A) {
  return A.sampler == IRT_MODE_USER_GEOM && A.accelMode != IRT_ACCEL_GRID;
}
// a single frame can run measured-cost work items (RenderArgs::splitList)
inline bool render_split_ok(const VariantForms &F, const RenderArgs &A) {
  return render_sphere_path(A) && F.split.fn != nullptr;
}
// a chained launch can merge its void packets (RenderArgs::voidBits, or voidList where F.voidList
// exists): these forms have no slot-table, work-item or persistent sibling
inline bool render_void_ok(const VariantForms &F, const RenderArgs &A) {
  return render_sphere_path(A) && F.voidBits.fn != nullptr && !A.slots && !A.queue && !A.numSplit && !A.schedOrder;
}
// the launch can be persistent (RenderArgs::queue)
inline bool render_queue_ok(const VariantForms &F, const RenderArgs &A) {
  return render_sphere_path(A) && F.queue.fn != nullptr;
}
// workgroups a persistent launch runs on a device with numCU compute units: every slot the queue
// kernel's occupancy allows (resident at once), at most `numBlocks`
int render_queue_wgs(const VariantForms &F, int numCU, int numBlocks);

// One launch: its kernel, its grid (workgroups = grid.x * grid.y: what the per-workgroup count ring
// is sized by) and k_accumulate's grid, the frame's 256-pixel blocks.
struct RenderPlan {
  KernelForm form;
  dim3 grid;
  size_t workgroups;
  int accumBlocks;
};
// The only place that maps a launch's arguments to a kernel and a grid.  queueWG: the workgroups of
// a persistent launch (A.queue; render_queue_wgs), unused otherwise.
RenderPlan plan_render(const VariantForms &F, const RenderArgs &A, int queueWG);
// launches the plan, and k_accumulate behind it for unchained progressive frames
void launch_render(const RenderArgs &A, const RenderPlan &plan, hipStream_t s);
// one empty launch of each of the variant's sphere-path kernels: the runtime's first-launch setup
// happens at context creation, not in the first frame
void prewarm_render(const VariantForms &F, hipStream_t s);
void launch_debug_locate(const RenderArgs &A, const float *xyz, int n, int *found, float *value,
                         hipStream_t s, bool wave);
// the unstructured samplers' point location (A.sampler: IRT_MODE_CUBQL or IRT_MODE_TRIANGLES)
// through the Tracer of their sphere-accel launches; value[i] is 0 where found[i] is
void launch_debug_locate_sampler(const RenderArgs &A, const float *xyz, int n, int *found, float *value,
                                 hipStream_t s);
void launch_shell_init(float *valueRanges, size_t numMCs, hipStream_t s);
// rects (null: not kept): per record its clamped shell rectangle {ylo, yhi, zlo, zhi}, ylo > yhi
// for a record that rasterises nothing -- what launch_shell_rebuild needs of the records
void launch_shell_build(const irt_icon_cell *cells, size_t n, int3 dims, float3 lo, float3 hi,
                        float *valueRanges, ushort4 *rects, hipStream_t s);
// irt_update_values*: values[k * 32 + j] becomes value[j] of record first + k in its block (the
// value halves only); d_values: device memory, 128 B per record
void launch_value_scatter(const float *d_values, size_t first, size_t n, float4 *blocks, hipStream_t s);
// irt_update_values_end: the shell's value ranges (initialised by launch_shell_init) from the
// blocks, meta words and stored rectangles, as launch_shell_build makes them from the records;
// stat[0..2] (preset to float_key(+inf), float_key(-inf), 0): the data range's least and greatest
// float_key and the last zero (k_shell_rebuild, irt_kernels.hip)
void launch_shell_rebuild(const float4 *blocks, const uint32_t *meta, const ushort4 *rects, size_t n,
                          int3 dims, float *valueRanges, unsigned long long *stat, hipStream_t s);
void launch_grid_build(const float4 *blocks, const uint32_t *meta, const float4 *trig, size_t n,
                       float3 lo, float3 hi, float *valueRanges, hipStream_t s);
void launch_grid_bits(const float *maxOp, uint32_t *bits, hipStream_t s);
// the TF's mean Woodcock samples per acceptance over the macrocells: out[0] += sum, out[1] += count
// (k_accept_stat, irt_kernels.hip)
void launch_accept_stat(const float *valueRanges, const float *maxOp, size_t numMCs, const float4 *lut, int size,
                        float lo, float hi, double *out, hipStream_t s);
void launch_max_opacities(const float *valueRanges, size_t numMCs, const float4 *lut, int size,
                          float lo, float hi, float *maxOp, hipStream_t s);
void launch_clear(uint32_t *fb, float4 *accum, size_t n, hipStream_t s);
constexpr int kCounterBuckets = 64;
// copies a launch's 16 counters to the host (plus, with `buckets`, the bucketed fallback
// counts, whose buckets it zeroes again) and zeroes the next launch's block
void launch_stats_out(const unsigned long long *cur, unsigned long long *host,
                      unsigned long long *next, unsigned long long *buckets, hipStream_t s);
void launch_copy_u32(const uint32_t *src, uint32_t *dst, size_t n, hipStream_t s);
// The scene build on the device (irt_build.hip): per-record blocks and the binned cube-map
// locator (irt_build.h) from the cells and their glibc corner trig in HBM.  On success the
// caller owns blocks / binHdr / fat; on failure it frees whatever is non-null.
struct DeviceScene {
  float4 *blocks = nullptr;
  uint32_t *meta = nullptr;  // per record (irt_build.h record_meta), kept for the lazy grid build
  uint4 *binHdr = nullptr;
  float4 *fat = nullptr;
  size_t entries = 0, binEntries = 0, bigCells = 0, bytes = 0;
};
int build_scene_device(const irt_icon_cell *d_cells, const float4 *d_trig, size_t n, size_t numRuns,
                       int G, hipStream_t s, DeviceScene &out);
// The slot table (irt_common.h kSlot4) of a built scene whose cells' radial edges are at most
// three values in all, if it fits in maxBytes (and the device's free memory); otherwise slots
// stays null.
struct SlotTable {
  float4 *slots = nullptr;
  int bins = 0;
  int subs = 0;  // sub-cells per slot unit (irt_common.h slot_unit; IRT_SLOT_SUBS=1|2|4)
  float edges[3] = {0.f, 0.f, 0.f};
  size_t bytes = 0;
  const char *skipped = nullptr;  // why no table was built (nullptr: built, or not asked for)
};
// Round 5: with the table C5 -9 %, C3s -3 %, but C3 +4 %, C4 +3 % (profiles/r05aa/): on by
// default only when the headers exceed the 256-MB last-level cache (C5: 2.7 GB; C3: 167 MB).
// Round 6: slot units of 2 or 4 sub-cells (a half or a quarter of the table): C5 -7.6 % / -6.0 %
// against no table, one sub-cell -7.5 to -9 % (profiles/r06x/); the default unit keeps the
// table within the scene's own bytes (C5: quads, 32 GB)
constexpr size_t kSlotAutoHdrBytes = (size_t)256 << 20;
// subs: sub-cells per slot unit (irt_common.h slot_unit), 1, 2 or 4; any other value: the finest
// unit whose table is at most autoBytes (and maxBytes), else 4
int build_slots_device(const uint32_t *hdr, const float4 *fat, uint32_t numCells, size_t maxBytes, int subs,
                       size_t autoBytes, hipStream_t s, SlotTable &out);
void launch_unpack(const uint32_t *gathered, int numRanks, int maxTiles, int W, int H,
                   uint32_t *fb, hipStream_t s, const int32_t *table = nullptr);

}  // namespace irt
