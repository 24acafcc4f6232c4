// irt_render.hip -- the hot path: the raygens woodcockTrackingWithAccel and
// woodcockTrackingAE (icon_rt/deviceCode.cu:239-341) as one gfx950 kernel.
//
// Mapping: one lane per pixel, one wave64 per 8x8 pixel packet (neighbouring rays visit
// the same cube-map cells, fat entries and majorants), a 256-thread workgroup per 16x16
// block, 16 workgroups per 64x64 frame tile -- the unit the reference's CPU parallel_for
// hands out (common/for_each.h:70-85) and the unit of the multi-GPU frame split.
//
// Where the time goes (profiles/): the kernel is a chain of dependent gathers per
// Woodcock sample -- cube-map cell header -> fat candidate entry -> height/value block --
// plus the VALU of the ray setup.  Design choices that follow from that:
//   * the binned locator (irt_common.h): a sample costs ~3 round trips instead of ~10;
//   * one Woodcock call site (the locate code is inlined once), counters aggregated per
//     wave in LDS, coarse height keys fetched only after the plane tests pass: fewer live
//     VGPRs, so more waves per SIMD hide the gathers;
//   * the sdda exit-point toSpherical (two glibc-exact asinf/atan2f) is evaluated only
//     when a later range can still read the RNG state it drives (see below).
//
// Bit-exactness: irt_common.h / irt_device.h and DESIGN.md section 3.
//
// One translation unit in three files: irt_tracer.h (sampling: the locators and the Woodcock
// loops, Tracer<OPT>), irt_raygen.h (one pixel's ray: generation, ranges and leaves, the pixel
// write) and this file -- the persistent launch's packet queue, the kernels (k_render,
// k_accumulate, the three k_debug_locate*) and the variant list with its launchers.

#include <initializer_list>

#include "irt_raygen.h"

namespace irt {

// The persistent launch's packet queues (RenderArgs::queue, kQueueWords u32 per launch slot):
// one counter per XCD, each on its own 128-B line, and the launch's done count.  XCD x owns
// the 16x16 blocks g (over every frame of the launch) with g % 8 == x -- the grid launch's
// workgroup-to-XCD deal, so each XCD's L2 sees the blocks it would have seen -- and hands out
// their packets in order; a wave on XCD x takes from queue x, and once that is exhausted from
// the others in turn (a plain load first, so finished queues cost no read-modify-write).  (One
// counter for the whole launch, with the next fetch issued at each packet's start: 0.40 ms per
// C3 frame against 0.09, profiles/r04b/.)  The launch's last wave resets every counter (each
// wave's last fetch precedes its done count).
constexpr int kQueueXcds = 8;
struct QueueCursor {
  int cur;        // the queue this wave takes from
  uint32_t dead;  // bit x: queue x is exhausted
};
__device__ __forceinline__ uint32_t queue_take(uint32_t *Q, uint32_t numBlocksAll, QueueCursor &c) {
  while (c.dead != (1u << kQueueXcds) - 1u) {
    const uint32_t x = (uint32_t)c.cur;
    // blocks g < numBlocksAll with g % 8 == x, four packets each
    const uint32_t limit = numBlocksAll > x ? 4u * ((numBlocksAll - x + kQueueXcds - 1) / kQueueXcds) : 0u;
    uint32_t v = 0xFFFFFFFFu;
    if (__lane_id() == 0) {
      uint32_t *q = Q + (size_t)x * kQueueLine;
      if (__hip_atomic_load(q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < limit) v = atomicAdd(q, 1u);
    }
    v = __builtin_amdgcn_readfirstlane(v);
    if (v < limit) return ((v >> 2) * kQueueXcds + x) * 4u + (v & 3u);  // block g's packet v & 3
    c.dead |= 1u << x;
    c.cur = (c.cur + 1) & (kQueueXcds - 1);
  }
  return 0xFFFFFFFFu;
}
__device__ __forceinline__ void queue_done(uint32_t *Q) {
  if (__lane_id() == 0) {
    __threadfence();
    const uint32_t waves = gridDim.x * (blockDim.x >> 6);
    if (atomicAdd(&Q[kQueueXcds * kQueueLine], 1u) == waves - 1u) {
      for (int x = 0; x <= kQueueXcds; ++x)
        __hip_atomic_store(&Q[(size_t)x * kQueueLine], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

// The raygen over the frame grid: one lane per pixel (see pixel_of).
template <int OPT>
__global__ void __launch_bounds__((OPT & OPT_WAVEWG) ? 64 : 256,
                                  ((OPT >> 8) & 15) ? ((OPT >> 8) & 15) : 1)
    k_render(RenderArgs A) {
  constexpr bool lean = (OPT & OPT_LEAN) != 0;
  constexpr bool wavewg = (OPT & OPT_WAVEWG) != 0;
  constexpr int kWpg = wavewg ? 1 : 4;  // waves per workgroup
  constexpr bool split = kWpg < 4;  // several workgroups per 256-pixel block
  static_assert(!split || (lean && Tracer<OPT>::kCoop), "one-wave workgroups: lean, cooperative kernels");
  constexpr int kT = 64 * kWpg;   // threads per workgroup
  constexpr int kW = kT / 64;            // waves per workgroup
  __shared__ float s_th[lean ? 1 : 256];
  __shared__ uint32_t s_cnt[kCnt];
  __shared__ LogfTab s_logf[16];
  __shared__ uint32_t s_sph[lean ? 1 : kSphBitWords];
  __shared__ int4 s_dda[split ? 1 : 256];  // sdda state needed only after a range's first leaf
  __shared__ float4 s_entry[kT];
  __shared__ CoopWave s_coop[kW];   // the cooperative Woodcock loop (kCoop kernels)
  __shared__ ScanWave s_scan[Tracer<OPT>::kWaveScan ? kW : 1];  // its wave-wide candidate scan
  __shared__ float4 s_acc[lean ? 1 : 256];  // kCoop: the accum pixels, prefetched
  __shared__ uint2 s_jmp[kLcgJumps];  // lcg_jump's {mul, add} (kLcgJumpTab)
  const int tid = threadIdx.x;
  if (A.wgTrace && tid == 0) {  // measurement only: the workgroup's start, where it ran
    uint32_t *w = A.wgTrace + 4 * (blockIdx.y * gridDim.x + blockIdx.x);
    w[0] = (uint32_t)__builtin_amdgcn_s_memrealtime();
    w[2] = __builtin_amdgcn_s_getreg((31 << 11) | 4);   // HW_REG_HW_ID
    w[3] = __builtin_amdgcn_s_getreg((15 << 11) | 20);  // HW_REG_XCC_ID
  }
  if (A.probeExit == 1) return;  // measurement only
  // Void packets (OPT_VOID: the kernels of launches with A.voidList -- chained progressive frames of
  // one camera; irt_launch.hip prepare_void, plan_render): the workgroup's packet from the launch's
  // work-item list, by the scalar unit, before anything else is in flight -- the prologue's LDS-DMA
  // included.  Such a launch has no block order and no split items.  Row (blockIdx.y = frame) y is
  // voidLive live items, the same in every row, then voidRow void items (RenderArgs::voidList).
  //   No deadlock: a live packet's wave of frame y waits for its wave of frame y - 1 alone, which has
  // the same blockIdx.x one row up and so is dispatched before it (rows are dispatched in order);
  // void and empty items wait for nothing.
  //   XCD locality: voidLive + voidRow is a multiple of 8, so every row starts on XCD 0 and workgroup x
  // runs on XCD x % 8; block b's live packets sit at x = b mod 8 (VoidLists), so they share that XCD's
  // L2 in every frame, as on the plain grid.
  //   The terrain kernels' list form leaves the resource gate (8 B of scratch, profiles/r09a_compact/
  // resources.txt), so only the flat kernel has one (OPT_VLIST); the others keep the bitmap on the
  // plain grid: the packet's bit (RenderArgs::voidBits), frame 0's wave renders the void packet and
  // the later frames' waves return at once.
  constexpr bool kVoid = (OPT & OPT_VOID) != 0;
  constexpr bool kList = kVoid && (OPT & OPT_VLIST) != 0;
  static_assert(kVoid || (OPT & OPT_VLIST) == 0, "OPT_VLIST: a form of the OPT_VOID kernels");
  uint32_t vitem = 0u;  // kList: this workgroup's packet (4 block + wave)
  // Interior packets (RenderArgs::interior; every OPT_VOID kernel): the
  // packet's class by the scalar unit -- the live item's top bit, read here with the packet; the
  // bitmap form reads the second bitmap's bit at the ray setup (nothing held through the prologue)
  // -- for the ray setup's one scalar branch (render_pixel_coop)
  uint32_t interior = 0u;
  static_assert(!kVoid || (wavewg && lean && Tracer<OPT>::kCoop &&
                           (OPT & (OPT_SPLIT | OPT_SLOT | OPT_STATS | OPT_TIMING | OPT_QUEUE | OPT_GRID | OPT_WEDGE)) == 0),
                "void packets: the default kernels' plain grid form");
  if constexpr (kVoid && !kList) {
    // (the arguments through fresh_args(): nothing this test loads stays live into the raygen)
    const RenderArgs &VA = fresh_args();
    const uint32_t vb = blockIdx.x, vwave = (vb >> 3) & 3u;
    const uint32_t vblk = ((vb >> 5) << 3) | (vb & 7u), vpkt = vblk * 4u + vwave;
    uint32_t isVoid = VA.voidBits ? (scalar_word(VA.voidBits, vpkt >> 5) >> (vpkt & 31u)) & 1u : 0u;
    asm volatile("" : "+s"(isVoid));  // one opaque scalar branch: the raygen below compiles as without it
    if (isVoid) {
      void_packet(VA, vblk, (int)vwave, blockIdx.y == 0, 1u);
      return;
    }
  }
  if constexpr (kList) {
    const RenderArgs &VA = fresh_args();
    const uint32_t vx = blockIdx.x, vlive = VA.voidLive;
    // row y's void item k: void packet j = y voidRow + k, if there is one
    const uint32_t j = blockIdx.y * VA.voidRow + (vx - vlive);
    const bool inVoid = vx >= vlive, none = inVoid && j >= VA.voidCount;
    // (always a read inside the list's voidLive + voidCount words, voidCount > 0)
    const uint32_t w = scalar_word(VA.voidList, none ? 0u : inVoid ? vlive + j : vx);
    vitem = __builtin_amdgcn_readfirstlane(none ? ~0u : w);
    // void items and the padding (~0u, in either part) end here, before the prologue
    uint32_t leave = __builtin_amdgcn_readfirstlane(inVoid || vitem == ~0u ? 1u : 0u);
    asm volatile("" : "+s"(leave));  // one opaque scalar branch: the raygen below compiles as without it
    if (leave) {
      const bool some = vitem != ~0u;
      void_packet(VA, some ? vitem >> 2 : 0u, (int)(some ? vitem & 3u : 0u), some, some ? (uint32_t)VA.numSamples : 0u);
      return;
    }
    // a live item: its class, then the plain packet number
    interior = vitem >> 31;
    vitem &= ~kItemInterior;
  }
  uint64_t tStart = 0;
  if constexpr ((OPT & OPT_TIMING) != 0) tStart = __builtin_amdgcn_s_memtime();
  // OPT_DMATAB (one-wave workgroups): the LCG jump and logf tables go straight from global
  // memory into LDS (global_load_lds, 16 B per lane: 1,040 + 256 B), and nothing waits for them
  // here -- the compiler's LDS-DMA tracking puts the vmcnt wait before their first read, in the
  // first Woodcock round, so the ray generation and setup overlap the loads (the register path
  // below waits for two round trips before the first ray is generated)
  constexpr bool dmaTab = (OPT & OPT_DMATAB) != 0 && kT == 64 && Tracer<OPT>::kCoop;
  if constexpr (dmaTab) {
    typedef __attribute__((address_space(3))) void *LdsPtr;
    const char *jt = reinterpret_cast<const char *>(&kLcgJumpTab.ma[0][0]);
    static_assert(sizeof(kLcgJumpTab.ma) == kLcgJumps * 8 && kLcgJumps * 8 <= 64 * 16 + 16, "jump table: 65 chunks");
    __builtin_amdgcn_global_load_lds((const void *)(jt + 16 * tid), (LdsPtr)s_jmp, 16, 0, 0);
    if (tid == 0)
      __builtin_amdgcn_global_load_lds((const void *)(jt + 1024), (LdsPtr)(reinterpret_cast<char *>(s_jmp) + 1024), 16, 0, 0);
    static_assert(sizeof(LogfTab) == 16, "logf table: one chunk per entry");
    if (tid < 16) __builtin_amdgcn_global_load_lds((const void *)(kLogfTab + tid), (LdsPtr)s_logf, 16, 0, 0);
  }
  // the prologue's global loads issued together, one wait (not one round trip each)
  const float th = lean ? 0.f : A.srgbTh[tid];
  const LogfTab lt = dmaTab ? LogfTab{0.0, 0.0} : kLogfTab[tid & 15];
  uint32_t sph[kSphBitWords / 256];
  if (!lean && A.numSph) {
#pragma unroll
    for (int k = 0; k < kSphBitWords / 256; ++k) sph[k] = A.sphBits[tid + 256 * k];
  }
  uint2 jmpv[(kLcgJumps + kT - 1) / kT];
#pragma unroll
  for (int k = 0; k < (kLcgJumps + kT - 1) / kT; ++k) {
    const int j = tid + kT * k;
    jmpv[k] = make_uint2(0u, 0u);
    if (!dmaTab && Tracer<OPT>::kCoop && j < kLcgJumps) jmpv[k] = make_uint2(kLcgJumpTab.ma[j][0], kLcgJumpTab.ma[j][1]);
  }
#pragma unroll
  for (int k = 0; k < (kLcgJumps + kT - 1) / kT; ++k) {
    const int j = tid + kT * k;
    if (!dmaTab && Tracer<OPT>::kCoop && j < kLcgJumps) *reinterpret_cast<uvec2 *>(&s_jmp[j]) = __builtin_bit_cast(uvec2, jmpv[k]);
  }
  if constexpr (!lean) s_th[tid] = th;
  if (!dmaTab && tid < 16) s_logf[tid] = lt;
  if (!lean && A.numSph) {
#pragma unroll
    for (int k = 0; k < kSphBitWords / 256; ++k) s_sph[tid + 256 * k] = sph[k];
  }
  if (tid < kCnt) s_cnt[tid] = 0;
  __shared__ uint32_t s_done;  // waves of this workgroup finished (the epilogue)
  if (tid == 0) s_done = 0;
  __shared__ uint32_t s_gbits[(OPT & OPT_GRID) ? kGridBitWords : 1];
  if constexpr ((OPT & OPT_GRID) != 0) {
#pragma unroll
    for (int k = 0; k < kGridBitWords / 256; ++k) s_gbits[tid + 256 * k] = A.gridBits[tid + 256 * k];
  }
  if constexpr (dmaTab)
    __builtin_amdgcn_wave_barrier();  // one wave: its LDS writes are ordered; no wait for the DMA
  else
    __syncthreads();
  if (A.probeExit == 2) return;  // measurement only
  Tracer<OPT> T{{}, A, s_logf, lean ? A.sphBits : s_sph, s_cnt, {0, 0, 0, 0, 0, 0, 0}};
  T.s_gbits = s_gbits;
  const float *th_p = lean ? A.srgbTh : s_th;
  // OPT_WAVEWG: four one-wave workgroups per 256-pixel block.  The hardware deals workgroup i
  // to XCD i % 8, so workgroup i renders wave (i >> 3) & 3 of block ((i >> 5) << 3) | (i & 7):
  // a block's four packets share one XCD's L2, as the four waves of a 256-thread workgroup do
  // (numBlocks is a multiple of 16)
  constexpr uint32_t kNwb = 4 / kWpg;  // workgroups per block
  // A single frame's costliest packets first (A.numSplit, measured-cost scheduling): the
  // launch's first numSplit workgroups render the work items splitList[b] = (packet << 8) | (part
  // << 4) | lg -- part `part` of 2^lg of the packet: its rays part * (64 >> lg) .. on lanes 0 ..
  // (64 >> lg) - 1 (lg = 0: the whole packet) --, ~0u an empty item (numSplit is a multiple of 8);
  // the regular workgroups follow, and those of the listed packets render nothing.
  uint32_t bx = blockIdx.x;
  int partSel = -1;  // (part << 8) | lg for a listed item, -1 for a regular workgroup
  uint32_t splitP = 0u;
  bool emptyItem = false;
  constexpr bool splitOk = wavewg && (OPT & OPT_SPLIT) != 0;
  if constexpr (splitOk) {
    if (bx < A.numSplit) {
      const uint32_t item = scalar_word(A.splitList, bx);
      emptyItem = item == ~0u;
      partSel = emptyItem ? 0 : (int)((((item >> 4) & 15u) << 8) | (item & 15u));
      splitP = emptyItem ? 0u : item >> 8;
    } else {
      bx -= A.numSplit;
    }
  }
  const uint32_t wg = split ? (((bx >> 3) / kNwb) << 3) | (bx & 7u) : bx;
  const int wwave = kList ? (int)(vitem & 3u) : partSel >= 0 ? (int)(splitP & 3u)
                                  : split ? (int)(((bx >> 3) % kNwb) * kWpg) : 0;  // the block's first wave in this workgroup
  const int ptid = split ? wwave * 64 + tid : tid;
  if constexpr ((OPT & OPT_TIMING) != 0) {
    T.tLast = tStart;
    T.tmark(0);  // prologue
  }
  const uint64_t c0 = A.schedCost ? wall_clock64() : 0;
  // grid.y = frame k of a progressive batch (accumID + k), whose colour goes to the sample
  // buffer for k_accumulate; a single frame writes accum/fb directly.  With measured-cost
  // scheduling (irt_context.hip) workgroup b renders block order[b].
  const uint32_t blk = kList ? vitem >> 2 : partSel >= 0 ? splitP >> 2 : A.schedOrder ? scalar_word(A.schedOrder, wg) : wg;  // uniform: an SGPR
  // a split packet's regular workgroup: nothing to render (its counts and trace are still written)
  const uint32_t pkt = blk * 4u + (uint32_t)wwave;
  const bool splitAway = splitOk && partSel < 0 && ((scalar_word(A.splitMask, pkt >> 5) >> (pkt & 31u)) & 1u);
  uint32_t launched = 0u;  // rays of this wave's pixels (uniform)
  bool pxActive = false;   // the one-lane-per-ray kernel's pixel
  if constexpr (Tracer<OPT>::kCoop) {
    // One call site for both launch forms.  Grid launch: this workgroup's block, once.
    // Persistent launch (A.queue): the wave pulls packets -- the 8x8-pixel unit a wave renders
    // -- from the launch's counter until none is left, as the reference's thread pool pulls
    // 64x64 tiles (common/thread_pool.h:146-161), each wave on its own (no workgroup
    // barrier: a wave whose packet finishes early takes the next one at once).  Every packet
    // renders exactly as in the grid launch (same block, wave, frame, seeds).  The next index
    // is fetched when a packet starts, so its round trip hides behind the packet's work.
    constexpr bool queued = (OPT & OPT_QUEUE) != 0;
    static_assert(!queued || (!split && (OPT & (OPT_STATS | OPT_TIMING)) == 0),
                  "persistent launches: 256-thread workgroups, no per-wave statistics");
    const uint32_t perFrame = (uint32_t)A.numTiles * 16u;  // blocks per frame
    const uint32_t blocksAll = perFrame * (uint32_t)A.numSamples;
    QueueCursor qc = {(int)(blockIdx.x & (kQueueXcds - 1)), 0u};  // workgroup b runs on XCD b % 8
    uint32_t p = queued ? queue_take(A.queue, blocksAll, qc) : 0u;
    bool more = !queued || p != 0xFFFFFFFFu;
    while (more) {
      uint32_t pblk = blk, nx = 0u;
      int pw = wwave + (tid >> 6), frame = (int)blockIdx.y;
      if constexpr (queued) {
        const uint32_t g = p >> 2;  // the packet's block over all frames
        frame = A.numSamples > 1 ? (int)(g / perFrame) : 0;
        pblk = g - (uint32_t)frame * perFrame;
        pw = (int)(p & 3u);
      }
      pblk = __builtin_amdgcn_readfirstlane(pblk);
      pw = __builtin_amdgcn_readfirstlane(pw);
      frame = __builtin_amdgcn_readfirstlane(frame);
      // the thread index, new to the compiler in every iteration: what derives from it (the
      // pixel's coordinates, LDS slot addresses) is recomputed per packet, not hoisted out of
      // the loop and held in VGPRs through it
      int ltid = tid;
      if constexpr (queued) {
        asm volatile("" : "+v"(ltid));
        // ... and so are the launch's arguments: the kernel-argument segment (RenderArgs is the
        // kernel's only argument, at offset 0) through a pointer the compiler cannot follow
        // across iterations.  Every value derived from them (the box's corners relative to
        // the eye, |eye|^2, cube-map and LUT scales, ...) is then computed per packet as in
        // the grid launch, instead of once before the loop and held in VGPRs (or scratch)
        // through every packet.
        typedef const __attribute__((address_space(4))) RenderArgs *KArgs;
        KArgs kp = (KArgs)__builtin_amdgcn_kernarg_segment_ptr();
        asm volatile("" : "+s"(kp));
        const RenderArgs &AL = *(const RenderArgs *)kp;
        Tracer<OPT> TL{{}, AL, s_logf, lean ? AL.sphBits : s_sph, s_cnt, {0, 0, 0, 0, 0, 0, 0}};
        TL.s_gbits = s_gbits;
        const Pixel ppx = pixel_of(AL, pblk, pw * 64 + (ltid & 63));
        launched += (uint32_t)__popcll(__ballot(ppx.active));
        render_pixel_coop<OPT>(AL, TL, ppx, lean ? AL.srgbTh : s_th, s_dda, s_entry, s_acc, s_coop[ltid >> 6],
                               &s_scan[Tracer<OPT>::kWaveScan ? ltid >> 6 : 0], s_jmp, ltid, AL.accumID + frame,
                               pblk, pw, frame);
        TL.flush_coop();  // this packet's counts (nothing carried from packet to packet)
      } else {
        const int pl = partSel & 255, pn = 64 >> pl;  // a split packet's part: pn rays
        Pixel ppx = pixel_of(A, pblk, pw * 64 + (partSel < 0 ? (ltid & 63) : ((partSel >> 8) * pn) | (ltid & (pn - 1))));
        if (partSel >= 0) ppx.active = ppx.active && (ltid & 63) < pn;
        if (splitAway || emptyItem) ppx.active = false;
        launched += (uint32_t)__popcll(__ballot(ppx.active));
        T.frame = frame;
        render_pixel_coop<OPT>(A, T, ppx, th_p, s_dda, s_entry, s_acc, s_coop[ltid >> 6],
                               &s_scan[Tracer<OPT>::kWaveScan ? ltid >> 6 : 0], s_jmp, ltid, cam_accum_id(A, frame),
                               pblk, pw, frame, partSel, interior);
        if (A.chain && frame < A.numSamples - 1 && frame != A.chainWithhold) {
          // chained frames: this wave's pixels are written through; tell frame + 1's wave
#ifdef IRT_PROBE_BUILD
          if (A.probeExit != 16)  // measurement only (16, probe build): the flag without the drain
#endif
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
          if (__lane_id() == 0)
            __hip_atomic_store(A.chainFlag + (size_t)pblk * 4u + (uint32_t)pw, A.chainEpoch + (uint32_t)frame + 1u,
                               __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
      }
      // the next packet once this one is done: a fetch issued at the packet's start (to
      // hide its round trip) made the packet's first gather wait for it as well (vector
      // memory counts retire in order) -- 0.32 ms per C3 frame against 0.09 (profiles/r04c/)
      if constexpr (queued) nx = queue_take(A.queue, blocksAll, qc);
      p = nx;
      more = queued && p != 0xFFFFFFFFu;
    }
    if constexpr (queued) queue_done(A.queue);
    T.flush_coop();
  }
  else {
    const Pixel px = pixel_of(A, blk, ptid);
    float4 *slot = A.numSamples > 1 ? A.sampleBuf + (size_t)blockIdx.y * gridDim.x * blockDim.x + blk * 256u + ptid
                                    : nullptr;
    if (px.active) render_pixel<OPT>(A, T, px, th_p, s_dda, s_entry, tid, A.accumID + (int)blockIdx.y, slot);
    pxActive = px.active;
    launched = (uint32_t)__popcll(__ballot(px.active));
  }
  if constexpr ((OPT & OPT_TIMING) != 0) {
    T.tmark(8);  // after the last woodcockFunc: pixel write, epilogue
    if ((tid & 63) == 0) {
      for (int k = 0; k < TimeAccOn::kTimeRegions; ++k)
        atomicAdd(&A.counters[5 + k], (unsigned long long)T.tAcc[k]);
      atomicAdd(&A.counters[14], (unsigned long long)(__builtin_amdgcn_s_memtime() - tStart));
      atomicAdd(&A.counters[15], 1ull);
    }
  }
  if constexpr ((OPT & OPT_STATS) != 0) {
    // Woodcock draws and zero-length sdda leaves: sums, per-wave maxima, draws histogram
    uint32_t ss = T.cnt.steps, sm = T.cnt.steps, ds = T.cnt.deg, dm = T.cnt.deg;
    for (int off = 32; off > 0; off >>= 1) {
      ss += __shfl_down(ss, off, 64);
      sm = max(sm, (uint32_t)__shfl_down(sm, off, 64));
      ds += __shfl_down(ds, off, 64);
      dm = max(dm, (uint32_t)__shfl_down(dm, off, 64));
    }
    const uint32_t d = T.cnt.steps;  // draws histogram: 0, 1-2, 3-5, > 5
    const int bkt = d == 0 ? 0 : (d <= 2 ? 1 : (d <= 5 ? 2 : 3));
    uint32_t hist[4];
    for (int k = 0; k < 4; ++k)
      hist[k] = T.kCoop ? Tracer<OPT>::wave_sum(T.cnt.candHist[k])
                        : (uint32_t)__popcll(__ballot(pxActive && bkt == k));
    if ((tid & 63) == 0) {
      atomicAdd(&A.counters[5], (unsigned long long)ss);
      atomicAdd(&A.counters[6], (unsigned long long)sm);
      atomicAdd(&A.counters[7], (unsigned long long)(T.kCoop ? T.cnt.hops : ds));       // uniform per wave
      atomicAdd(&A.counters[8], (unsigned long long)(T.kCoop ? T.cnt.locRounds : dm));  // likewise
      atomicMax(&A.counters[9], (unsigned long long)sm);
      atomicMax(&A.counters[10], (unsigned long long)dm);
      atomicAdd(&A.counters[11], (unsigned long long)T.cnt.rounds);  // uniform per wave
      for (int k = 0; k < 4; ++k)
        if (hist[k]) atomicAdd(&A.counters[12 + k], (unsigned long long)hist[k]);
    }
  }
  if (A.counters || A.schedCost || A.wgTrace) {
    const int lane = (int)__lane_id();
    if (A.counters && lane == 0 && launched) atomicAdd(&s_cnt[0], launched);  // rays launched, once per wave
    // The last wave of the workgroup to get here writes the workgroup's counts and duration.
    // No end-of-workgroup barrier: a wave that finishes early frees its slot at once instead
    // of waiting for the slowest wave of its workgroup.  The acq-rel LDS add orders every
    // wave's count adds before the last wave's reads.
    uint32_t prev = 0;
    if (lane == 0)
      prev = __hip_atomic_fetch_add(&s_done, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_WORKGROUP);
    prev = (uint32_t)__shfl((int)prev, 0, 64);
    if (prev == (blockDim.x >> 6) - 1u) {
      if (A.counters) flush_counters(A, s_cnt, lane);
      if (A.schedCost && lane == 0 && (wavewg || wwave == 0) && !splitAway && !emptyItem) {  // this workgroup's duration, for the next launches' order
        // per packet (4 per block; a 256-thread workgroup's in its first packet's slot), a split
        // packet's part counted for the whole packet (parts x its duration)
        uint64_t dt = wall_clock64() - c0;
        if (partSel >= 0) dt <<= (partSel & 255);
        A.schedCost[pkt] = dt > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)dt;
      }
      if (A.wgTrace && lane == 0)
        A.wgTrace[4 * (blockIdx.y * gridDim.x + blockIdx.x) + 1] = (uint32_t)__builtin_amdgcn_s_memrealtime();
    }
  }
}

// ------------------------------------------------------------------ progressive batch
// The lerp chain of K consecutive frames (deviceCode.cu:333-334, accumID..accumID+K-1) over
// the per-frame samples k_render stored, in frame order: bit-identical to K launches.
// Frames whose ray missed the box leave the pixel untouched (kNoSample), as the
// reference's raygen returns before writing (294-295); fb is written after the last frame.
__global__ void __launch_bounds__(256) k_accumulate(RenderArgs A) {
  __shared__ float s_th[256];
  s_th[threadIdx.x] = A.srgbTh[threadIdx.x];
  __syncthreads();
  const uint32_t gid = blockIdx.x * 256u + threadIdx.x;
  const Pixel px = pixel_of(A, blockIdx.x, (int)threadIdx.x);
  if (!px.active) return;
  const size_t lanes = (size_t)gridDim.x * 256u;
  float4 a = A.accum[px.outIdx];
  bool wrote = false;
  for (int k = 0; k < A.numSamples; ++k) {
    const float4 c = A.sampleBuf[(size_t)k * lanes + gid];
    if (c.w == kNoSample) continue;
    const float w = 1.f / (float)(A.accumID + k + 1);
    a.x = w * c.x + (1.f - w) * a.x;
    a.y = w * c.y + (1.f - w) * a.y;
    a.z = w * c.z + (1.f - w) * a.z;
    a.w = w * c.w + (1.f - w) * a.w;
    wrote = true;
  }
  if (!wrote) return;
  A.accum[px.outIdx] = a;
  A.fb[px.outIdx] = srgb_byte(s_th, a.x) + (srgb_byte(s_th, a.y) << 8) +
                    (srgb_byte(s_th, a.z) << 16) + (make_8bit(a.w) << 24);
}

// ------------------------------------------------------------------ debug: point location
// The default kernel's Tracer::locate (sampleVolume over the binned lists) on given points:
// the device locator pinned point by point (tests/test_gpu_parity.py), e.g. exactly on
// radial bin edges, which frames almost never hit.
__global__ void __launch_bounds__(256) k_debug_locate(RenderArgs A, const float *xyz, int n,
                                                      int *found, float *value) {
  __shared__ uint32_t s_sph[kSphBitWords];
  __shared__ uint32_t s_cnt[kCnt];
  for (int i = threadIdx.x; i < kSphBitWords; i += 256) s_sph[i] = A.numSph ? A.sphBits[i] : 0u;
  if (threadIdx.x < kCnt) s_cnt[threadIdx.x] = 0;
  __syncthreads();
  Tracer<kDefaultVariant & ~OPT_MONO> T{{}, A, nullptr, s_sph, s_cnt, {0, 0, 0, 0, 0, 0, 0}};
  const int j = (int)(blockIdx.x * 256 + threadIdx.x);
  if (j < n) {
    float v = 0.f;
    found[j] = T.locate(xyz[3 * j], xyz[3 * j + 1], xyz[3 * j + 2], v) ? 1 : 0;
    value[j] = v;
  }
}

// The same points through the cooperative kernel's wave-wide candidate scan
// (Tracer::locate_wave; every lane of a wave calls it, lanes past n with want = false):
// pins its dealt-out candidates and its second pass on radial bin edges to the serial path.
template <int O>
__global__ void __launch_bounds__(256) k_debug_locate_wave(RenderArgs A, const float *xyz, int n,
                                                           int *found, float *value) {
  __shared__ uint32_t s_sph[kSphBitWords];
  __shared__ uint32_t s_cnt[kCnt];
  __shared__ CoopWave s_coop[4];
  __shared__ ScanWave s_scan[4];
  for (int i = threadIdx.x; i < kSphBitWords; i += 256) s_sph[i] = A.numSph ? A.sphBits[i] : 0u;
  if (threadIdx.x < kCnt) s_cnt[threadIdx.x] = 0;
  __syncthreads();
  Tracer<O> T{{}, A, nullptr, s_sph, s_cnt, {0, 0, 0, 0, 0, 0, 0}};
  static_assert(Tracer<O>::kWaveScan, "the default kernel scans wave-wide");
  const int j = (int)(blockIdx.x * 256 + threadIdx.x);
  const bool want = j < n;
  float x = 0.f, y = 0.f, z = 0.f;
  if (want) {
    x = xyz[3 * j];
    y = xyz[3 * j + 1];
    z = xyz[3 * j + 2];
  }
  float v = 0.f;
  const bool f = T.locate_wave(want, x, y, z, v, s_coop[threadIdx.x >> 6], s_scan[threadIdx.x >> 6]);
  if (want) {
    found[j] = f ? 1 : 0;
    value[j] = v;
  }
}

void launch_debug_locate(const RenderArgs &A, const float *xyz, int n, int *found, float *value,
                         hipStream_t s, bool wave) {
  if (n <= 0) return;
  constexpr int D = kDefaultVariant & ~OPT_MONO;
  if (wave && A.slots)  // the scan from the slot table (OPT_SLOT), as the scene's launches run it
    hipLaunchKernelGGL(k_debug_locate_wave<D | OPT_SLOT>, dim3((n + 255) / 256), dim3(256), 0, s, A, xyz, n, found, value);
  else if (wave)
    hipLaunchKernelGGL(k_debug_locate_wave<D>, dim3((n + 255) / 256), dim3(256), 0, s, A, xyz, n, found, value);
  else
    hipLaunchKernelGGL(k_debug_locate, dim3((n + 255) / 256), dim3(256), 0, s, A, xyz, n, found, value);
}

// The unstructured samplers' point location (Tracer::locate_wedge for IRT_MODE_CUBQL,
// Tracer::locate_tri for IRT_MODE_TRIANGLES, chosen by A.sampler) on given points, through the
// Tracer instantiation of their sphere-accel launches (VariantForms::wedge, kSamplerVariant): the
// frames' own code on records and points a frame almost never samples
// (tests/test_gpu_samplers.py).
__global__ void __launch_bounds__(256) k_debug_locate_sampler(RenderArgs A, const float *xyz, int n,
                                                              int *found, float *value) {
  __shared__ uint32_t s_cnt[kCnt];
  if (threadIdx.x < kCnt) s_cnt[threadIdx.x] = 0;
  __syncthreads();
  Tracer<kSamplerVariant> T{{}, A, nullptr, nullptr, s_cnt, {0, 0, 0, 0, 0, 0, 0}};
  const int j = (int)(blockIdx.x * 256 + threadIdx.x);
  if (j < n) {
    float v = 0.f;
    const bool f = T.locate(xyz[3 * j], xyz[3 * j + 1], xyz[3 * j + 2], v);
    found[j] = f ? 1 : 0;
    value[j] = f ? v : 0.f;
  }
}

void launch_debug_locate_sampler(const RenderArgs &A, const float *xyz, int n, int *found, float *value,
                                 hipStream_t s) {
  if (n <= 0) return;
  hipLaunchKernelGGL(k_debug_locate_sampler, dim3((n + 255) / 256), dim3(256), 0, s, A, xyz, n, found, value);
}

// ------------------------------------------------------------------ variants / launcher
// Variant numbers: irt_kernels.h OPT_* (the numbering is explained there).
static_assert((kDefaultVariant & OPT_MONO) != 0, "variant numbering");

// A launch's kernel and grid are one value, RenderPlan, computed in one function, plan_render, from
// the launch's arguments and its variant's row of the table below; everything else reads it: the
// launch itself, the count ring's size, the debug hooks.  The table has one VariantForms per listed
// variant, filled by make_forms<N>: the k_render instantiation of each form a launch of variant N
// can take, null where N has none.  Which forms exist is decided there and nowhere else -- what
// irt_launch.hip may put into RenderArgs (render_split_ok & co., irt_kernels.h), what
// prewarm_render launches and what render_queue_wgs measures are reads of the table.  A new form
// is a new member, its line in make_forms and its test in plan_render.
//
// The product build lists the default (one-wave workgroups) with its two scene forms, 5376
// (four-wave workgroups) and the statistics variant (IRT_COUNTERS, profiles/wave_stats.py).  The
// A/B variants are built only by `make VARIANTS=all` (libicon_rt_hip_all.so, loaded through
// IRT_LIB_PATH by the profiles/ tools and by tests/test_gpu_parity.py when present), one line per
// family, in the order they were added:
//   four-wave workgroups, full LDS: no waves-per-SIMD floor, 4 and 5 waves, statistics, OPT_SERIAL,
//     OPT_SCAN1, OPT_TIMING (all but the first three at 4 waves);
//   OPT_LEAN at 4 and 5 waves, | OPT_WAVEWG at 4 and 5, OPT_TIMING at 5 waves, OPT_LEAN at 6,
//     OPT_FASTSPH on 5376 and on 6296832, OPT_WAVEWG at 6 waves, 6296832 | OPT_NOMISS;
//   | OPT_DMATAB and its hole-free form; | OPT_DPPSCAN: the default and its hole-free form, each
//     again with OPT_TIMING;
//   the default | OPT_NOHOLESKIP, | OPT_NOVOIDRUN, | OPT_VOIDLOC (the form for scenes with holes);
//   OPT_FASTSPH on the hole-free form and on the default; OPT_STATS on the default and its
//     hole-free form.
#ifdef IRT_ALL_VARIANTS
#define IRT_VARIANTS(X)                                                                  \
  X(4096) X(5120) X(5376) X(36864) X(70656) X(136192) X(529408)                          \
  X(2102272) X(2102528) X(6296576) X(6296832) X(529664) X(2102784) X(33559808)           \
  X(39851264) X(6297088) X(6558976)                                                      \
  X(73405696) X(73667840) X(73405728) X(73667872) X(73930016) X(74192160)                \
  X(73405732) X(73405730) X(1147147552)                                                  \
  X(107222304) X(106960160) X(73438496) X(73700640)
#else
#define IRT_VARIANTS(X) X(73405728) X(73667872) X(1147147552) X(5376) X(36864)
#endif
static_assert(kDefaultVariant == 73405728 && (kDefaultVariant | kNoMissBit) == 73667872 && kNoMissBit == OPT_NOMISS &&
                  (kDefaultVariant | kVoidLocBit) == 1147147552 && kVoidLocBit == OPT_VOIDLOC,
              "the product build's variant list names the default and its scene forms (scene_variant)");

// k_render<ID> as a launch form: one-wave workgroups (OPT_WAVEWG) run four per 256-pixel block
template <int ID>
constexpr KernelForm form() {
  return {k_render<ID>, ID, (ID & OPT_WAVEWG) ? 64 : 256};
}

// The forms of variant N.  The grid accel and the unstructured samplers: their own instantiations
// of the raygen (kept out of the default kernel, whose registers they would cost); the wedge
// kernels hold a 6-vertex Newton state: no waves-per-SIMD floor.  Both run the cooperative
// Woodcock loop with its miss mode (C2: TRIANGLES 3.4x, CUBQL 2.5x faster than one lane per ray;
// profiles/r02b_investigation/).
template <int N>
constexpr VariantForms make_forms() {
  constexpr int K = N & ~OPT_MONO;
  constexpr int D = kDefaultVariant & ~OPT_MONO;
  constexpr int DB = D & ~(0xF00 | OPT_WAVEWG | OPT_LEAN);  // 256-thread workgroups, full LDS
  constexpr int DW = DB | OPT_WEDGE | (K & OPT_SERIAL);
  static_assert(DW == (kSamplerVariant | (K & OPT_SERIAL)), "k_debug_locate_sampler runs the samplers' Tracer");
  constexpr int DG = DB | 0x400;  // the grid-accel raygen: 4 waves/SIMD as measured in round 2
  VariantForms f = {};
  f.variant = N;
  f.plain = form<K>();
  f.wedgeGrid = form<DW | OPT_GRID>();  // CUBQL / TRIANGLES
  f.wedge = form<DW>();
  f.grid = form<DG | OPT_GRID | (K & OPT_SERIAL)>();
  // Persistent launches (OPT_QUEUE, 3-4x slower: DESIGN.md section 5) are compiled into the A/B
  // library only (make VARIANTS=all); the product library has no persistent kernel.
#ifdef IRT_ALL_VARIANTS
  constexpr int kNoQueue = OPT_WAVEWG | OPT_SERIAL | OPT_STATS | OPT_TIMING;  // bits without a persistent form
  if constexpr ((K & kNoQueue) == 0) f.queue = form<K | OPT_QUEUE>();
#endif
  // The default and its two scene forms: a single frame with measured-cost work items runs their
  // split-capable form, a scene with a slot table their OPT_SLOT form, ...
  if constexpr (K == D || K == (D | kNoMissBit) || K == (D | kVoidLocBit)) {
    f.split = form<K | OPT_SPLIT>();
    f.slot = form<K | OPT_SLOT>();
    f.slotSplit = form<K | OPT_SPLIT | OPT_SLOT>();
    // ... and chained progressive frames with void packets the OPT_VOID form, which has no OPT_SLOT
    // or OPT_SPLIT sibling (render_void_ok): the bitmap on the plain grid, and for the flat kernel
    // the work-item list (k_render: the terrain kernels' list form needs scratch)
    f.voidBits = form<K | OPT_VOID>();
    if constexpr (K == (D | kNoMissBit)) f.voidList = form<K | OPT_VOID | OPT_VLIST>();
  }
  return f;
}

constexpr VariantForms kForms[] = {
#define IRT_FORMS(N) make_forms<N>(),
    IRT_VARIANTS(IRT_FORMS)
#undef IRT_FORMS
};

const VariantForms *forms_of(int variant) {
  for (const VariantForms &f : kForms)
    if (f.variant == variant) return &f;
  return nullptr;
}

int render_variants(int *out, int cap) {
  int n = 0;
  for (const VariantForms &f : kForms) {
    if (n < cap && out) out[n] = f.variant;
    ++n;
  }
  return n;
}

bool render_queue_compiled() {
  for (const VariantForms &f : kForms)
    if (f.queue.fn) return true;
  return false;
}

// The precedence: the samplers, the grid accelerator, then the sphere path's forms -- queue, void
// list, void bitmap, slot table, work items -- each only where the variant has it.  The grid follows
// from the form chosen, never from the arguments alone.
RenderPlan plan_render(const VariantForms &F, const RenderArgs &A, int queueWG) {
  const bool g = A.accelMode == IRT_ACCEL_GRID;
  const KernelForm *k = &F.plain;
  if (A.sampler != IRT_MODE_USER_GEOM) k = g ? &F.wedgeGrid : &F.wedge;
  else if (g) k = &F.grid;
  else if (A.queue && F.queue.fn) k = &F.queue;
  else if (A.voidList && F.voidList.fn) k = &F.voidList;
  else if (A.voidBits && F.voidBits.fn) k = &F.voidBits;
  else if (A.slots && F.slot.fn) k = A.numSplit ? &F.slotSplit : &F.slot;
  else if (A.numSplit && F.split.fn) k = &F.split;
  RenderPlan P;
  P.form = *k;
  P.accumBlocks = A.numTiles * 16;
  if (k == &F.queue)  // persistent: the resident workgroups pull the packets
    P.grid = dim3((uint32_t)queueWG, 1);
  else if (k == &F.voidList)  // rows of live and void work items, one row per frame
    P.grid = dim3(A.voidLive + A.voidRow, (uint32_t)A.numSamples);
  else  // the frame's blocks, behind the listed work items (A.numSplit), per frame
    P.grid = dim3((uint32_t)(P.accumBlocks * (256 / k->threads)) + A.numSplit, (uint32_t)A.numSamples);
  P.workgroups = (size_t)P.grid.x * P.grid.y;
  return P;
}

void launch_render(const RenderArgs &A, const RenderPlan &P, hipStream_t s) {
  hipLaunchKernelGGL(P.form.fn, P.grid, dim3(P.form.threads), 0, s, A);
  // progressive batch: the lerp chain over the frames' samples (chained frames lerp in k_render)
  if (A.numSamples > 1 && !A.chain) hipLaunchKernelGGL(k_accumulate, dim3(P.accumBlocks), dim3(256), 0, s, A);
}

int render_queue_wgs(const VariantForms &F, int numCU, int numBlocks) {
  int occ = 0;
  if (!F.queue.fn || hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, F.queue.fn, F.queue.threads, 0) != hipSuccess ||
      occ < 1) {
    (void)hipGetLastError();
    occ = 1;
  }
  const long long n = (long long)occ * numCU;
  return (int)(n < numBlocks ? n : numBlocks);
}

// The first launch of a kernel pays the HIP runtime's lazy per-kernel setup on the host
// (~0.6 ms between the launch's start event and the dispatch, against a ~0.1 ms frame): a
// one-workgroup launch that returns at once (probeExit 1) at context creation takes it there,
// for every form of the sphere path (the grid accelerator's and the samplers' kernels pay it in
// their first frame).
void prewarm_render(const VariantForms &F, hipStream_t s) {
  RenderArgs A = {};
  A.probeExit = 1;
  A.numSamples = 1;
  for (const KernelForm *k : {&F.plain, &F.split, &F.slotSplit, &F.slot, &F.voidList, &F.voidBits, &F.queue})
    if (k->fn) hipLaunchKernelGGL(k->fn, dim3(1), dim3(k->threads), 0, s, A);
}

}  // namespace irt

