// irt_sched.cpp -- measured-cost scheduling, the pure part: one order buffer's words from a
// launch's measured packet costs (csrc/irt_launch.hip sched_prepare uploads them).

#include <string.h>

#include <algorithm>
#include <utility>
#include <vector>

#include "irt_internal.h"

namespace irt {

uint32_t sched_order(const uint32_t *cost, int numBlocks, int tilesX, int tileStride, int policy,
                     int splitLg, float splitFactor, int numCU, bool wavewg, size_t cap,
                     uint32_t maxSplit, uint32_t *out) {
  // longest-processing-time first over whole 64x64 tiles (16 consecutive workgroups, kept
  // together for the locator's cache locality)
  const int nt = numBlocks / 16;
  // group size in tiles: 1, or a band of consecutive launch tiles (one image row of tiles)
  const int band = policy == 2 ? std::max(1, tilesX / std::max(1, tileStride)) : 1;
  const int ng = (nt + band - 1) / band;
  std::vector<std::pair<uint64_t, int>> groups(ng);
  for (int g = 0; g < ng; ++g) {
    uint64_t sum = 0;
    for (int t = g * band; t < std::min(nt, (g + 1) * band); ++t)
      for (int j = 0; j < 64; ++j) sum += cost[64 * t + j];
    groups[g] = {policy == 3 ? (uint64_t)g : sum, g};
  }
  std::stable_sort(groups.begin(), groups.end(),
                   [](const std::pair<uint64_t, int> &a, const std::pair<uint64_t, int> &b) {
                     return a.first > b.first;
                   });
  int p = 0;
  for (const auto &g : groups)
    for (int t = g.second * band; t < std::min(nt, (g.second + 1) * band); ++t, ++p)
      for (int j = 0; j < 16; ++j) out[16 * p + j] = (uint32_t)(16 * t + j);
  // Work items ahead of the regular order (one-wave workgroups only), costliest first: every
  // packet whose measured duration exceeds splitFactor x the frame's ideal span (all packets'
  // durations over the resident slots), in 2^splitLg parts of 64 >> splitLg rays -- such a packet
  // would end the frame after the rest, and it is lane-bound: its parts take about 1/2^splitLg of
  // its time. (Packets shorter than the span are better left whole and in place: listing them
  // first, whole, or splitting them cost C3 +16 to +27 %, profiles/r05s_split/.) A packet's parts
  // are 8 items apart, so they run on one XCD; at most a tenth of the packets, maxSplit items.
  uint32_t *list = out + cap, *mask = list + maxSplit;
  memset(mask, 0, (4 * cap + 31) / 32 * sizeof(uint32_t));
  uint32_t ns = 0;
  // (a work item holds the packet index in 24 bits: no splits past 2^24 packets)
  if (splitLg > 0 && splitFactor > 0.f && wavewg && 4 * (size_t)numBlocks < ((size_t)1 << 24)) {
    const size_t np = 4 * (size_t)numBlocks;
    double total = 0.0;
    for (size_t k = 0; k < np; ++k) total += cost[k];
    const double span = total / (double)std::max(1, 20 * numCU);  // 5 waves x 4 SIMDs per CU
    const size_t most = np / 10;
    std::vector<uint32_t> byCost(np);
    for (size_t k = 0; k < np; ++k) byCost[k] = (uint32_t)k;
    std::partial_sort(byCost.begin(), byCost.begin() + std::min(most, np), byCost.end(),
                      [&](uint32_t a, uint32_t b) { return cost[a] > cost[b] || (cost[a] == cost[b] && a < b); });
    const uint32_t parts = 1u << splitLg;
    std::vector<uint32_t> heavy;
    for (size_t k = 0; k < most && (heavy.size() + 8) * parts <= maxSplit; ++k) {
      const double v = (double)cost[byCost[k]];
      if (!(v > splitFactor * span) || v <= 0.0) break;
      heavy.push_back(byCost[k]);
    }
    while (heavy.size() % 8) heavy.push_back(~0u);  // empty packets: their parts render nothing
    for (size_t g = 0; g < heavy.size(); g += 8)
      for (uint32_t part = 0; part < parts; ++part)
        for (size_t j = 0; j < 8; ++j)
          list[ns++] = heavy[g + j] == ~0u ? ~0u : (heavy[g + j] << 8) | (part << 4) | (uint32_t)splitLg;
    while (ns % 8) list[ns++] = ~0u;
    for (size_t k = 0; k < ns; ++k)
      if (list[k] != ~0u) mask[(list[k] >> 8) >> 5] |= 1u << ((list[k] >> 8) & 31);
  }
  return ns;
}

}  // namespace irt
