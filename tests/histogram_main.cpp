// A stand-alone check of host/irt_histogram.cpp (irt_histogram_cells, the histogram's definition on
// the host, and the argument check it shares with irt_histogram), built by tests/test_histogram_cpu.py
// with -fsanitize=address,undefined and run there: every input and output array is a heap block of
// exactly the size the call may touch, so a read or write past it is the sanitizer's to report.
// Exit status 0: every check passed.
#include <math.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "irt_internal.h"

static int g_errors = 0;  // set_error calls seen

namespace irt {
void set_error(const char *fmt, ...) {
  (void)fmt;
  ++g_errors;
}
}  // namespace irt

static int fail(const char *what, int n) {
  fprintf(stderr, "histogram_main: %s (n = %d)\n", what, n);
  return 1;
}

struct Out {
  std::vector<uint64_t> bins, tails, outside;
  Out(int bands, int nbins, uint64_t fill) : bins((size_t)bands * nbins, fill), tails((size_t)bands * 3, fill), outside(1, fill) {}
  irt_histogram_out all() { return {bins.data(), tails.data(), outside.data()}; }
};

// the definition once more, item by item, the band by a linear search
static int check(const std::vector<irt_icon_cell> &cells, irt_box1f vr, int nbins, int weighting,
                 const std::vector<float> *edges) {
  const int bands = edges ? (int)edges->size() - 1 : 1;
  Out o(bands, nbins, 0xA5A5A5A5ull), want(bands, nbins, 0);
  if (irt_histogram_cells(cells.data(), cells.size(), vr, nbins, weighting, edges ? edges->data() : nullptr, bands,
                          o.all()) != IRT_OK)
    return fail("refused", nbins);
  for (const irt_icon_cell &c : cells)
    for (int l = 0; l < c.numLayers; ++l) {
      const float v = c.value[l], h0 = c.height[l], h1 = c.height[l + 1];
      uint64_t w = 1;
      if (weighting == IRT_HIST_THICKNESS) {
        const float d = h1 - h0;
        w = d > 0.f && d <= 1048576.0f ? (uint64_t)(d * 64.0f) : 0;
      }
      if (!w) continue;
      int b = 0;
      if (edges) {
        const float m = (h0 + h1) * 0.5f;
        b = -1;
        for (int k = 0; k < bands; ++k)
          if ((*edges)[k] <= m && m < (*edges)[k + 1]) b = k;
        if (b < 0) {
          want.outside[0] += w;
          continue;
        }
      }
      const float t = (v - vr.lower) / (vr.upper - vr.lower);
      if (!isfinite(v) || isnan(t))
        want.tails[3 * b + 2] += w;
      else if (t < 0.f)
        want.tails[3 * b] += w;
      else if (t > 1.f)
        want.tails[3 * b + 1] += w;
      else {
        int k = (int)(t * (float)nbins);
        if (k > nbins - 1) k = nbins - 1;
        want.bins[(size_t)b * nbins + k] += w;
      }
    }
  if (o.bins != want.bins || o.tails != want.tails || o.outside != want.outside) return fail("bins, tails or outside", nbins);
  // each output alone (the others NULL) is the same output, written over what the buffer held
  Out one(bands, nbins, 7);
  irt_histogram_out only = {nullptr, one.tails.data(), nullptr};
  if (irt_histogram_cells(cells.data(), cells.size(), vr, nbins, weighting, edges ? edges->data() : nullptr, bands,
                          only) != IRT_OK || one.tails != o.tails)
    return fail("tails alone", nbins);
  only = {one.bins.data(), nullptr, nullptr};
  if (irt_histogram_cells(cells.data(), cells.size(), vr, nbins, weighting, edges ? edges->data() : nullptr, bands,
                          only) != IRT_OK || one.bins != o.bins || one.outside[0] != 7)
    return fail("bins alone", nbins);
  return 0;
}

int main() {
  uint32_t s = 97531u;
  auto rnd = [&]() {
    s = s * 1664525u + 1013904223u;
    return (float)(s >> 8) * (1.f / 16777216.f);
  };
  const float special[] = {0.25f, 0.75f, -0.f, NAN, INFINITY, -INFINITY, 0.24999f, 0.75001f, 3e38f, -3e38f};
  const size_t counts[] = {0, 1, 5, 64, 257};
  const int binCounts[] = {1, 2, 7, 300, 4096};
  for (size_t n : counts) {
    std::vector<irt_icon_cell> cells(n);
    for (size_t i = 0; i < n; ++i) {
      irt_icon_cell &c = cells[i];
      memset(&c, 0, sizeof(c));
      c.numLayers = i == 0 ? 31 : (i == 1 ? 0 : (int)(rnd() * 32.f));
      if (c.numLayers > 31) c.numLayers = 31;
      float h = 6.371e6f + floorf(rnd() * 2000.f) * 0.5f;
      for (int j = 0; j < 32; ++j) {
        c.height[j] = h;
        const float r = rnd();
        h += r < 0.1f ? 0.f : (r < 0.2f ? -250.f : floorf(rnd() * 4000.f) * 0.5f);  // zero and inverted layers too
        c.value[j] = rnd() < 0.25f ? special[(int)(rnd() * 10.f) % 10] : rnd() * 1.5f - 0.25f;
      }
      if (i == 3) c.height[5] = 3e38f, c.height[6] = -3e38f;  // a thickness that overflows, and a mid-height of 0
    }
    std::vector<float> three = {6.3710e6f, 6.3752255e6f, 6.3752260e6f, 6.39e6f};
    std::vector<float> many(65);
    for (int k = 0; k <= 64; ++k) many[k] = 6.37e6f + 1500.f * (float)k;
    const irt_box1f vr = {0.25f, 0.75f}, wide = {-3e38f, 3e38f};  // (upper - lower overflows: t = 0 or NaN)
    for (int nb : binCounts)
      for (int weighting = 0; weighting <= 1; ++weighting) {
        if (check(cells, vr, nb, weighting, nullptr) || check(cells, wide, nb, weighting, nullptr)) return 1;
        if (nb <= 1365 && check(cells, vr, nb, weighting, &three)) return 1;
        if (nb <= 64 && check(cells, vr, nb, weighting, &many)) return 1;
      }
  }
  // the refusals
  std::vector<irt_icon_cell> cells(4);
  memset(cells.data(), 0, cells.size() * sizeof(irt_icon_cell));
  Out o(64, 64, 9);
  const irt_box1f vr = {0.f, 1.f};
  std::vector<float> e = {1.f, 2.f, 3.f, 4.f}, bad;
  int refused = 0, tried = 0;
  g_errors = 0;
  auto inval = [&](int rc) {
    ++tried;
    refused += rc == IRT_E_INVALID;
  };
  inval(irt_histogram_cells(cells.data(), 4, vr, 0, 0, nullptr, 1, o.all()));
  inval(irt_histogram_cells(cells.data(), 4, vr, 4097, 0, nullptr, 1, o.all()));
  inval(irt_histogram_cells(cells.data(), 4, vr, 7, 0, e.data(), 0, o.all()));
  inval(irt_histogram_cells(cells.data(), 4, vr, 7, 0, e.data(), 65, o.all()));
  inval(irt_histogram_cells(cells.data(), 4, vr, 2048, 0, e.data(), 3, o.all()));
  inval(irt_histogram_cells(cells.data(), 4, {1.f, 1.f}, 7, 0, nullptr, 1, o.all()));
  inval(irt_histogram_cells(cells.data(), 4, {0.f, NAN}, 7, 0, nullptr, 1, o.all()));
  inval(irt_histogram_cells(cells.data(), 4, {-INFINITY, 0.f}, 7, 0, nullptr, 1, o.all()));
  inval(irt_histogram_cells(cells.data(), 4, vr, 7, 2, nullptr, 1, o.all()));
  inval(irt_histogram_cells(cells.data(), 4, vr, 7, -1, nullptr, 1, o.all()));
  inval(irt_histogram_cells(cells.data(), 4, vr, 7, 0, nullptr, 2, o.all()));
  bad = {1.f, 2.f, 2.f, 4.f};
  inval(irt_histogram_cells(cells.data(), 4, vr, 7, 0, bad.data(), 3, o.all()));
  bad = {1.f, 2.f, 3.f, NAN};
  inval(irt_histogram_cells(cells.data(), 4, vr, 7, 0, bad.data(), 3, o.all()));
  bad = {-INFINITY, 2.f, 3.f, 4.f};
  inval(irt_histogram_cells(cells.data(), 4, vr, 7, 0, bad.data(), 3, o.all()));
  inval(irt_histogram_cells(nullptr, 4, vr, 7, 0, nullptr, 1, o.all()));
  if (refused != tried || g_errors != tried) return fail("a bad argument was accepted, or refused without a message", refused);
  cells[2].numLayers = 32;
  if (irt_histogram_cells(cells.data(), 4, vr, 7, 0, nullptr, 1, o.all()) != IRT_E_DATA) return fail("numLayers 32 accepted", 32);
  cells[2].numLayers = -1;
  if (irt_histogram_cells(cells.data(), 4, vr, 7, 0, nullptr, 1, o.all()) != IRT_E_DATA) return fail("numLayers -1 accepted", -1);
  for (uint64_t x : o.bins)
    if (x != 9) return fail("a refused call wrote", 0);
  if (o.tails[0] != 9 || o.outside[0] != 9) return fail("a refused call wrote", 1);
  // no records: nothing is read, NULL included, the outputs zeroed; no outputs: nothing is written
  if (irt_histogram_cells(nullptr, 0, vr, 64, 0, nullptr, 1, o.all()) != IRT_OK || o.bins[63] != 0 || o.bins[64] != 9 ||
      o.tails[2] != 0 || o.tails[3] != 9 || o.outside[0] != 0)
    return fail("no records", 0);
  cells[2].numLayers = 3;
  const irt_histogram_out none = {nullptr, nullptr, nullptr};
  if (irt_histogram_cells(cells.data(), 4, vr, 7, 0, nullptr, 1, none) != IRT_OK) return fail("no outputs refused", 4);
  printf("histogram_main: ok\n");
  return 0;
}
