// icon_rt_main.cpp -- the icon_rt application on the MI355X backend: mirrors
// icon_rt/hostCode.cu main() (703-968) step by step, with the launch going through the C
// ABI of include/icon_rt_hip.h.
//
//   icon_rt <file.ic> [--num-cells N] [--lat-range a:b] [--lon-range a:b]
//           [-mode 0|1|2]                       (0 cell sample(), 1 triangles, 2 wedges)
//           [Pipeline flags: --size W H, --camera ..., -fovy f, --xf f, --sample-limit N]
//           [--synth rootN bisections levels]   (no .ic file: synthetic ICON grid)
//           [--bench K]                         (render K extra frames, print timing)
//           [--frames-per-launch B]             (--bench: B consecutive progressive frames
//                                                per launch, irt_render_accumulate)
//           [--true-size]                       (dir_du/dir_dv over the real W/H instead
//                                                of the reference's hard-coded 512)
//           [--accel sphere|grid]               (the "Accel mode" UI option,
//                                                hostCode.cu:853-857, 170-199)
//           [--gpus N]                          (N devices in this process: the frame's
//                                                64x64 tiles dealt over them, RCCL gather
//                                                to device 0; include/icon_rt_hip_multi.h)
//           [--dump-fb file]                    (the final RGBA8 framebuffer, raw W*H u32)
//           [--levels r0,r1,...]                (the field on the spheres of these radii, metres
//                                                from the centre, in place of the volume:
//                                                irt_render_levels; one device)
//           [--levels-back]                     (... with the far sides of spheres the camera
//                                                is outside of, IRT_LEVELS_BACK)
//           [--section lat0,lon0,lat1,lon1,n --section-levels r0,r1,...]
//                                               (the vertical cross-section along the great circle
//                                                between two points, degrees, on n columns and the
//                                                levels of these radii, metres from the centre, in
//                                                place of the frame: irt_section; one device; the
//                                                curtain goes to icon_rt_section.png, the last level
//                                                in the top row, and raw to --dump-fb, row k = level k)
//           [--histogram N [--histogram-thickness] [--histogram-bands r0,r1,...]]
//                                               (the distribution of the field's values over the
//                                                transfer function's value range in N bins, in place
//                                                of the frame: irt_histogram; one device; counted per
//                                                layer or, --histogram-thickness, weighted by the layer's
//                                                thickness in 1/64 m; per altitude band between the
//                                                ascending radii of --histogram-bands.  One line per
//                                                band on stdout: the N counts, then the tails)
//           [--graticule latStepDeg,lonStepDeg] [--lines FILE] [--line-width PX] [--lines-over]
//                                               (lines on the globe, drawn into the frame the app writes,
//                                                whichever render call made it: irt_render_overlay on the
//                                                sphere of the shell's lower radius; one device.  FILE is
//                                                text, one "lat lon" pair in degrees per line, a blank line
//                                                between polylines, # starts a comment -- e.g. a coastline
//                                                a user exports from Natural Earth; none is shipped.  Lines
//                                                are PX pixels wide at the sub-camera point (default 1.5),
//                                                under the volume or, --lines-over, on top of it)
//           [--contour R:c0,c1,... [--contour-grid NLAT,NLON]]
//                                               (isolines of the field at radius R, metres from the
//                                                centre, at the values c0, c1, ... (at most 16):
//                                                irt_contour_latlon on a wrapped NLAT x NLON grid, pole to
//                                                pole -- 361,720 by default, half a degree -- drawn through
//                                                the same overlay, after the --graticule and --lines
//                                                segments, --line-width wide.  The overlay then lies on the
//                                                sphere of radius R, the level surface of --levels R)

#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <fstream>
#include <string>
#include <vector>

#include <hip/hip_runtime_api.h>

#include "icon_rt_hip.h"
#include "icon_rt_hip_multi.h"
#include "pipeline.h"

using namespace irt_host;

namespace {

struct AppState {  // hostCode.cu:65-92 (the parts this backend uses)
  std::string filepath;
  long maxNumCells = -1;
  irt_box1f latRange{-INFINITY, INFINITY};
  irt_box1f lonRange{-INFINITY, INFINITY};
  int synth[3] = {0, 0, 0};
  int benchFrames = 0;
  int framesPerLaunch = 1;
  bool trueSize = false;
  int accelMode = IRT_ACCEL_SPHERE;  // g_appState.accelMode (hostCode.cu:75)
  int mode = IRT_MODE_USER_GEOM;     // g_appState.mode: the sampler (Params.h:29-31)
  int gpus = 0;                      // > 0: the multi-GPU split over devices 0..gpus-1
  std::string dumpFb;
  std::vector<float> levels;         // --levels: irt_render_levels in place of irt_render
  bool levelsBack = false;
  std::vector<float> section;        // --section: lat0, lon0, lat1, lon1 (degrees), n
  std::vector<float> sectionLevels;  // --section-levels
  int histBins = 0;                  // --histogram: irt_histogram in place of the frame
  bool histogram = false, histThickness = false;
  std::vector<float> histBands;      // --histogram-bands: the band edges
  std::vector<float> graticule;      // --graticule: latStepDeg, lonStepDeg
  std::string linesFile;             // --lines
  float lineWidth = 1.5f;            // --line-width, pixels
  bool lineWidthGiven = false;
  bool linesOver = false;            // --lines-over
  float contourRadius = 0.f;         // --contour R:c0,c1,...
  std::vector<float> contour;        // ... the thresholds
  bool contourGiven = false;
  std::vector<float> contourGrid;    // --contour-grid: NLAT, NLON
} g;

void parseList(const std::string &list, std::vector<float> &out) {
  for (size_t a = 0; a < list.size();) {
    const size_t b = std::min(list.find(',', a), list.size());
    out.push_back(strtof(list.substr(a, b - a).c_str(), nullptr));
    a = b + 1;
  }
}

bool endsWith(const std::string &s, const std::string &suffix) {
  return s.size() >= suffix.size() && s.compare(s.size() - suffix.size(), suffix.size(), suffix) == 0;
}

void parseRange(const std::string &s, irt_box1f &r) {  // hostCode.cu:115-124
  r.lower = std::stof(s.substr(0, s.find(':')));
  r.upper = std::stof(s.substr(s.find(':') + 1));
}

void parseCommandLine(int argc, char *argv[]) {  // hostCode.cu:106-129
  for (int i = 1; i < argc; ++i) {
    std::string arg = argv[i];
    if (arg[0] != '-' && endsWith(arg, ".ic"))
      g.filepath = arg;
    else if (arg == "--num-cells" && i + 1 < argc)
      g.maxNumCells = atol(argv[++i]);
    else if (arg == "--lat-range" && i + 1 < argc)
      parseRange(argv[++i], g.latRange);
    else if (arg == "--lon-range" && i + 1 < argc)
      parseRange(argv[++i], g.lonRange);
    else if (arg == "-mode" && i + 1 < argc)
      g.mode = atoi(argv[++i]);  // hostCode.cu:125-127
    else if (arg == "--synth" && i + 3 < argc) {
      for (int k = 0; k < 3; ++k) g.synth[k] = atoi(argv[++i]);
    } else if (arg == "--bench" && i + 1 < argc)
      g.benchFrames = atoi(argv[++i]);
    else if (arg == "--frames-per-launch" && i + 1 < argc)
      g.framesPerLaunch = atoi(argv[++i]) < 1 ? 1 : atoi(argv[i]);
    else if (arg == "--true-size")
      g.trueSize = true;
    else if (arg == "--accel" && i + 1 < argc)
      g.accelMode = std::string(argv[++i]) == "grid" ? IRT_ACCEL_GRID : IRT_ACCEL_SPHERE;
    else if (arg == "--gpus" && i + 1 < argc)
      g.gpus = atoi(argv[++i]);
    else if (arg == "--dump-fb" && i + 1 < argc)
      g.dumpFb = argv[++i];
    else if (arg == "--levels" && i + 1 < argc)
      parseList(argv[++i], g.levels);
    else if (arg == "--levels-back")
      g.levelsBack = true;
    else if (arg == "--section" && i + 1 < argc)
      parseList(argv[++i], g.section);
    else if (arg == "--section-levels" && i + 1 < argc)
      parseList(argv[++i], g.sectionLevels);
    else if (arg == "--histogram" && i + 1 < argc) {
      g.histogram = true;
      g.histBins = atoi(argv[++i]);
    } else if (arg == "--histogram-thickness")
      g.histThickness = true;
    else if (arg == "--histogram-bands" && i + 1 < argc)
      parseList(argv[++i], g.histBands);
    else if (arg == "--graticule" && i + 1 < argc)
      parseList(argv[++i], g.graticule);
    else if (arg == "--lines" && i + 1 < argc)
      g.linesFile = argv[++i];
    else if (arg == "--line-width" && i + 1 < argc)
      g.lineWidth = strtof(argv[++i], nullptr), g.lineWidthGiven = true;
    else if (arg == "--lines-over")
      g.linesOver = true;
    else if (arg == "--contour" && i + 1 < argc) {
      const std::string v = argv[++i];
      const size_t colon = v.find(':');
      g.contourGiven = true;
      g.contourRadius = strtof(v.substr(0, colon).c_str(), nullptr);
      if (colon != std::string::npos) parseList(v.substr(colon + 1), g.contour);
    } else if (arg == "--contour-grid" && i + 1 < argc)
      parseList(argv[++i], g.contourGrid);
  }
}

// --lines FILE: "lat lon" in degrees per line, a blank line between polylines, # starts a comment
bool readLines(const std::string &path, std::vector<float> &lat, std::vector<float> &lon, std::vector<int32_t> &first) {
  std::ifstream f(path);
  if (!f) return false;
  const double rad = 3.14159265358979323846 / 180.0;
  std::string line;  // of any length
  first.assign(1, 0);
  while (std::getline(f, line)) {
    line = line.substr(0, line.find('#'));
    double a, b;
    if (sscanf(line.c_str(), "%lf %lf", &a, &b) == 2) {
      lat.push_back((float)(a * rad));
      lon.push_back((float)(b * rad));
    } else if (first.back() != (int32_t)lat.size()) {
      first.push_back((int32_t)lat.size());  // a blank line ends a polyline
    }
  }
  if (first.back() != (int32_t)lat.size()) first.push_back((int32_t)lat.size());
  return true;
}

void die(const char *what) {
  fprintf(stderr, "%s: %s\n", what, irt_last_error());
  exit(1);
}

void dieMulti(const char *what) {
  fprintf(stderr, "%s: %s\n", what, irt_multi_last_error());
  exit(1);
}

}  // namespace

int main(int argc, char *argv[]) {
  if (argc < 2) {
    fprintf(stderr, "Usage: icon_rt <file.ic> [options]\n");
    return -1;
  }
  parseCommandLine(argc, argv);
  if (!g.levels.empty() && (g.gpus > 0 || g.benchFrames > 0)) {
    fprintf(stderr, "icon_rt: --levels renders on one device and has no --bench form\n");
    return -1;
  }
  if (!g.section.empty() || !g.sectionLevels.empty()) {
    if (g.gpus > 0 || g.benchFrames > 0) {
      fprintf(stderr, "icon_rt: --section runs on one device and has no --bench form\n");
      return -1;
    }
    if (g.section.size() != 5 || g.sectionLevels.empty() || !(g.section[4] >= 1.f && g.section[4] < 2147483648.f) ||
        !g.levels.empty()) {
      fprintf(stderr, "icon_rt: --section takes lat0,lon0,lat1,lon1,n (degrees; n >= 1) with --section-levels "
                      "r0,r1,... and without --levels\n");
      return -1;
    }
  }
  if (g.histogram || g.histThickness || !g.histBands.empty()) {
    if (g.gpus > 0 || g.benchFrames > 0 || !g.levels.empty() || !g.section.empty()) {
      fprintf(stderr, "icon_rt: --histogram runs on one device, without --bench, --levels and --section\n");
      return -1;
    }
    if (!g.histogram || g.histBins < 1 || g.histBands.size() == 1) {
      fprintf(stderr, "icon_rt: --histogram takes the number of bins (at least 1); --histogram-thickness and "
                      "--histogram-bands r0,r1,... (at least two radii) go with it\n");
      return -1;
    }
  }

  if (g.contourGiven || !g.contourGrid.empty()) {
    if (!g.contourGiven || g.contour.empty() || g.contour.size() > IRT_CONTOUR_MAX_THRESHOLDS ||
        !(g.contourRadius > 0.f) || (!g.contourGrid.empty() && g.contourGrid.size() != 2)) {
      fprintf(stderr, "icon_rt: --contour takes R:c0,c1,... (a positive radius, 1 to %d values); --contour-grid "
                      "NLAT,NLON goes with it\n", IRT_CONTOUR_MAX_THRESHOLDS);
      return -1;
    }
  }
  const bool lines = !g.graticule.empty() || !g.linesFile.empty() || g.contourGiven;
  if (lines || g.linesOver || g.lineWidthGiven) {
    if (g.gpus > 0 || g.benchFrames > 0 || !g.section.empty() || g.histogram) {
      fprintf(stderr, "icon_rt: --graticule, --lines and --contour draw into a frame on one device, without --bench, --section "
                      "and --histogram\n");
      return -1;
    }
    if (!lines || (!g.graticule.empty() && g.graticule.size() != 2) || !(g.lineWidth > 0.f)) {
      fprintf(stderr, "icon_rt: --graticule takes latStepDeg,lonStepDeg; --line-width PX (positive) and --lines-over go "
                      "with it, with --lines FILE or with --contour\n");
      return -1;
    }
  }

  // load (hostCode.cu:717-734) or synthesise
  std::vector<irt_icon_cell> cells;
  size_t n = 0;
  if (!g.filepath.empty()) {
    if (irt_load_ic(g.filepath.c_str(), g.maxNumCells, nullptr, 0, &n)) die("load");
    cells.resize(n);
    if (irt_load_ic(g.filepath.c_str(), g.maxNumCells, cells.data(), n, &n)) die("load");
  } else if (g.synth[0] > 0) {
    if (irt_synth_grid(g.synth[0], g.synth[1], g.synth[2], 75e3f, 0.f, 1234, nullptr, 0, &n)) die("synth");
    cells.resize(n);
    if (irt_synth_grid(g.synth[0], g.synth[1], g.synth[2], 75e3f, 0.f, 1234, cells.data(), n, &n))
      die("synth");
    if (g.maxNumCells >= 0 && (size_t)g.maxNumCells < n) cells.resize(g.maxNumCells);
  } else {
    fprintf(stderr, "Usage: icon_rt <file.ic> [options]\n");
    return -1;
  }
  // lat/lon filter (hostCode.cu:736-758)
  if (irt_filter_cells(cells.data(), cells.size(), g.latRange, g.lonRange, &n)) die("filter");
  cells.resize(n);

  // bounds, dataRange, unitDistance (hostCode.cu:792-808, 838-840)
  irt_volume_info info;
  if (irt_compute_volume_info(cells.data(), cells.size(), &info)) die("volume info");

  Pipeline pl(argc, argv, "icon_rt");  // hostCode.cu:813
  const int imgWidth = 512, imgHeight = 512;  // hostCode.cu:815
  Frame fb(imgWidth, imgHeight);
  pl.setFrame(&fb);

  // default transfer function (hostCode.cu:823-836)
  Transfunc defaultTF;
  if (!pl.transfuncValid()) {
    irt_vec4f lut300[300];
    irt_box1f vr;
    irt_default_transfunc(info.dataRange, lut300, &vr);
    defaultTF.valueRange = vr;
    defaultTF.lut.assign(lut300, lut300 + 300);
    pl.setTransfunc(&defaultTF);
  }

  // the accelerators (hostCode.cu:868-910): one HIP context replaces OptiX/cuBQL/shell
  irt_context *ctx = nullptr;
  irt_multi *multi = nullptr;
  auto t0 = std::chrono::steady_clock::now();
  if (g.gpus > 0) {  // one context per device, an RCCL communicator over them
    std::vector<int> devs(g.gpus);
    for (int d = 0; d < g.gpus; ++d) devs[d] = d;
    if (irt_multi_create_cells(cells.data(), cells.size(), devs.data(), g.gpus, &multi))
      dieMulti("irt_multi_create_cells");
    ctx = irt_multi_context(multi, 0);
    fprintf(stderr, "icon_rt: %d devices, frame tiles dealt by cost, RCCL gather to device 0\n", g.gpus);
  } else if (irt_create(cells.data(), cells.size(), 0, &ctx)) {
    die("irt_create");
  }
  auto t1 = std::chrono::steady_clock::now();
  irt_get_volume_info(ctx, &info);
  fprintf(stderr, "icon_rt: %zu cells, %.2f GiB HBM, locator %d^2 x 6, build %.2f s\n",
          cells.size(), info.deviceBytes / 1073741824.0, info.locatorFaceRes,
          std::chrono::duration<double>(t1 - t0).count());
  pl.setTransfuncUpdateHandler([&](const Transfunc *tf, int) {
    if (multi) {
      if (irt_multi_set_transfunc(multi, tf->lut.data(), tf->size(), tf->valueRange, tf->opacity))
        dieMulti("irt_multi_set_transfunc");
    } else if (irt_set_transfunc(ctx, tf->lut.data(), tf->size(), tf->valueRange, tf->opacity)) {
      die("irt_set_transfunc");
    }
  });

  // camera (hostCode.cu:819-821 viewAll, pipeline.cu:444-454 cmdline override, 939-945)
  const int divW = g.trueSize ? fb.width : imgWidth, divH = g.trueSize ? fb.height : imgHeight;
  irt_launch_params lp;
  memset(&lp, 0, sizeof(lp));
  if (pl.camera.fromCmdline) {
    irt_camera_look_at(pl.camera.vp, pl.camera.vi, pl.camera.vu, pl.camera.fovyDeg, divW, divH, &lp);
  } else {
    irt_camera_view_all(info.bounds, 90.f, divW, divH, &lp);
  }
  lp.ambientColor = {1.f, 1.f, 1.f};  // hostCode.cu:925-926
  lp.ambientRadiance = 1.f;
  lp.unitDistance = info.unitDistance;
  lp.raygen = IRT_RAYGEN_WITH_ACCEL;  // setRayGen(woodcockTrackingWithAccel) (863)
  lp.accelMode = g.accelMode;         // toggleAccelMode (hostCode.cu:170-199)
  if (g.mode == IRT_MODE_CUBQL || g.mode == IRT_MODE_TRIANGLES) {
    // toggleMode (hostCode.cu:152-168): buildCuBQLAccel / buildTriangleAccel's geometry
    for (int d = 0; d < (multi ? g.gpus : 1); ++d)
      if (irt_build_wedge_accel(multi ? irt_multi_context(multi, d) : ctx, cells.data(), cells.size()))
        die("irt_build_wedge_accel");
    lp.mode = g.mode;
  } else if (g.mode != IRT_MODE_USER_GEOM) {
    fprintf(stderr, "icon_rt: unknown -mode %d; using the cell sampler (-mode 0)\n", g.mode);
  }

  if (!g.section.empty()) {  // the curtain in place of the frame loop: an image of its own
    const Transfunc *tf = pl.getTransfunc(0);
    if (irt_set_transfunc(ctx, tf->lut.data(), tf->size(), tf->valueRange, tf->opacity)) die("irt_set_transfunc");
    const int nCol = (int)g.section[4], nLev = (int)g.sectionLevels.size();
    const double rad = 3.14159265358979323846 / 180.0;
    std::vector<float> lat(nCol), lon(nCol);
    double arc = 0.0;
    if (irt_great_circle((float)(g.section[0] * rad), (float)(g.section[1] * rad), (float)(g.section[2] * rad),
                         (float)(g.section[3] * rad), nCol, lat.data(), lon.data(), &arc))
      die("irt_great_circle");
    const size_t nPix = (size_t)nCol * nLev;
    irt_section_out out;
    memset(&out, 0, sizeof(out));
    if (hipMalloc((void **)&out.rgba, nPix * 4) != hipSuccess) die("hipMalloc");
    if (irt_section(ctx, lp.mode, lat.data(), lon.data(), nCol, g.sectionLevels.data(), nullptr, nLev, lp.ambientColor,
                    lp.ambientRadiance, out, 0.f, nullptr))
      die("irt_section");
    std::vector<uint32_t> h(nPix);
    if (hipDeviceSynchronize() != hipSuccess ||
        hipMemcpy(h.data(), out.rgba, nPix * 4, hipMemcpyDeviceToHost) != hipSuccess)
      die("section copy");
    (void)hipFree(out.rgba);
    const std::string fileName = pl.name + "_section.png";
    if (!writePNG(fileName, h.data(), nCol, nLev, /*flip*/ true)) die("section write");
    printf("Output: %s (%d columns over %.6f rad x %d levels)\n", fileName.c_str(), nCol, arc, nLev);
    if (!g.dumpFb.empty()) {  // raw: [k * n + c], RGBA8 with r in the low byte
      FILE *f = fopen(g.dumpFb.c_str(), "wb");
      if (!f || fwrite(h.data(), 4, h.size(), f) != h.size()) die("dump-fb write");
      fclose(f);
    }
    irt_destroy(ctx);
    return 0;
  }

  if (g.histogram) {  // the distribution in place of the frame loop: text on stdout
    const Transfunc *tf = pl.getTransfunc(0);
    const int nBands = g.histBands.empty() ? 1 : (int)g.histBands.size() - 1, nBins = g.histBins;
    const size_t nb = (size_t)nBands * nBins, nt = (size_t)nBands * 3;
    irt_histogram_out out;
    memset(&out, 0, sizeof(out));
    if (hipMalloc((void **)&out.bins, nb * 8) != hipSuccess || hipMalloc((void **)&out.tails, nt * 8) != hipSuccess ||
        hipMalloc((void **)&out.outside, 8) != hipSuccess)
      die("hipMalloc");
    if (irt_histogram(ctx, tf->valueRange, nBins, g.histThickness ? IRT_HIST_THICKNESS : IRT_HIST_COUNT,
                      g.histBands.empty() ? nullptr : g.histBands.data(), nBands, out, nullptr))
      die("irt_histogram");
    std::vector<uint64_t> bins(nb), tails(nt);
    uint64_t outside = 0;
    if (hipDeviceSynchronize() != hipSuccess ||
        hipMemcpy(bins.data(), out.bins, nb * 8, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(tails.data(), out.tails, nt * 8, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(&outside, out.outside, 8, hipMemcpyDeviceToHost) != hipSuccess)
      die("histogram copy");
    (void)hipFree(out.bins), (void)hipFree(out.tails), (void)hipFree(out.outside);
    printf("histogram: %d bins over [%.9g, %.9g], %s, %d band(s)\n", nBins, (double)tf->valueRange.lower,
           (double)tf->valueRange.upper, g.histThickness ? "thickness in 1/64 m" : "count", nBands);
    for (int b = 0; b < nBands; ++b) {
      printf("band %d:", b);
      for (int k = 0; k < nBins; ++k) printf(" %llu", (unsigned long long)bins[(size_t)b * nBins + k]);
      printf(" | under %llu over %llu nonfinite %llu\n", (unsigned long long)tails[3 * b],
             (unsigned long long)tails[3 * b + 1], (unsigned long long)tails[3 * b + 2]);
    }
    printf("outside: %llu\n", (unsigned long long)outside);
    irt_destroy(ctx);
    return 0;
  }

  // the lines: segments of the graticule (style 1, thin and translucent) and of the file's polylines
  // (style 0), PX pixels wide at the sub-camera point -- a pixel's angle at the frame's centre times
  // the camera's distance from the sphere, over its radius
  irt_overlay *overlay = nullptr;
  irt_vec4f *cover = nullptr;
  const float surface = g.contourGiven ? g.contourRadius : info.sphericalBounds.lower.x;
  if (lines) {
    const double rad = 3.14159265358979323846 / 180.0;
    float w = 0.f;
    if (irt_overlay_width(&lp, surface, g.lineWidth, &w)) die("irt_overlay_width");
    const irt_overlay_style styles[3] = {{{1.f, 1.f, 1.f, 1.f}, w}, {{0.75f, 0.75f, 0.75f, 0.7f}, w},
                                         {{0.05f, 0.05f, 0.05f, 1.f}, w}};  // (2: the isolines)
    std::vector<irt_overlay_segment> seg;
    size_t nSeg = 0;
    const float maxArc = (float)rad;  // 1 degree pieces
    if (!g.linesFile.empty()) {
      std::vector<float> lat, lon;
      std::vector<int32_t> first;
      if (!readLines(g.linesFile, lat, lon, first)) {
        fprintf(stderr, "icon_rt: cannot read %s\n", g.linesFile.c_str());
        return 1;
      }
      if (irt_overlay_segments(lat.data(), lon.data(), first.data(), (int)first.size() - 1, maxArc, 0, nullptr, 0, &nSeg))
        die("irt_overlay_segments");
      seg.resize(nSeg);
      if (irt_overlay_segments(lat.data(), lon.data(), first.data(), (int)first.size() - 1, maxArc, 0, seg.data(),
                               seg.size(), &nSeg))
        die("irt_overlay_segments");
    }
    if (!g.graticule.empty()) {
      const float sLat = (float)(g.graticule[0] * rad), sLon = (float)(g.graticule[1] * rad);
      const size_t have = seg.size();
      if (irt_graticule(sLat, sLon, maxArc, 1, nullptr, 0, &nSeg)) die("irt_graticule");
      seg.resize(have + nSeg);
      if (irt_graticule(sLat, sLon, maxArc, 1, seg.data() + have, nSeg, &nSeg)) die("irt_graticule");
    }
    if (g.contourGiven) {  // the isolines, on the device; they come last, so the others keep their indices
      const double pi = 3.14159265358979323846;
      const int numLat = g.contourGrid.empty() ? 361 : (int)g.contourGrid[0];
      const int numLon = g.contourGrid.empty() ? 720 : (int)g.contourGrid[1];
      if (numLat < 2 || numLon < 2) {
        fprintf(stderr, "icon_rt: --contour-grid %d,%d: at least 2,2\n", numLat, numLon);
        return -1;
      }
      std::vector<float> lat(numLat), lon(numLon);
      for (int j = 0; j < numLat; ++j) lat[j] = (float)(-0.5 * pi + pi * (double)j / (double)(numLat - 1));
      lat[0] = -(float)(0.5 * pi), lat[numLat - 1] = (float)(0.5 * pi);
      for (int i = 0; i < numLon; ++i) lon[i] = (float)(-pi + 2.0 * pi * (double)i / (double)numLon);
      const std::vector<int32_t> style(g.contour.size(), 2);
      const int T = (int)g.contour.size();
      size_t perT[IRT_CONTOUR_MAX_THRESHOLDS] = {};
      if (irt_contour_latlon(ctx, lp.mode, lat.data(), numLat, lon.data(), numLon, g.contourRadius, g.contour.data(),
                             style.data(), T, IRT_CONTOUR_WRAP, nullptr, 0, &nSeg, perT, nullptr))
        die("irt_contour_latlon");
      irt_overlay_segment *dSeg = nullptr;
      const size_t have = seg.size();
      if (nSeg) {
        if (hipMalloc((void **)&dSeg, nSeg * sizeof(irt_overlay_segment)) != hipSuccess) {
          fprintf(stderr, "icon_rt: no device memory for %zu isoline segments\n", nSeg);
          return 1;
        }
        if (irt_contour_latlon(ctx, lp.mode, lat.data(), numLat, lon.data(), numLon, g.contourRadius, g.contour.data(),
                               style.data(), T, IRT_CONTOUR_WRAP, dSeg, nSeg, &nSeg, perT, nullptr))
          die("irt_contour_latlon");
        seg.resize(have + nSeg);
        // (the null stream's copy runs behind the emit pass)
        if (hipMemcpy(seg.data() + have, dSeg, nSeg * sizeof(irt_overlay_segment), hipMemcpyDeviceToHost) != hipSuccess) {
          fprintf(stderr, "icon_rt: copying the isoline segments back failed\n");
          return 1;
        }
        (void)hipFree(dSeg);
      }
      fprintf(stderr, "icon_rt: isolines at radius %.9g on a %d x %d grid:", (double)g.contourRadius, numLat, numLon);
      for (int t = 0; t < T; ++t) fprintf(stderr, " %.9g: %zu", (double)g.contour[t], perT[t]);
      fprintf(stderr, " segments\n");
    }
    if (irt_overlay_create(ctx, seg.data(), seg.size(), styles, 3, 0, &overlay)) die("irt_overlay_create");
    // the line layer is lerped from the first frame on (0 * old at accumID 0): it starts cleared
    const size_t coverBytes = (size_t)fb.width * fb.height * sizeof(irt_vec4f);
    if (hipMalloc((void **)&cover, coverBytes) != hipSuccess || hipMemset(cover, 0, coverBytes) != hipSuccess) {
      fprintf(stderr, "icon_rt: no device memory for the line layer (%zu bytes)\n", coverBytes);
      return 1;
    }
    fprintf(stderr, "icon_rt: %zu line segments, half-width %.3g rad, %s the frame\n", seg.size(), (double)w,
            g.linesOver ? "over" : "under");
  }
  auto drawLines = [&] {  // into the frame the render call just wrote
    if (overlay && irt_render_overlay(ctx, overlay, &lp, fb.width, fb.height, surface, g.linesOver ? IRT_OVERLAY_OVER : 0,
                                      fb.accumBuffer, cover, fb.fbPointer, nullptr, nullptr))
      die("irt_render_overlay");
  };

  pl.clearFramebuffer = [&] {
    if (irt_clear_frame(ctx, fb.fbPointer, fb.accumBuffer, (size_t)fb.width * fb.height, nullptr))
      die("clear");
  };
  pl.setRayGen([&] {
    if (multi) {
      if (irt_multi_render(multi, &lp, fb.width, fb.height, 1, fb.fbPointer, nullptr)) dieMulti("irt_multi_render");
      return;
    }
    if (!g.levels.empty()) {  // the level surfaces in place of the volume; the frame loop is the same
      if (irt_render_levels(ctx, &lp, fb.width, fb.height, g.levels.data(), (int)g.levels.size(),
                            g.levelsBack ? IRT_LEVELS_BACK : 0, fb.fbPointer, fb.accumBuffer, nullptr, nullptr, 0.f,
                            nullptr))
        die("irt_render_levels");
      drawLines();
      return;
    }
    if (irt_render(ctx, &lp, fb.width, fb.height, fb.fbPointer, fb.accumBuffer, nullptr))
      die("irt_render");
    irt_render_stats st;
    irt_get_render_stats(ctx, &st);
    drawLines();
  });

  do {  // hostCode.cu:931-965
    lp.accumID = pl.frameID;
    pl.launch();
    pl.present();
  } while (pl.isRunning());

  if (g.benchFrames > 0) {
    // as bench.py: per-launch counting off, the launches back to back, one wait at the end
    for (int d = 0; d < (multi ? g.gpus : 1); ++d)
      if (irt_set_statistics(multi ? irt_multi_context(multi, d) : ctx, 0)) die("irt_set_statistics");
    const int B = g.framesPerLaunch;
    auto render = [&](int k, int n) {  // B > 1: frames k .. k+n-1 of the accumulation in one launch
      lp.accumID = B > 1 ? k : 0;
      if (multi) {
        if (irt_multi_render(multi, &lp, fb.width, fb.height, n, fb.fbPointer, nullptr)) dieMulti("irt_multi_render");
        return;
      }
      const int rc = n > 1 ? irt_render_accumulate(ctx, &lp, fb.width, fb.height, n, fb.fbPointer,
                                                   fb.accumBuffer, nullptr)
                           : irt_render(ctx, &lp, fb.width, fb.height, fb.fbPointer, fb.accumBuffer, nullptr);
      if (rc) die("irt_render");
    };
    auto sync = [&] {
      if (multi && irt_multi_synchronize(multi)) dieMulti("irt_multi_synchronize");
      if (hipDeviceSynchronize() != hipSuccess) die("hipDeviceSynchronize");
    };
    render(0, B);  // warm-up
    sync();
    const auto a = std::chrono::steady_clock::now();
    for (int k = 0; k < g.benchFrames; k += B) render(B + k, std::min(B, g.benchFrames - k));
    sync();
    const double total = std::chrono::duration<double>(std::chrono::steady_clock::now() - a).count();
    const double px = (double)fb.width * fb.height * g.benchFrames;
    printf("bench: %d frames %dx%d, %d per launch, %d device(s): %.4f ms/frame, %.1f Mray/s\n", g.benchFrames,
           fb.width, fb.height, B, multi ? g.gpus : 1, 1e3 * total / g.benchFrames, px / total / 1e6);
  }
  if (!g.dumpFb.empty()) {  // the final framebuffer (after --bench's frames), raw (x + W*y, RGBA8 with r in the low byte)
    if (multi && irt_multi_synchronize(multi)) dieMulti("irt_multi_synchronize");
    std::vector<uint32_t> h((size_t)fb.width * fb.height);
    if (hipDeviceSynchronize() != hipSuccess ||
        hipMemcpy(h.data(), fb.fbPointer, h.size() * 4, hipMemcpyDeviceToHost) != hipSuccess)
      die("dump-fb copy");
    FILE *f = fopen(g.dumpFb.c_str(), "wb");
    if (!f || fwrite(h.data(), 4, h.size(), f) != h.size()) die("dump-fb write");
    fclose(f);
  }
  if (cover) (void)hipFree(cover);
  if (multi)
    irt_multi_destroy(multi);
  else
    irt_destroy(ctx);  // (with its overlay)
  return 0;
}
