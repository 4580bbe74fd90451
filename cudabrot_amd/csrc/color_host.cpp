// color_host.cpp -- the colour stage on the host (include/cudabrot_amd.h, "Colour image"): the restatement
// cb_compose_color, the level selection the device path shares (color.hip finds its buckets with the same
// functions) and the PPM writer.  Host code only.
#include <hip/hip_runtime_api.h>
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "color_math.h"

namespace cb {

int color_params_ok(const cb_color_params *p) {
  if (!p) return 0;
  if (p->compose != CB_COMPOSE_RGB && p->compose != CB_COMPOSE_HSL) return 0;
  const double b = p->black_percent, w = p->white_percent;
  if (!isfinite(b) || !isfinite(w) || !isfinite(p->hue_shift)) return 0;
  return b >= 0.0 && w >= 0.0 && b + w < 100.0;
}

void color_ranks(uint64_t n, const cb_color_params *p, uint64_t *nb, uint64_t *nw) {
  *nb = (uint64_t) ((double) n * (p->black_percent / 100.0));
  *nw = (uint64_t) ((double) n * (p->white_percent / 100.0));
}

// B + W < 100 keeps nb, nw below the pixel count, so both searches find their bin.
uint32_t color_select_low(const uint64_t *bins, uint32_t n_bins, uint64_t rank, uint64_t *below) {
  uint64_t cum = 0;
  for (uint32_t k = 0; k < n_bins; ++k) {
    if (cum + bins[k] > rank) {
      *below = cum;
      return k;
    }
    cum += bins[k];
  }
  *below = cum;
  return n_bins - 1;
}

uint32_t color_select_high(const uint64_t *bins, uint32_t n_bins, uint64_t rank, uint64_t *above) {
  uint64_t cum = 0;
  for (uint32_t k = n_bins; k-- > 0;) {
    if (cum + bins[k] > rank) {
      *above = cum;
      return k;
    }
    cum += bins[k];
  }
  *above = cum;
  return 0;
}

PlaneLevels color_plane_levels(uint32_t black, uint32_t white) {
  PlaneLevels l;
  l.black = black;
  l.white = white;
  l.inv = white > black ? 1.0 / (double) (white - black) : 0.0;
  return l;
}

}  // namespace cb

extern "C" {

int cb_compose_color(const uint16_t *const gray[3], int w, int h, const cb_color_params *p, uint16_t *rgb_be,
                     uint16_t levels[6]) {
  using namespace cb;
  if (!gray || !gray[0] || !gray[1] || !gray[2] || !rgb_be || w <= 0 || h <= 0 || !color_params_ok(p)) {
    return (int) hipErrorInvalidValue;
  }
  const uint64_t n = (uint64_t) w * (uint64_t) h;
  uint64_t nb = 0, nw = 0;
  color_ranks(n, p, &nb, &nw);
  PlaneLevels l[3];
  std::vector<uint64_t> hist(65536);
  for (int j = 0; j < 3; ++j) {
    std::fill(hist.begin(), hist.end(), 0ull);
    for (uint64_t i = 0; i < n; ++i) hist[gray[j][i]]++;
    uint64_t rest = 0;
    const uint32_t black = color_select_low(hist.data(), 65536, nb, &rest);
    const uint32_t white = color_select_high(hist.data(), 65536, nw, &rest);
    l[j] = color_plane_levels(black, white);
    if (levels) {
      levels[2 * j] = (uint16_t) black;
      levels[2 * j + 1] = (uint16_t) white;
    }
  }
  for (uint64_t i = 0; i < n; ++i) {
    uint32_t rgb[3];
    color_compose(p->compose, p->hue_shift, color_stretch(gray[0][i], l[0]), color_stretch(gray[1][i], l[1]),
                  color_stretch(gray[2][i], l[2]), rgb);
    for (int c = 0; c < 3; ++c) rgb_be[3 * i + (uint64_t) c] = (uint16_t) color_swap16(rgb[c]);
  }
  return 0;
}

int cb_save_ppm_be(const char *path, const uint16_t *rgb_be, int w, int h) {
  if (!path || !rgb_be || w <= 0 || h <= 0) return 1;
  const uint64_t samples = 3ull * (uint64_t) w * (uint64_t) h;
  FILE *output = fopen(path, "wb");
  if (!output) return 1;
  if (fprintf(output, "P6\n%d %d\n%d\n", w, h, 0xffff) <= 0) {  // the PGM header's form (cb_save_image_be)
    fclose(output);
    return 2;
  }
  if (!fwrite(rgb_be, samples * sizeof(uint16_t), 1, output)) {
    fclose(output);
    return 3;
  }
  fclose(output);
  return 0;
}

}  // extern "C"
