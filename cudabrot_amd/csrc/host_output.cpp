// host_output.cpp -- the output stage of the reference's host driver: tone mapping and the PGM
// writer (cudabrot.cu:416-468, 548-577).  Host code, as in the reference.
#include <errno.h>
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <functional>
#include <vector>

#include "../../include/cudabrot_amd.h"
#include "color_math.h"  // equalize_key

namespace {

// Clamp, cudabrot.cu:416-420
inline uint16_t clamp_u16(double v) {
  if (v <= 0) return 0;
  if (v >= 0xffff) return 0xffff;
  return (uint16_t) v;
}

// The reference converts double -> uint16_t implicitly (cudabrot.cu:447); x86-64 does that through
// cvttsd2si and keeps the low 16 bits.  NaN (an all-zero histogram gives scale = inf, 0 * inf) comes
// out as 0 there; pinned here so that the result does not depend on the compiler.
inline uint16_t to_u16(double v) {
  if (v != v) return 0;
  return (uint16_t) (int64_t) v;
}

}  // namespace

extern "C" {

// The value of one pixel: GetLinearColorScale's scale, DoGammaCorrection (or the plain scaling of
// cudabrot.cu:462-466 when gamma <= 0), the conversion to uint16.  ONE definition, used by the host
// path below and by the tables of the device path (tonemap.hip), so that both give the same bytes.
uint16_t cb_tone_value(uint64_t count, uint64_t max, double gamma) {
  const double linear_scale = ((double) 0xffff) / ((double) max);  // cudabrot.cu:436
  const double scaled = ((double) count) * linear_scale;
  if (gamma <= 0.0) return to_u16(scaled);
  const double top = 0xffff;
  const double v = top * pow(scaled / top, 1 / gamma);  // cudabrot.cu:443-449
  return (v != v) ? (uint16_t) 0 : clamp_u16(v);
}

void cb_set_grayscale_pixels(const cb_pixel *hist, int w, int h, double gamma, uint16_t *gray_out,
                             uint64_t *max_out, double *scale_out) {
  const uint64_t n = (uint64_t) w * (uint64_t) h;
  // GetLinearColorScale, cudabrot.cu:425-439
  uint64_t max = 0;
  for (uint64_t i = 0; i < n; i++) {
    if (hist[i] > max) max = hist[i];
  }
  if (max_out) *max_out = max;
  if (scale_out) *scale_out = ((double) 0xffff) / ((double) max);
  for (uint64_t i = 0; i < n; i++) gray_out[i] = cb_tone_value(hist[i], max, gamma);
}

int cb_white_clip_ok(double clip_percent) { return isfinite(clip_percent) && clip_percent >= 0.0 && clip_percent < 100.0; }

uint64_t cb_white_rank(uint64_t lit, double clip_percent) {
  if (lit == 0) return 0;
  const uint64_t r = (uint64_t) ((double) lit * (clip_percent / 100.0));  // color_ranks' arithmetic (color_host.cpp)
  return r < lit - 1 ? r : lit - 1;
}

// "White clip" of include/cudabrot_amd.h, the definition: the lit counters, partially ordered around rank r.
int cb_white_count(const cb_pixel *hist, uint64_t n, double clip_percent, uint64_t *white_out, uint64_t *lit_out,
                   uint64_t *clipped_out) {
  if (!hist || !white_out || !lit_out || !clipped_out || !cb_white_clip_ok(clip_percent)) return 1;  // hipErrorInvalidValue
  std::vector<uint64_t> lit;
  for (uint64_t i = 0; i < n; i++) {
    if (hist[i] > 0) lit.push_back(hist[i]);
  }
  uint64_t white = 0, clipped = 0;
  if (!lit.empty()) {
    const uint64_t r = cb_white_rank(lit.size(), clip_percent);
    std::nth_element(lit.begin(), lit.begin() + (ptrdiff_t) r, lit.end(), std::greater<uint64_t>());
    white = lit[(size_t) r];
    for (uint64_t c : lit) clipped += c > white ? 1u : 0u;
  }
  *white_out = white;
  *lit_out = lit.size();
  *clipped_out = clipped;
  return 0;
}

int cb_set_grayscale_pixels_white(const cb_pixel *hist, int w, int h, double gamma, double clip_percent, uint16_t *gray_out,
                                  uint64_t *max_out, double *scale_out, uint64_t *white_out) {
  if (!hist || !gray_out || w <= 0 || h <= 0 || !cb_white_clip_ok(clip_percent)) return 1;  // hipErrorInvalidValue
  const uint64_t n = (uint64_t) w * (uint64_t) h;
  uint64_t max = 0, white = 0, lit = 0, clipped = 0;
  for (uint64_t i = 0; i < n; i++) {
    if (hist[i] > max) max = hist[i];
  }
  const int rc = cb_white_count(hist, n, clip_percent, &white, &lit, &clipped);
  if (rc) return rc;
  if (max_out) *max_out = max;
  if (scale_out) *scale_out = ((double) 0xffff) / ((double) white);
  if (white_out) *white_out = white;
  // the clamp is on the count: gamma <= 0, the reference's unclamped branch, needs no case of its own
  for (uint64_t i = 0; i < n; i++) gray_out[i] = cb_tone_value(hist[i] < white ? hist[i] : white, white, gamma);
  return 0;
}

// "Equalised image" of include/cudabrot_amd.h, the definition: the key, the bins, the table, the image.
uint32_t cb_equalize_key(uint64_t count) { return cb::equalize_key(count); }

int cb_equalize_bins(const cb_pixel *hist, uint64_t n, uint64_t *bins_out, uint64_t *lit_out, uint64_t *max_out) {
  if (!hist || n == 0 || !bins_out || !lit_out || !max_out) return 1;  // hipErrorInvalidValue
  memset(bins_out, 0, CB_EQUALIZE_KEYS * sizeof(uint64_t));
  uint64_t lit = 0, max = 0;
  for (uint64_t i = 0; i < n; i++) {
    if (hist[i] == 0) continue;
    bins_out[cb::equalize_key(hist[i])]++;
    lit++;
    if (hist[i] > max) max = hist[i];
  }
  *lit_out = lit;
  *max_out = max;
  return 0;
}

int cb_equalize_table(const uint64_t *bins, double gamma, uint16_t *table_out, uint64_t *keys_out, uint64_t *levels_out) {
  if (!bins || !table_out || !keys_out || !levels_out) return 1;  // hipErrorInvalidValue
  uint64_t lit = 0, le = 0, keys = 0, levels = 0;
  for (uint32_t k = 0; k < CB_EQUALIZE_KEYS; k++) lit += bins[k];
  table_out[0] = 0;
  std::vector<bool> seen(65536, false);
  // an empty bin has the rank, and so the value, of the key below it: cb_tone_value is called once per lit key
  for (uint32_t k = 1; k < CB_EQUALIZE_KEYS; k++) {
    table_out[k] = table_out[k - 1];
    if (bins[k] == 0) continue;
    le += bins[k];
    // the full rank is full white: cb_tone_value(lit, lit, gamma) is 65535 in exact arithmetic, and 65534 in doubles for
    // about one lit in seven (lit * (65535.0 / lit) rounds below 65535 and the conversion truncates)
    table_out[k] = (le == lit && gamma > 0.0) ? (uint16_t) 0xffff : cb_tone_value(le, lit, gamma);
    if (!seen[table_out[k]]) levels++;
    seen[table_out[k]] = true;
    keys++;
  }
  *keys_out = keys;
  *levels_out = levels;
  return 0;
}

int cb_set_grayscale_pixels_equalized(const cb_pixel *hist, int w, int h, double gamma, uint16_t *gray_out, uint64_t *max_out,
                                      double *scale_out, uint64_t *lit_out) {
  if (!hist || !gray_out || w <= 0 || h <= 0) return 1;  // hipErrorInvalidValue
  const uint64_t n = (uint64_t) w * (uint64_t) h;
  std::vector<uint64_t> bins(CB_EQUALIZE_KEYS);
  std::vector<uint16_t> table(CB_EQUALIZE_KEYS);
  uint64_t lit = 0, max = 0, keys = 0, levels = 0;
  int rc = cb_equalize_bins(hist, n, bins.data(), &lit, &max);
  if (rc == 0) rc = cb_equalize_table(bins.data(), gamma, table.data(), &keys, &levels);
  if (rc) return rc;
  if (max_out) *max_out = max;
  if (scale_out) *scale_out = ((double) 0xffff) / ((double) max);  // what the unflagged call reports
  if (lit_out) *lit_out = lit;
  for (uint64_t i = 0; i < n; i++) gray_out[i] = table[cb::equalize_key(hist[i])];
  return 0;
}

// "Density filter" of include/cudabrot_amd.h: the table of thresholds, the only floating point of the definition.
int cb_density_thresholds(int radius, double alpha, uint64_t n0, uint64_t *thresholds_out) {
  if (!thresholds_out || radius < 1 || radius > CB_DENSITY_MAX_RADIUS || !isfinite(alpha) || alpha < 1.0 / 16.0 ||
      alpha > 4.0 || n0 < 1 || n0 > (1ull << 20)) {
    return 1;  // hipErrorInvalidValue
  }
  double v[CB_DENSITY_MAX_RADIUS + 1];
  for (int r = 1; r <= radius; ++r) v[r] = floor((double) n0 * pow((double) radius / (double) r, 1.0 / alpha));
  if (!(v[1] < (double) CB_DENSITY_MAX_SMOOTHED)) return 1;  // (before any conversion: v[1] may pass 2^64)
  thresholds_out[0] = ~0ull;
  for (int r = 1; r <= radius; ++r) thresholds_out[r] = (uint64_t) v[r];
  return 0;
}

namespace {

// A table a filter accepts: T[0] = 2^64 - 1, T[1] < 2^22, non-increasing, T[R] >= 1.
bool density_table_ok(int radius, const uint64_t *t) {
  if (!t || radius < 1 || radius > CB_DENSITY_MAX_RADIUS || t[0] != ~0ull || t[1] >= CB_DENSITY_MAX_SMOOTHED) return false;
  for (int r = 1; r <= radius; ++r) {
    if (t[r] > t[r - 1] || t[r] < 1) return false;
  }
  return true;
}

}  // namespace

int cb_density_arguments_ok(const void *hist, int w, int h, int planes, int group, int radius, const uint64_t *thresholds,
                            const void *out) {
  if (!hist || !out || w <= 0 || h <= 0 || planes <= 0 || (group != 1 && group != 3) || planes % group != 0) return 0;
  if (!density_table_ok(radius, thresholds)) return 0;
  const uint64_t bytes = (uint64_t) w * (uint64_t) h * (uint64_t) planes * sizeof(cb_pixel);
  const uintptr_t a = (uintptr_t) hist, b = (uintptr_t) out;
  return (a + bytes <= b || b + bytes <= a) ? 1 : 0;  // output and input may not alias
}

// The definition, plainly: every lit pixel spreads its counters over its neighbourhood.
int cb_density_filter(const cb_pixel *hist, int w, int h, int planes, int group, int radius, const uint64_t *thresholds,
                      uint64_t *out) {
  if (!cb_density_arguments_ok(hist, w, h, planes, group, radius, thresholds, out)) return 1;  // hipErrorInvalidValue
  const uint64_t n = (uint64_t) w * (uint64_t) h;
  for (uint64_t i = 0; i < n * (uint64_t) planes; i++) {
    if (hist[i] >= CB_DENSITY_MAX_COUNT) return 1;  // decided before anything is written
  }
  uint64_t binomial[CB_DENSITY_MAX_RADIUS + 1][2 * CB_DENSITY_MAX_RADIUS + 1] = {};  // [r][i + r] = C(2r, i + r)
  binomial[0][0] = 1;
  for (int r = 1; r <= radius; ++r) {
    uint64_t row[2 * CB_DENSITY_MAX_RADIUS + 2] = {1};
    for (int k = 1; k <= 2 * r; ++k) {
      for (int i = k; i >= 1; --i) row[i] += row[i - 1];
    }
    for (int i = 0; i <= 2 * r; ++i) binomial[r][i] = row[i];
  }
  std::vector<uint64_t> acc((size_t) (n * (uint64_t) planes), 0);
  for (int g = 0; g < planes / group; ++g) {
    const cb_pixel *in = hist + (uint64_t) g * (uint64_t) group * n;
    for (int y = 0; y < h; ++y) {
      for (int x = 0; x < w; ++x) {
        const uint64_t at = (uint64_t) y * (uint64_t) w + (uint64_t) x;
        uint64_t key = 0;
        for (int p = 0; p < group; ++p) key += in[(uint64_t) p * n + at];
        int r = 0;
        while (r < radius && key <= thresholds[r + 1]) ++r;  // the largest r with r = 0 or key <= T[r]
        for (int p = 0; p < group; ++p) {
          const uint64_t plane = ((uint64_t) g * (uint64_t) group + (uint64_t) p) * n;
          const uint64_t count = in[(uint64_t) p * n + at];
          out[plane + at] = (key != 0 && r == 0) ? count : 0;  // sharp
          if (key == 0 || r == 0 || count == 0) continue;
          for (int dy = -r; dy <= r; ++dy) {
            if (y + dy < 0 || y + dy >= h) continue;
            for (int dx = -r; dx <= r; ++dx) {
              if (x + dx < 0 || x + dx >= w) continue;
              acc[plane + (uint64_t) (y + dy) * (uint64_t) w + (uint64_t) (x + dx)] +=
                  (count * binomial[r][dy + r] * binomial[r][dx + r]) << (32 - 4 * r);
            }
          }
        }
      }
    }
  }
  for (uint64_t i = 0; i < n * (uint64_t) planes; i++) out[i] = (out[i] << 8) + (acc[i] >> 24);
  return 0;
}

int cb_save_image(const char *path, uint16_t *gray, int w, int h) {
  const uint64_t pixel_count = (uint64_t) w * (uint64_t) h;
  // big-endian samples, cudabrot.cu:566-570
  for (uint64_t i = 0; i < pixel_count; i++) {
    const uint16_t tmp = gray[i];
    gray[i] = (uint16_t) (((tmp & 0xff) << 8) | (tmp >> 8));
  }
  return cb_save_image_be(path, gray, w, h);
}

int cb_save_image_be(const char *path, const uint16_t *gray_be, int w, int h) {
  const uint64_t pixel_count = (uint64_t) w * (uint64_t) h;
  FILE *output = fopen(path, "wb");
  if (!output) return 1;
  if (fprintf(output, "P5\n%d %d\n%d\n", w, h, 0xffff) <= 0) {  // cudabrot.cu:557
    fclose(output);
    return 2;
  }
  if (!fwrite(gray_be, pixel_count * sizeof(uint16_t), 1, output)) {
    fclose(output);
    return 3;
  }
  fclose(output);
  return 0;
}

}  // extern "C"
