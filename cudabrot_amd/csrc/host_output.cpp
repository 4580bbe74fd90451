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
#include "equalize_local.h"  // equalize_key (color_math.h) and the local grid

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

namespace cb {

void equalize_table_keys(const uint64_t *bins, uint32_t n_keys, double gamma, uint16_t *table_out, uint64_t *keys_out,
                         uint64_t *levels_out) {
  uint64_t lit = 0, le = 0, keys = 0, levels = 0;
  for (uint32_t k = 0; k < n_keys; k++) lit += bins[k];
  table_out[0] = 0;
  std::vector<bool> seen(65536, false);
  // an empty bin has the rank, and so the value, of the key below it: cb_tone_value is called once per lit key
  for (uint32_t k = 1; k < n_keys; k++) {
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
}

namespace {

bool local_clip_ok(uint32_t clip_q) { return clip_q == 0 || (clip_q >= 256 && clip_q <= 65536); }

// "Locally equalised image", clip: n_keys bins of one tile -> its clipped bins (which may be `bins` itself) and E.
uint64_t local_clip(const uint64_t *bins, uint32_t n_keys, uint32_t clip_q, uint64_t *clipped) {
  uint64_t lit = 0, keys = 0;
  for (uint32_t k = 0; k < n_keys; k++) {
    lit += bins[k];
    keys += bins[k] != 0 ? 1u : 0u;
  }
  if (clip_q == 0 || keys == 0) {
    if (clipped != bins) memcpy(clipped, bins, n_keys * sizeof(uint64_t));
    return 0;
  }
  const uint64_t share = (uint64_t) clip_q * lit / (256 * keys), limit = share > 1 ? share : 1;
  uint64_t excess = 0;
  for (uint32_t k = 0; k < n_keys; k++) excess += bins[k] > limit ? bins[k] - limit : 0;
  const uint64_t each = excess / keys, more = excess % keys;
  uint64_t m = 0;  // the lit keys so far
  for (uint32_t k = 0; k < n_keys; k++) {
    const uint64_t b = bins[k];
    clipped[k] = b == 0 ? 0 : (b < limit ? b : limit) + each + (m < more ? 1u : 0u);
    m += b != 0 ? 1u : 0u;
  }
  return excess;
}

uint64_t largest(const cb_pixel *hist, uint64_t n) {
  uint64_t max = 0;
  for (uint64_t i = 0; i < n; i++) {
    if (hist[i] > max) max = hist[i];
  }
  return max;
}

// bins_t of the definition, n_keys entries a tile (every key of the array is below n_keys), and lit.
void local_bins(const cb_pixel *hist, const LocalGrid &g, uint32_t n_keys, uint64_t *bins, uint64_t *lit_out) {
  memset(bins, 0, (size_t) g.tx * g.ty * n_keys * sizeof(uint64_t));
  uint64_t lit = 0;
  for (uint32_t p = 0; p < g.planes; ++p) {
    for (uint32_t j = 0; j < g.ty; ++j) {
      for (uint32_t y = g.ey[j]; y < g.ey[j + 1]; ++y) {
        const cb_pixel *row = hist + ((uint64_t) p * g.h + y) * g.w;
        for (uint32_t i = 0; i < g.tx; ++i) {
          uint64_t *mine = bins + (size_t) (j * g.tx + i) * n_keys;
          for (uint32_t x = g.ex[i]; x < g.ex[i + 1]; ++x) {
            if (row[x] == 0) continue;
            mine[equalize_key(row[x])]++;
            lit++;
          }
        }
      }
    }
  }
  *lit_out = lit;
}

}  // namespace

void local_equalize_tables(const uint64_t *bins, uint32_t n_keys, uint32_t tiles, uint32_t clip_q, double gamma,
                           uint16_t *tables_out, uint64_t *lit_out, uint64_t *lit_tiles_out, uint64_t *moved_out) {
  std::vector<uint64_t> all(n_keys, 0), clipped(n_keys);
  std::vector<bool> empty(tiles, false);
  uint64_t lit = 0, lit_tiles = 0, moved = 0, keys = 0, levels = 0;
  for (uint32_t t = 0; t < tiles; ++t) {
    const uint64_t *mine = bins + (size_t) t * n_keys;
    uint64_t lit_t = 0;
    for (uint32_t k = 0; k < n_keys; k++) {
      all[k] += mine[k];
      lit_t += mine[k];
    }
    empty[t] = lit_t == 0;
    if (empty[t]) continue;
    lit += lit_t;
    lit_tiles++;
    moved += local_clip(mine, n_keys, clip_q, clipped.data());
    equalize_table_keys(clipped.data(), n_keys, gamma, tables_out + (size_t) t * n_keys, &keys, &levels);
  }
  if (lit_tiles < tiles) {  // the empty tiles take the global curve, unclipped
    std::vector<uint16_t> global(n_keys);
    equalize_table_keys(all.data(), n_keys, gamma, global.data(), &keys, &levels);
    for (uint32_t t = 0; t < tiles; ++t) {
      if (empty[t]) memcpy(tables_out + (size_t) t * n_keys, global.data(), n_keys * sizeof(uint16_t));
    }
  }
  *lit_out = lit;
  *lit_tiles_out = lit_tiles;
  *moved_out = moved;
}

}  // namespace cb

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
  cb::equalize_table_keys(bins, CB_EQUALIZE_KEYS, gamma, table_out, keys_out, levels_out);
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

// "Locally equalised image" of include/cudabrot_amd.h, the definition: the grid, the bins, the clip, the tables, the blend.
int cb_local_equalize_ok(int w, int h, int planes, int tx, int ty, uint32_t clip_q) {
  return (w > 0 && h > 0 && planes >= 1 && tx >= 1 && tx <= cb::kLocalMaxTiles && ty >= 1 && ty <= cb::kLocalMaxTiles &&
          tx <= w && ty <= h && cb::local_clip_ok(clip_q))
             ? 1
             : 0;
}

int cb_local_equalize_bins(const cb_pixel *hist, int w, int h, int planes, int tx, int ty, uint64_t *bins_out,
                           uint64_t *lit_out, uint64_t *max_out) {
  if (!hist || !bins_out || !lit_out || !max_out || !cb_local_equalize_ok(w, h, planes, tx, ty, 0)) return 1;  // hipErrorInvalidValue
  cb::local_bins(hist, cb::local_grid(w, h, planes, tx, ty), CB_EQUALIZE_KEYS, bins_out, lit_out);
  *max_out = cb::largest(hist, (uint64_t) w * (uint64_t) h * (uint64_t) planes);
  return 0;
}

int cb_local_equalize_clip(const uint64_t *bins, uint32_t clip_q, uint64_t *clipped_out, uint64_t *moved_out) {
  if (!bins || !clipped_out || !moved_out || !cb::local_clip_ok(clip_q)) return 1;  // hipErrorInvalidValue
  *moved_out = cb::local_clip(bins, CB_EQUALIZE_KEYS, clip_q, clipped_out);
  return 0;
}

int cb_set_grayscale_pixels_local_equalized(const cb_pixel *hist, int w, int h, int planes, int tx, int ty, uint32_t clip_q,
                                            double gamma, uint16_t *gray_out, uint64_t *max_out, double *scale_out,
                                            uint64_t *lit_out, uint64_t *lit_tiles_out, uint64_t *moved_out) {
  if (!hist || !gray_out || !cb_local_equalize_ok(w, h, planes, tx, ty, clip_q)) return 1;  // hipErrorInvalidValue
  const cb::LocalGrid g = cb::local_grid(w, h, planes, tx, ty);
  const uint64_t n = (uint64_t) w * (uint64_t) h * (uint64_t) planes;
  const uint64_t max = cb::largest(hist, n);
  uint64_t lit = 0, lit_tiles = 0, moved = 0;
  const uint32_t n_keys = cb::equalize_key(max) + 1, tiles = g.tx * g.ty;  // every key of the image is below n_keys
  std::vector<uint64_t> bins((size_t) tiles * n_keys);
  std::vector<uint16_t> tables((size_t) tiles * n_keys);
  cb::local_bins(hist, g, n_keys, bins.data(), &lit);
  cb::local_equalize_tables(bins.data(), n_keys, tiles, clip_q, gamma, tables.data(), &lit, &lit_tiles, &moved);
  if (max_out) *max_out = max;
  if (scale_out) *scale_out = ((double) 0xffff) / ((double) max);  // what the unflagged call reports
  if (lit_out) *lit_out = lit;
  if (lit_tiles_out) *lit_tiles_out = lit_tiles;
  if (moved_out) *moved_out = moved;
  std::vector<cb::LocalPlace> columns((size_t) w);
  for (uint32_t x = 0; x < g.w; ++x) columns[x] = cb::local_place(g.cx, g.tx, 2 * x + 1);
  for (uint32_t p = 0; p < g.planes; ++p) {
    for (uint32_t y = 0; y < g.h; ++y) {
      const cb::LocalPlace row = cb::local_place(g.cy, g.ty, 2 * y + 1);
      const uint16_t *upper = tables.data() + (size_t) row.i0 * g.tx * n_keys, *lower = tables.data() + (size_t) row.i1 * g.tx * n_keys;
      const uint64_t at = ((uint64_t) p * g.h + y) * g.w;
      for (uint32_t x = 0; x < g.w; ++x) {
        const cb::LocalPlace &col = columns[x];
        const size_t k = cb::equalize_key(hist[at + x]), left = (size_t) col.i0 * n_keys + k, right = (size_t) col.i1 * n_keys + k;
        gray_out[at + x] = (uint16_t) cb::local_blend(upper[left], upper[right], lower[left], lower[right], col, row);
      }
    }
  }
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
