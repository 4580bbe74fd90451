// equalize_local.h -- the arithmetic of the locally equalised image (include/cudabrot_amd.h, "Locally equalised image";
// DESIGN.md 4.28), ONE definition for the host functions (host_output.cpp) and the two kernels (equalize_local.hip): the
// tile grid, the place of a pixel between two tile centres, and the integer blend of four table values.
#pragma once

#include "color_math.h"

namespace cb {

constexpr int kLocalMaxTiles = CB_LOCAL_EQUALIZE_MAX_TILES;  // a side

// The grid of a canvas: the tile edges and the doubled tile centres of both axes.
struct LocalGrid {
  uint32_t w, h, planes, tx, ty;
  uint32_t ex[kLocalMaxTiles + 1], ey[kLocalMaxTiles + 1];  // ex[i] = floor(i * w / tx)
  uint32_t cx[kLocalMaxTiles], cy[kLocalMaxTiles];          // cx[i] = ex[i] + ex[i + 1]
};

inline LocalGrid local_grid(int w, int h, int planes, int tx, int ty) {  // of arguments cb_local_equalize_ok admits
  LocalGrid g = {};
  g.w = (uint32_t) w, g.h = (uint32_t) h, g.planes = (uint32_t) planes, g.tx = (uint32_t) tx, g.ty = (uint32_t) ty;
  for (uint32_t i = 0; i <= g.tx; ++i) g.ex[i] = (uint32_t) ((uint64_t) i * g.w / g.tx);
  for (uint32_t j = 0; j <= g.ty; ++j) g.ey[j] = (uint32_t) ((uint64_t) j * g.h / g.ty);
  for (uint32_t i = 0; i < g.tx; ++i) g.cx[i] = g.ex[i] + g.ex[i + 1];
  for (uint32_t j = 0; j < g.ty; ++j) g.cy[j] = g.ey[j] + g.ey[j + 1];
  return g;
}

// Where p = 2 * position + 1 stands among the t ascending doubled centres c: the two tiles it lies between, its distance
// a from the first centre and the distance d of the two.  At or outside the outermost centres (and with one tile) it is
// that tile alone: (i, i, 0, 1).
struct alignas(16) LocalPlace {  // (one 16-byte load on the device)
  uint32_t i0, i1, a, d;
};
CB_COLOR_FN LocalPlace local_place(const uint32_t *c, uint32_t t, uint32_t p) {
  uint32_t at = 0, lo = c[0], hi = c[0];
  for (uint32_t i = 1; i < t; ++i) {
    const uint32_t v = c[i];
    if (v <= p) {
      at = i;
      lo = v;
    }
    hi = (v > p && hi <= p) ? v : hi;  // the first centre above p
  }
  const bool alone = p <= c[0] || hi <= p;  // hi <= p: no centre above p
  LocalPlace place;
  place.i0 = at;
  place.i1 = alone ? at : at + 1u;
  place.a = alone ? 0u : p - lo;
  place.d = alone ? 1u : hi - lo;
  return place;
}

// The pixel of the four table values: below 2^57 throughout (d of x times d of y is at most w * h <= 2^40).
CB_COLOR_FN uint32_t local_blend(uint64_t v00, uint64_t v10, uint64_t v01, uint64_t v11, const LocalPlace &x,
                                 const LocalPlace &y) {
  const uint64_t ax = x.a, bx = x.d - x.a, ay = y.a, by = y.d - y.a;
  const uint64_t num = by * (bx * v00 + ax * v10) + ay * (bx * v01 + ax * v11);
  const uint64_t den = (uint64_t) x.d * (uint64_t) y.d;
  return (uint32_t) ((num + den / 2u) / den);
}

// ---- the host's steps (host_output.cpp) ----

// cb_equalize_table over the first n_keys keys: bins and table_out have n_keys entries, every key from n_keys on is empty.
void equalize_table_keys(const uint64_t *bins, uint32_t n_keys, double gamma, uint16_t *table_out, uint64_t *keys_out,
                         uint64_t *levels_out);
// The step between the two kernels: `tiles` rows of n_keys bins -> as many rows of table values, every tile clipped and
// tabulated, an empty one given the global table; and the three reported numbers.
void local_equalize_tables(const uint64_t *bins, uint32_t n_keys, uint32_t tiles, uint32_t clip_q, double gamma,
                           uint16_t *tables_out, uint64_t *lit_out, uint64_t *lit_tiles_out, uint64_t *moved_out);

}  // namespace cb
