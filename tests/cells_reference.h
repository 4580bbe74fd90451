/* cells_reference.h -- the cell grid of the sample plane (include/cudabrot_amd.h, "Focused render"), restated once for the
 * CPU restatements that draw from a cell list or mark cells (tests/focus_reference.c, tests/aim_reference.c).  Written from
 * the definition, not from the kernels; for the tests only.  n = 4 << level cells of side 2^-level per side of [-2, 2]^2,
 * cell index row * n + col. */
#pragma once

#include <math.h>
#include <stdint.h>

/* The cell that holds the point: (x + 2) * 2^L is exact; x = 2 is clamped into the last cell. */
static inline uint32_t cells_cell_of(int level, double re, double im) {
  const int n = 4 << level;
  int col = (int) ((re + 2.0) * ldexp(1.0, level));
  int row = (int) ((im + 2.0) * ldexp(1.0, level));
  if (col > n - 1) col = n - 1;
  if (row > n - 1) row = n - 1;
  return (uint32_t) row * (uint32_t) n + (uint32_t) col;
}

/* A point of cell list entry j = high half of (a << 32 | b) * n_cells, from the two uniform coordinates x, y. */
static inline void cells_point_of(int level, const uint32_t *cells, uint32_t n_cells, uint32_t a, uint32_t b, double x,
                                  double y, uint32_t *j_out, double *re, double *im) {
  const unsigned __int128 product = (unsigned __int128) (((uint64_t) a << 32) | (uint64_t) b) * (unsigned __int128) n_cells;
  const uint32_t j = (uint32_t) (uint64_t) (product >> 64);
  const uint32_t cell = cells[j];
  const uint32_t n = 4u << level;
  *j_out = j;
  *re = (-2.0 + (double) (cell % n) * ldexp(1.0, -level)) + (x + 2.0) * ldexp(1.0, -(level + 2));
  *im = (-2.0 + (double) (cell / n) * ldexp(1.0, -level)) + (y + 2.0) * ldexp(1.0, -(level + 2));
}

/* The six-draw mapping on the generator's outputs themselves: a, b pick the entry, (x1, x2) and (y1, y2) are the two draws
 * of each coordinate (v = x1 | (x2 >> 11) << 32, the coordinate (v + 1) * 2^-51 - 2). */
static inline void cells_map(int level, const uint32_t *cells, uint32_t n_cells, uint32_t a, uint32_t b, uint32_t x1,
                             uint32_t x2, uint32_t y1, uint32_t y2, uint32_t *j_out, double *re, double *im) {
  const double vx = (double) ((uint64_t) x1 | ((uint64_t) (x2 >> 11) << 32));
  const double vy = (double) ((uint64_t) y1 | ((uint64_t) (y2 >> 11) << 32));
  const double x = (vx + 1.0) * 0x1p-53 * 4.0 - 2.0; /* rocrand_uniform_double * 4 - 2: every step exact */
  const double y = (vy + 1.0) * 0x1p-53 * 4.0 - 2.0;
  cells_point_of(level, cells, n_cells, a, b, x, y, j_out, re, im);
}
