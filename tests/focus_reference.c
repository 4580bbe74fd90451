/* focus_reference.c -- CPU restatement of the focused render (include/cudabrot_amd.h, "Focused render"), for the tests
 * only.  Plain C on the oracle's generator and shortcuts (oracle/liboracle.so), written from the definition, not from the
 * kernels; compiled by the tests with
 *   gcc -O2 -shared -fPIC -ffp-contract=off -mfma -fopenmp
 *   focus_probe  the pilot pass: the mask of the cells whose samples have an accepted orbit with an in-canvas point
 *   focus_cells  the mask dilated by d cells (Chebyshev), as an ascending list
 *   focus_draw   the draw from a cell list (six draws per sample), or -- cells == NULL -- a normal render
 *   focus_map    the six-draw mapping alone, on given generator outputs
 * The grid's arithmetic -- the cell that holds a point, the six-draw mapping -- is tests/cells_reference.h's.
 * Each launch has an OpenMP variant (n_omp > 0: that many workers, atomic increments and bit sets). */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "buddha_oracle.h"
#include "cells_reference.h"

typedef struct {
  uint64_t samples, rejected, never_escaped, too_fast, recorded, iterate_steps, replay_steps, increments;
} focus_counters;

static inline double step(double cr, double ci, double *r, double *i, int ship) {
  const double ii = (*i) * (*i);
  const double t = fma(*r, *r, -ii);
  const double nr = cr + t;
  const double ni = ship ? fma(__builtin_fabs(*r) + __builtin_fabs(*r), __builtin_fabs(*i), ci) : fma((*r) + (*r), *i, ci);
  *r = nr;
  *i = ni;
  return fma(ni, ni, nr * nr);
}

/* IncrementPixelCounter's test: 1 and the pixel if the point is on the canvas. */
static inline int pixel_of(const orc_dims *d, double re, double im, uint64_t *index) {
  if ((re < d->min_real) || (im < d->min_imag)) return 0;
  const int col = (int) ((re - d->min_real) / d->delta_real);
  const int row = (int) ((im - d->min_imag) / d->delta_imag);
  if (row < 0 || row >= d->h || col < 0 || col >= d->w) return 0;
  *index = (uint64_t) row * (uint64_t) d->w + (uint64_t) col;
  return 1;
}

void focus_map(int level, const uint32_t *cells, uint32_t n_cells, uint32_t a, uint32_t b, uint32_t x1, uint32_t x2,
               uint32_t y1, uint32_t y2, uint32_t *j_out, double *re, double *im) {
  cells_map(level, cells, n_cells, a, b, x1, x2, y1, y2, j_out, re, im);
}

/* One sample c through the reference's path.  hist != NULL: the draw; else mask != NULL: the probe. */
static void one_sample(const orc_dims *d, const orc_iters *it, int ship, double cr, double ci, uint64_t *hist,
                       uint32_t *mask, int level, int atomic, focus_counters *c) {
  c->samples++;
  if (!ship && (orc_in_main_cardioid(cr, ci) || orc_in_order2_bulb(cr, ci))) {
    c->rejected++;
    return;
  }
  const int M = it->max_escape_iterations;
  double r = cr, i = ci;
  int k = M;
  for (int n = 0; n < M; ++n) {
    if (step(cr, ci, &r, &i, ship) > 4.0) {
      k = n;
      break;
    }
  }
  if (k >= M) {
    c->never_escaped++;
    c->iterate_steps += (uint64_t) (M > 0 ? M : 0);
    return;
  }
  c->iterate_steps += (uint64_t) k + 1u;
  if (k < it->min_escape_iterations) {
    c->too_fast++;
    return;
  }
  if (hist) c->recorded++;
  r = cr;
  i = ci;
  for (;;) {
    const double m = step(cr, ci, &r, &i, ship);
    uint64_t index;
    c->replay_steps++;
    if (pixel_of(d, r, i, &index)) {
      if (!hist) { /* the probe: the first in-canvas point marks the sample's cell and ends the replay */
        const uint32_t cell = cells_cell_of(level, cr, ci);
        if (atomic) {
          __atomic_fetch_or(mask + (cell >> 5), 1u << (cell & 31u), __ATOMIC_RELAXED);
        } else {
          mask[cell >> 5] |= 1u << (cell & 31u);
        }
        c->recorded++;
        return;
      }
      if (atomic) {
        __atomic_fetch_add(hist + index, 1u, __ATOMIC_RELAXED);
      } else {
        hist[index] += 1u;
      }
      c->increments++;
    }
    if (m > 4.0) return;
  }
}

static void counters_add(focus_counters *dst, const focus_counters *src) {
  uint64_t *a = (uint64_t *) dst;
  const uint64_t *b = (const uint64_t *) src;
  for (size_t k = 0; k < sizeof(focus_counters) / sizeof(uint64_t); ++k) a[k] += b[k];
}

/* samples_per_thread samples from each of states[0 .. n_threads), advancing them.  cells != NULL: six draws per sample
 * from the list; else four, uniform.  hist != NULL: the draw; else the probe into mask. */
static void launch(const orc_dims *d, const orc_iters *it, int ship, orc_xorwow *states, uint64_t n_threads,
                   int samples_per_thread, int level, const uint32_t *cells, uint32_t n_cells, uint64_t *hist,
                   uint32_t *mask, focus_counters *out, int n_omp) {
  focus_counters total;
  memset(&total, 0, sizeof(total));
  const int workers = n_omp > 0 ? n_omp : 1;
#pragma omp parallel num_threads(workers) if (n_omp > 0)
  {
    focus_counters c;
    memset(&c, 0, sizeof(c));
#pragma omp for schedule(dynamic, 16)
    for (int64_t t = 0; t < (int64_t) n_threads; t++) {
      for (int k = 0; k < samples_per_thread; ++k) {
        double re, im;
        if (cells) {
          const uint32_t a = orc_xorwow_next(&states[t]);
          const uint32_t b = orc_xorwow_next(&states[t]);
          const double x = orc_uniform_double(&states[t]) * 4.0 - 2.0;
          const double y = orc_uniform_double(&states[t]) * 4.0 - 2.0;
          uint32_t j;
          cells_point_of(level, cells, n_cells, a, b, x, y, &j, &re, &im);
        } else {
          re = orc_uniform_double(&states[t]) * 4.0 - 2.0;
          im = orc_uniform_double(&states[t]) * 4.0 - 2.0;
        }
        one_sample(d, it, ship, re, im, hist, mask, level, n_omp > 0, &c);
      }
    }
#pragma omp critical(focus_counters_sum)
    counters_add(&total, &c);
  }
  counters_add(out, &total);
}

void focus_probe(const orc_dims *d, const orc_iters *it, int ship, orc_xorwow *states, uint64_t n_threads,
                 int samples_per_thread, int level, uint32_t *mask, focus_counters *out, int n_omp) {
  launch(d, it, ship, states, n_threads, samples_per_thread, level, NULL, 0, NULL, mask, out, n_omp);
}

void focus_draw(const orc_dims *d, uint64_t *hist, const orc_iters *it, int ship, orc_xorwow *states,
                uint64_t n_threads, int samples_per_thread, int level, const uint32_t *cells, uint32_t n_cells,
                focus_counters *out, int n_omp) {
  launch(d, it, ship, states, n_threads, samples_per_thread, level, cells, n_cells, hist, NULL, out, n_omp);
}

/* The mask dilated by `dilate` cells in the Chebyshev metric, clipped at the grid's edge: every set cell marks the box
 * around it; then the marked cells in ascending order.  cells_out must hold n * n entries.  Returns their number. */
uint32_t focus_cells(int level, const uint32_t *mask, int dilate, uint32_t *cells_out) {
  const long n = 4L << level;
  unsigned char *grid = (unsigned char *) calloc((size_t) n * (size_t) n, 1);
  uint32_t found = 0;
  for (long row = 0; row < n; ++row) {
    for (long col = 0; col < n; ++col) {
      const uint64_t index = (uint64_t) row * (uint64_t) n + (uint64_t) col;
      if (!((mask[index >> 5] >> (index & 31u)) & 1u)) continue;
      for (long y = row - dilate < 0 ? 0 : row - dilate; y <= row + dilate && y < n; ++y) {
        for (long x = col - dilate < 0 ? 0 : col - dilate; x <= col + dilate && x < n; ++x) grid[y * n + x] = 1;
      }
    }
  }
  for (long index = 0; index < n * n; ++index) {
    if (grid[index]) cells_out[found++] = (uint32_t) index;
  }
  free(grid);
  return found;
}
