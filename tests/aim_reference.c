/* aim_reference.c -- CPU restatement of the aimed render (include/cudabrot_amd.h, "Aimed render"), for the tests only.
 * Plain C on the oracle's generator and shortcuts (oracle/liboracle.so), written from the definition, not from the kernels;
 * the steps, the projection and the binning are tests/plot_reference.c's and the save schedule tests/bounded_reference.c's,
 * included here, and the grid's arithmetic tests/cells_reference.h's.  Compiled by the tests with
 *   gcc -O2 -shared -fPIC -ffp-contract=off -mfma [-fopenmp]
 *   aim_launch  one launch: a SOURCE (cells NULL: four draws per sample, uniform; else six, from the list, mapped as
 *               tests/focus_reference.c maps them), an un-aimed render (escaping or bounded orbits, a step, c sampled or
 *               fixed) and a SINK (hist: the draw; else mask: the probe).
 *   aim_map     the six-draw mapping alone, on given generator outputs.
 * A bounded orbit is replayed in one of two modes that must agree bit for bit, the probe's mask and replay_steps included:
 *   mode 0  the definition: all M points, each with weight 1;
 *   mode 1  cycle compression at chunk boundaries of 60 steps with the refined Brent save schedule: the transient with
 *           weight 1, then ONE period with the exact integer weights.
 * It notes, per run, what a case must reach (aim_extra).  OpenMP variant: n_omp > 0 workers, atomic adds and bit sets. */
#include "bounded_reference.c"
#include "cells_reference.h"

typedef struct {
  uint64_t samples, rejected, never_escaped, too_fast, recorded, iterate_steps, replay_steps, increments, skipped_steps;
} aim_counters;

/* marking: samples that mark a cell (the probe); plotted: samples whose orbit is plotted (accepted escaping orbits, or
 * bounded samples); cycles, no_cycle: bounded samples by whether the schedule finds their orbit on an exact cycle;
 * both_weights: cycles in which both weights q + 1 and q occur; in_canvas, off_canvas: the plotted points, by weight, by
 * whether they are binned (the probe: the points up to the one that ends the replay). */
typedef struct {
  uint64_t marking, plotted, cycles, no_cycle, both_weights, in_canvas, off_canvas;
} aim_extra;

void aim_map(int level, const uint32_t *cells, uint32_t n_cells, uint32_t a, uint32_t b, uint32_t x1, uint32_t x2,
             uint32_t y1, uint32_t y2, uint32_t *j_out, double *re, double *im) {
  cells_map(level, cells, n_cells, a, b, x1, x2, y1, y2, j_out, re, im);
}

/* One sample (sr, si): z_0, and c as well unless c is fixed.  hist != NULL: the draw; else the probe into mask. */
static void aim_sample(const orc_dims *d, const orc_iters *it, int bounded, int formula, int degree, int ship, int reject,
                       const double *P, const double *c_fixed, int mode, double sr, double si, uint64_t *hist,
                       uint32_t *mask, int level, int atomic, aim_counters *cnt, aim_extra *ex) {
  const int M = it->max_escape_iterations > 0 ? it->max_escape_iterations : 0;
  const double cr = c_fixed ? c_fixed[0] : sr, ci = c_fixed ? c_fixed[1] : si;
  cnt->samples++;
  if (reject && (orc_in_main_cardioid(sr, si) || orc_in_order2_bulb(sr, si))) {
    cnt->rejected++;
    return;
  }
  /* iterate: k steps made without an escape; the schedule's cycle z_s .. z_{s+p-1}, if it finds one (bounded kind) */
  double r = sr, i = si, saved_r = 0.0, saved_i = 0.0;
  int saved = 0, k = 0, escaped = 0, s = M + 1, p = 0;
  while (k < M) {
    if (plot_step(formula, degree, ship, cr, ci, &r, &i) > 4.0) {
      escaped = 1;
      break;
    }
    k++;
    if (bounded && p == 0 && k % CHUNK == 0) {
      if (saved > 0 && same_bits(r, saved_r) && same_bits(i, saved_i)) {
        s = saved;
        p = k - saved;
        if (mode == 1) break;
      } else if (bounded_brent_save((uint32_t) (k / CHUNK))) {
        saved_r = r;
        saved_i = i;
        saved = k;
      }
    }
  }
  int naive; /* the plotted orbit z_1 .. z_naive */
  if (bounded) {
    if (escaped) { /* z_{k+1} escapes: nothing plotted */
      cnt->too_fast++;
      cnt->iterate_steps += (uint64_t) k + 1u;
      return;
    }
    cnt->never_escaped++;
    cnt->iterate_steps += (uint64_t) M;
    naive = M;
    if (p > 0) {
      ex->cycles++;
      ex->both_weights += (M - s) % p < p - 1;
    } else {
      ex->no_cycle++;
    }
  } else {
    if (!escaped) {
      cnt->never_escaped++;
      cnt->iterate_steps += (uint64_t) M;
      return;
    }
    cnt->iterate_steps += (uint64_t) k + 1u;
    if (k < it->min_escape_iterations) {
      cnt->too_fast++;
      return;
    }
    naive = k + 1;
  }
  ex->plotted++;
  const int compressed = bounded && mode == 1 && p > 0;
  const int end = compressed ? s - 1 + p : naive;
  if (bounded && mode == 1 && hist) cnt->skipped_steps += (uint64_t) (M - k) + (uint64_t) (M - end);
  if (hist) {
    cnt->recorded++;
    cnt->replay_steps += (uint64_t) naive;
  }
  const double ku = fma(P[2], cr, P[3] * ci); /* once per sample */
  const double kv = fma(P[6], cr, P[7] * ci);
  r = sr;
  i = si;
  for (int j = 1; j <= end; ++j) {
    (void) plot_step(formula, degree, ship, cr, ci, &r, &i);
    const uint64_t w = (compressed && j >= s) ? (uint64_t) ((M - j) / p) + 1u : 1u;
    const double u = fma(P[0], r, fma(P[1], i, ku));
    const double v = fma(P[4], r, fma(P[5], i, kv));
    uint64_t index;
    if (!bin_of(d, u, v, &index)) {
      ex->off_canvas += hist ? w : 1u;
      continue;
    }
    if (!hist) { /* the probe: the first in-canvas point marks the SAMPLE's cell and ends the replay */
      const uint32_t cell = cells_cell_of(level, sr, si);
      if (atomic) {
        __atomic_fetch_or(mask + (cell >> 5), 1u << (cell & 31u), __ATOMIC_RELAXED);
      } else {
        mask[cell >> 5] |= 1u << (cell & 31u);
      }
      ex->in_canvas++;
      ex->marking++;
      cnt->recorded++;
      cnt->replay_steps += (uint64_t) j;
      return;
    }
    ex->in_canvas += w;
    if (atomic) {
      __atomic_fetch_add(hist + index, w, __ATOMIC_RELAXED);
    } else {
      hist[index] += w;
    }
    cnt->increments += w;
  }
  if (!hist) cnt->replay_steps += (uint64_t) naive; /* no point on the canvas: all of them made */
}

/* samples_per_thread samples from each of states[0 .. n_threads), advancing them.  cells != NULL: six draws per sample from
 * the list; else four, uniform.  hist != NULL: the draw; else the probe into mask.  reject: cardioid and bulb (the caller's
 * choice: the Mandelbrot step on a sampled c of the escaping kind).  out and extra gain what these samples add. */
void aim_launch(const orc_dims *d, uint64_t *hist, uint32_t *mask, const orc_iters *it, int bounded, int formula, int degree,
                int ship, int reject, const double *P, const double *c_fixed, int mode, orc_xorwow *states,
                uint64_t n_threads, int samples_per_thread, int level, const uint32_t *cells, uint32_t n_cells,
                aim_counters *out, aim_extra *extra, int n_omp) {
  aim_counters total;
  aim_extra total_ex;
  memset(&total, 0, sizeof(total));
  memset(&total_ex, 0, sizeof(total_ex));
  const int workers = n_omp > 0 ? n_omp : 1;
#pragma omp parallel num_threads(workers) if (n_omp > 0)
  {
    aim_counters mine;
    aim_extra mine_ex;
    memset(&mine, 0, sizeof(mine));
    memset(&mine_ex, 0, sizeof(mine_ex));
#pragma omp for schedule(dynamic, 16)
    for (int64_t t = 0; t < (int64_t) n_threads; t++) {
      for (int k = 0; k < samples_per_thread; ++k) {
        double sr, si;
        if (cells) {
          const uint32_t a = orc_xorwow_next(&states[t]);
          const uint32_t b = orc_xorwow_next(&states[t]);
          const double x = orc_uniform_double(&states[t]) * 4.0 - 2.0;
          const double y = orc_uniform_double(&states[t]) * 4.0 - 2.0;
          uint32_t j;
          cells_point_of(level, cells, n_cells, a, b, x, y, &j, &sr, &si);
        } else {
          sr = orc_uniform_double(&states[t]) * 4.0 - 2.0;
          si = orc_uniform_double(&states[t]) * 4.0 - 2.0;
        }
        aim_sample(d, it, bounded, formula, degree, ship, reject, P, c_fixed, mode, sr, si, hist, mask, level, n_omp > 0,
                   &mine, &mine_ex);
      }
    }
#pragma omp critical(aim_counters_sum)
    {
      bounded_add((uint64_t *) &total, (const uint64_t *) &mine, sizeof(total) / sizeof(uint64_t));
      bounded_add((uint64_t *) &total_ex, (const uint64_t *) &mine_ex, sizeof(total_ex) / sizeof(uint64_t));
    }
  }
  bounded_add((uint64_t *) out, (const uint64_t *) &total, sizeof(total) / sizeof(uint64_t));
  bounded_add((uint64_t *) extra, (const uint64_t *) &total_ex, sizeof(total_ex) / sizeof(uint64_t));
}
