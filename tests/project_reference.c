/* project_reference.c -- CPU restatement of the projected render (include/cudabrot_amd.h, "Projected render"), for the
 * tests only.  Plain C on the oracle's generator and shortcuts (oracle/liboracle.so), written from the definition, not
 * from the kernels; compiled by the tests with
 *   gcc -O2 -shared -fPIC -ffp-contract=off -mfma -fopenmp
 *   project_draw   one launch: samples_per_thread samples from each generator, every visited point plotted at P
 *   project_point  the plot of one point alone: (u, v) of (z, c) under P
 * project_draw has an OpenMP variant (n_omp > 0: that many workers, atomic increments). */
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "buddha_oracle.h"

typedef struct {
  uint64_t samples, rejected, never_escaped, too_fast, recorded, iterate_steps, replay_steps, increments;
} project_counters;

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

/* P is P[2][4] row-major: rows (u, v), columns (z_re, z_im, c_re, c_im). */
void project_point(const double *P, double zr, double zi, double cr, double ci, double *u, double *v) {
  const double ku = fma(P[2], cr, P[3] * ci);
  const double kv = fma(P[6], cr, P[7] * ci);
  *u = fma(P[0], zr, fma(P[1], zi, ku));
  *v = fma(P[4], zr, fma(P[5], zi, kv));
}

static void one_sample(const orc_dims *d, const orc_iters *it, int ship, const double *P, double cr, double ci,
                       uint64_t *hist, int atomic, project_counters *c) {
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
  c->recorded++;
  const double ku = fma(P[2], cr, P[3] * ci); /* once per sample */
  const double kv = fma(P[6], cr, P[7] * ci);
  r = cr;
  i = ci;
  for (;;) {
    const double m = step(cr, ci, &r, &i, ship);
    const double u = fma(P[0], r, fma(P[1], i, ku));
    const double v = fma(P[4], r, fma(P[5], i, kv));
    uint64_t index;
    c->replay_steps++;
    if (pixel_of(d, u, v, &index)) {
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

static void counters_add(project_counters *dst, const project_counters *src) {
  uint64_t *a = (uint64_t *) dst;
  const uint64_t *b = (const uint64_t *) src;
  for (size_t k = 0; k < sizeof(project_counters) / sizeof(uint64_t); ++k) a[k] += b[k];
}

/* samples_per_thread samples from each of states[0 .. n_threads), advancing them; four draws per sample. */
void project_draw(const orc_dims *d, uint64_t *hist, const orc_iters *it, int ship, const double *P,
                  orc_xorwow *states, uint64_t n_threads, int samples_per_thread, project_counters *out, int n_omp) {
  project_counters total;
  memset(&total, 0, sizeof(total));
  const int workers = n_omp > 0 ? n_omp : 1;
#pragma omp parallel num_threads(workers) if (n_omp > 0)
  {
    project_counters c;
    memset(&c, 0, sizeof(c));
#pragma omp for schedule(dynamic, 16)
    for (int64_t t = 0; t < (int64_t) n_threads; t++) {
      for (int k = 0; k < samples_per_thread; ++k) {
        const double re = orc_uniform_double(&states[t]) * 4.0 - 2.0;
        const double im = orc_uniform_double(&states[t]) * 4.0 - 2.0;
        one_sample(d, it, ship, P, re, im, hist, n_omp > 0, &c);
      }
    }
#pragma omp critical(project_counters_sum)
    counters_add(&total, &c);
  }
  counters_add(out, &total);
}
