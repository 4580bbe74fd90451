/* julia_reference.c -- CPU restatement of the Julia render (include/cudabrot_amd.h, "Julia render"), for the tests only.
 * Plain C on the oracle's generator (oracle/liboracle.so), written from the definition, not from the kernels; compiled by
 * the tests with
 *   gcc -O2 -shared -fPIC -ffp-contract=off -mfma [-fopenmp]
 *   julia_draw  one launch: samples_per_thread starting points from each generator, the escaping orbits under the fixed
 *               c plotted at P
 *   julia_step  one step of one point
 * julia_draw has an OpenMP variant (n_omp > 0: that many workers, atomic increments); without -fopenmp the pragmas are
 * ignored and it runs on one thread. */
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "buddha_oracle.h"

typedef struct {
  uint64_t samples, rejected, never_escaped, too_fast, recorded, iterate_steps, replay_steps, increments;
} julia_counters;

/* One step z <- step(c, z); returns |z'|^2 as tested.  degree 2: the reference's step, ship != 0 its Burning Ship
 * variant; degree 3 .. 8: degree - 1 multiplications by z, left to right, then + c. */
double julia_step(int degree, int ship, double cr, double ci, double *r, double *i) {
  const double zr = *r, zi = *i;
  double nr, ni;
  if (degree == 2) {
    const double ii = zi * zi;
    nr = cr + fma(zr, zr, -ii);
    ni = ship ? fma(fabs(zr) + fabs(zr), fabs(zi), ci) : fma(zr + zr, zi, ci);
  } else {
    double wr = zr, wi = zi;
    for (int n = 1; n < degree; ++n) {
      const double t = wi * zi;
      const double s = wi * zr;
      const double pr = fma(wr, zr, -t);
      const double pi = fma(wr, zi, s);
      wr = pr;
      wi = pi;
    }
    nr = cr + wr;
    ni = ci + wi;
  }
  *r = nr;
  *i = ni;
  return fma(ni, ni, nr * nr);
}

/* The binning of (u, v): the reference's IncrementPixelCounter with u for re and v for im. */
static int bin_of(const orc_dims *d, double u, double v, uint64_t *index) {
  if (u < d->min_real || v < d->min_imag) return 0;
  const int col = (int) ((u - d->min_real) / d->delta_real);
  const int row = (int) ((v - d->min_imag) / d->delta_imag);
  if (col < 0 || col >= d->w || row < 0 || row >= d->h) return 0;
  *index = (uint64_t) row * (uint64_t) d->w + (uint64_t) col;
  return 1;
}

/* One starting point z_0 = (sr, si). */
static void one_start(const orc_dims *d, const orc_iters *it, int degree, int ship, const double *P, const double *c,
                      double ku, double kv, double sr, double si, uint64_t *hist, int atomic, julia_counters *cnt) {
  const int max = it->max_escape_iterations;
  cnt->samples++;
  /* escape index: the first z_{k+1} with |z|^2 > 4 among z_1 .. z_max; z_0 is not tested */
  double r = sr, i = si;
  int k = 0;
  while (k < max && !(julia_step(degree, ship, c[0], c[1], &r, &i) > 4.0)) k++;
  if (k >= max) {
    cnt->never_escaped++;
    if (max > 0) cnt->iterate_steps += (uint64_t) max;
    return;
  }
  cnt->iterate_steps += (uint64_t) k + 1u;
  if (k < it->min_escape_iterations) {
    cnt->too_fast++;
    return;
  }
  cnt->recorded++;
  /* replay z_1 .. z_{k+1}, each plotted at (z_re, z_im, c_re, c_im) with the fixed c */
  r = sr;
  i = si;
  for (int n = 0; n <= k; ++n) {
    (void) julia_step(degree, ship, c[0], c[1], &r, &i);
    cnt->replay_steps++;
    const double u = fma(P[0], r, fma(P[1], i, ku));
    const double v = fma(P[4], r, fma(P[5], i, kv));
    uint64_t index;
    if (bin_of(d, u, v, &index)) {
      if (atomic) {
        __atomic_fetch_add(hist + index, 1u, __ATOMIC_RELAXED);
      } else {
        hist[index]++;
      }
      cnt->increments++;
    }
  }
}

static void counters_add(julia_counters *dst, const julia_counters *src) {
  uint64_t *a = (uint64_t *) dst;
  const uint64_t *b = (const uint64_t *) src;
  for (size_t k = 0; k < sizeof(julia_counters) / sizeof(uint64_t); ++k) a[k] += b[k];
}

/* samples_per_thread starting points from each of states[0 .. n_threads), advancing them; four draws per sample. */
void julia_draw(const orc_dims *d, uint64_t *hist, const orc_iters *it, int degree, int ship, const double *P,
                const double *c, orc_xorwow *states, uint64_t n_threads, int samples_per_thread, julia_counters *out,
                int n_omp) {
  const double ku = fma(P[2], c[0], P[3] * c[1]); /* from the fixed c */
  const double kv = fma(P[6], c[0], P[7] * c[1]);
  julia_counters total;
  memset(&total, 0, sizeof(total));
  const int workers = n_omp > 0 ? n_omp : 1;
#pragma omp parallel num_threads(workers) if (n_omp > 0)
  {
    julia_counters mine;
    memset(&mine, 0, sizeof(mine));
#pragma omp for schedule(dynamic, 16)
    for (int64_t t = 0; t < (int64_t) n_threads; t++) {
      for (int s = 0; s < samples_per_thread; ++s) {
        const double sr = orc_uniform_double(&states[t]) * 4.0 - 2.0;
        const double si = orc_uniform_double(&states[t]) * 4.0 - 2.0;
        one_start(d, it, degree, ship, P, c, ku, kv, sr, si, hist, n_omp > 0, &mine);
      }
    }
#pragma omp critical(julia_counters_sum)
    counters_add(&total, &mine);
  }
  counters_add(out, &total);
}
