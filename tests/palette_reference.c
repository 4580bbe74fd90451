/* palette_reference.c -- CPU restatement of the palette render (include/cudabrot_amd.h, "Palette render"), for the tests
 * only.  Plain C on the oracle's generator and shortcuts (oracle/liboracle.so), written from the definition, not from
 * the kernels; compiled by the tests with
 *   gcc -O2 -shared -fPIC -ffp-contract=off -mfma [-fopenmp]
 *   palette_draw  one launch: samples_per_thread samples from each generator; c is the sample (julia == 0: a projected
 *                 render, with cardioid / bulb rejection for the Mandelbrot step) or fixed (julia != 0: a Julia render,
 *                 the sample is z_0); every in-canvas point of an accepted orbit with escape index k adds the three
 *                 weights of lut[k] to its pixel in the three planes of hist
 * palette_draw has an OpenMP variant (n_omp > 0: that many workers, atomic increments); without -fopenmp the pragmas are
 * ignored and it runs on one thread. */
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "buddha_oracle.h"

typedef struct {
  uint64_t samples, rejected, never_escaped, too_fast, recorded, iterate_steps, replay_steps, increments;
  /* not a counter of the definition: the replay steps of the accepted orbits whose entry has no weight (what the product
   * kernel adds to skipped_steps on their account) */
  uint64_t zero_entry_steps;
} palette_counters;

/* One step z <- step(c, z); returns |z'|^2 as tested.  degree 2: the reference's step, ship != 0 its Burning Ship
 * variant; degree 3 .. 8: degree - 1 multiplications by z, left to right, then + c. */
static double step(int degree, int ship, double cr, double ci, double *r, double *i) {
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

/* One sample (sr, si): z_0, and c as well unless c is fixed. */
static void one_sample(const orc_dims *d, const orc_iters *it, int degree, int ship, const double *P, int julia,
                       const double *c_fixed, const uint32_t *lut, double sr, double si, uint64_t *hist, int atomic,
                       palette_counters *cnt) {
  const int max = it->max_escape_iterations;
  const double cr = julia ? c_fixed[0] : sr, ci = julia ? c_fixed[1] : si;
  cnt->samples++;
  if (!julia && degree == 2 && !ship && (orc_in_main_cardioid(sr, si) || orc_in_order2_bulb(sr, si))) {
    cnt->rejected++;
    return;
  }
  /* escape index: the first z_{k+1} with |z|^2 > 4 among z_1 .. z_max; z_0 is not tested */
  double r = sr, i = si;
  int k = 0;
  while (k < max && !(step(degree, ship, cr, ci, &r, &i) > 4.0)) k++;
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
  const uint32_t entry = lut[k];
  const uint64_t weight[3] = {entry & 0xffu, (entry >> 8) & 0xffu, (entry >> 16) & 0xffu};
  if ((entry & 0xffffffu) == 0u) cnt->zero_entry_steps += (uint64_t) k + 1u;
  const uint64_t plane_pixels = (uint64_t) d->w * (uint64_t) d->h;
  const double ku = fma(P[2], cr, P[3] * ci);
  const double kv = fma(P[6], cr, P[7] * ci);
  /* replay z_1 .. z_{k+1} */
  r = sr;
  i = si;
  for (int n = 0; n <= k; ++n) {
    (void) step(degree, ship, cr, ci, &r, &i);
    cnt->replay_steps++;
    const double u = fma(P[0], r, fma(P[1], i, ku));
    const double v = fma(P[4], r, fma(P[5], i, kv));
    uint64_t index;
    if (!bin_of(d, u, v, &index)) continue;
    for (int j = 0; j < 3; ++j) {
      if (weight[j] == 0u) continue;
      if (atomic) {
        __atomic_fetch_add(hist + (uint64_t) j * plane_pixels + index, weight[j], __ATOMIC_RELAXED);
      } else {
        hist[(uint64_t) j * plane_pixels + index] += weight[j];
      }
      cnt->increments += weight[j];
    }
  }
}

static void counters_add(palette_counters *dst, const palette_counters *src) {
  uint64_t *a = (uint64_t *) dst;
  const uint64_t *b = (const uint64_t *) src;
  for (size_t k = 0; k < sizeof(palette_counters) / sizeof(uint64_t); ++k) a[k] += b[k];
}

/* samples_per_thread samples from each of states[0 .. n_threads), advancing them; four draws per sample.  hist: three
 * planes of w*h counters; lut: max_escape_iterations entries. */
void palette_draw(const orc_dims *d, uint64_t *hist, const orc_iters *it, int degree, int ship, const double *P, int julia,
                  const double *c_fixed, const uint32_t *lut, orc_xorwow *states, uint64_t n_threads,
                  int samples_per_thread, palette_counters *out, int n_omp) {
  palette_counters total;
  memset(&total, 0, sizeof(total));
  const int workers = n_omp > 0 ? n_omp : 1;
#pragma omp parallel num_threads(workers) if (n_omp > 0)
  {
    palette_counters mine;
    memset(&mine, 0, sizeof(mine));
#pragma omp for schedule(dynamic, 16)
    for (int64_t t = 0; t < (int64_t) n_threads; t++) {
      for (int s = 0; s < samples_per_thread; ++s) {
        const double sr = orc_uniform_double(&states[t]) * 4.0 - 2.0;
        const double si = orc_uniform_double(&states[t]) * 4.0 - 2.0;
        one_sample(d, it, degree, ship, P, julia, c_fixed, lut, sr, si, hist, n_omp > 0, &mine);
      }
    }
#pragma omp critical(palette_counters_sum)
    counters_add(&total, &mine);
  }
  counters_add(out, &total);
}
