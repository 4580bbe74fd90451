/* phoenix_reference.c -- CPU restatement of the Phoenix render (include/cudabrot_amd.h, "Phoenix render"), for the tests
 * only.  Plain C on the oracle's generator (oracle/liboracle.so), written from the definition, not from the kernels;
 * compiled by the tests with
 *   gcc -O2 -shared -fPIC -ffp-contract=off -mfma [-fopenmp]
 *   phoenix_step   one step of one state (z, y)
 *   phoenix_draw   one launch: samples_per_thread samples from each generator; c is the sample (c_fixed NULL) or fixed (the
 *                  sample is then z_0 alone).  Beside the definition's counters it returns two executed-work discounts of
 *                  the round scheduler's early-out, which are no part of the definition: at every k
 *                  that is a multiple of CHUNK with k < max the orbit is compared with the saved point, and where it is
 *                  not found there the point is saved after 1, 2, 3, 4, 6, 8, 12 ... chunks; a sample found at k discounts
 *                  max - k steps.  skipped_state compares the whole state (z, y), skipped_z_only z alone, everything else
 *                  the same.
 * phoenix_draw has an OpenMP variant (n_omp > 0: that many workers, atomic increments); without -fopenmp the pragmas are
 * ignored and it runs on one thread. */
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "buddha_oracle.h"

#define CHUNK 60 /* steps between the points the product kernel compares */

typedef struct {
  uint64_t samples, rejected, never_escaped, too_fast, recorded, iterate_steps, replay_steps, increments;
  /* not counters of the definition: the two discounts, and the samples each rule found */
  uint64_t skipped_state, skipped_z_only, cycles_state, cycles_z_only;
} phoenix_counters;

/* (z, y) <- step; returns |z'|^2 as tested.  The definition's sequence: mandel_step's four operations, then four fused. */
double phoenix_step(double cr, double ci, double p_re, double p_im, double *r, double *i, double *y_re, double *y_im) {
  const double zr = *r, zi = *i;
  const double ii = zi * zi;
  const double t = fma(zr, zr, -ii);
  double nr = cr + t;
  double ni = fma(zr + zr, zi, ci);
  nr = fma(p_re, *y_re, nr);
  nr = fma(-p_im, *y_im, nr);
  ni = fma(p_re, *y_im, ni);
  ni = fma(p_im, *y_re, ni);
  *y_re = zr;
  *y_im = zi;
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

static int same_bits(double a, double b) { return memcmp(&a, &b, sizeof(a)) == 0; }

/* The scheduler's save rule: the chunks done have no set bit below their top two. */
static int saves_after(unsigned chunks) {
  int top = 0;
  while ((chunks >> (top + 1)) != 0u) top++;
  return top < 1 || (chunks & ((1u << (top - 1)) - 1u)) == 0u;
}

/* One sample (sr, si): z_0, and c as well unless c is fixed. */
static void one_sample(const orc_dims *d, const orc_iters *it, const double *P, const double *c_fixed, const double *p,
                       double sr, double si, uint64_t *hist, int atomic, phoenix_counters *cnt) {
  const int max = it->max_escape_iterations;
  const double cr = c_fixed ? c_fixed[0] : sr, ci = c_fixed ? c_fixed[1] : si;
  cnt->samples++;
  /* escape index: the first z_{k+1} with |z|^2 > 4 among z_1 .. z_max; z_0 is not tested */
  double r = sr, i = si, yr = 0.0, yi = 0.0;
  double s_r = 0.0, s_i = 0.0, s_yr = 0.0, s_yi = 0.0; /* the saved state */
  int saved = 0, found_state = 0, found_z = 0;
  int k = 0;
  while (k < max && !(phoenix_step(cr, ci, p[0], p[1], &r, &i, &yr, &yi) > 4.0)) {
    k++;
    if (k % CHUNK == 0 && k < max) { /* (z_k, y_k), tested and not escaping */
      if (saved) {
        const int z_same = same_bits(r, s_r) && same_bits(i, s_i);
        if (z_same && !found_z) found_z = k;
        if (z_same && same_bits(yr, s_yr) && same_bits(yi, s_yi) && !found_state) found_state = k;
      }
      if (saves_after((unsigned) (k / CHUNK))) {
        s_r = r;
        s_i = i;
        s_yr = yr;
        s_yi = yi;
        saved = 1;
      }
    }
  }
  if (found_state) {
    cnt->cycles_state++;
    cnt->skipped_state += (uint64_t) (max - found_state);
  }
  if (found_z) {
    cnt->cycles_z_only++;
    cnt->skipped_z_only += (uint64_t) (max - found_z);
  }
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
  const double ku = fma(P[2], cr, P[3] * ci); /* once per sample */
  const double kv = fma(P[6], cr, P[7] * ci);
  /* replay z_1 .. z_{k+1} from (z_0, y_0 = 0) */
  r = sr;
  i = si;
  yr = 0.0;
  yi = 0.0;
  for (int n = 0; n <= k; ++n) {
    (void) phoenix_step(cr, ci, p[0], p[1], &r, &i, &yr, &yi);
    cnt->replay_steps++;
    const double u = fma(P[0], r, fma(P[1], i, ku));
    const double v = fma(P[4], r, fma(P[5], i, kv));
    uint64_t index;
    if (!bin_of(d, u, v, &index)) continue;
    if (atomic) {
      __atomic_fetch_add(hist + index, 1u, __ATOMIC_RELAXED);
    } else {
      hist[index] += 1u;
    }
    cnt->increments++;
  }
}

static void counters_add(phoenix_counters *dst, const phoenix_counters *src) {
  uint64_t *a = (uint64_t *) dst;
  const uint64_t *b = (const uint64_t *) src;
  for (size_t k = 0; k < sizeof(phoenix_counters) / sizeof(uint64_t); ++k) a[k] += b[k];
}

/* samples_per_thread samples from each of states[0 .. n_threads), advancing them; four draws per sample.  hist: one plane
 * of w*h counters; P: P[2][4] row-major; c_fixed NULL: c is the sample; p: (p_re, p_im). */
void phoenix_draw(const orc_dims *d, uint64_t *hist, const orc_iters *it, const double *P, const double *c_fixed,
                  const double *p, orc_xorwow *states, uint64_t n_threads, int samples_per_thread, phoenix_counters *out,
                  int n_omp) {
  phoenix_counters total;
  memset(&total, 0, sizeof(total));
  const int workers = n_omp > 0 ? n_omp : 1;
#pragma omp parallel num_threads(workers) if (n_omp > 0)
  {
    phoenix_counters mine;
    memset(&mine, 0, sizeof(mine));
#pragma omp for schedule(dynamic, 16)
    for (int64_t t = 0; t < (int64_t) n_threads; t++) {
      for (int s = 0; s < samples_per_thread; ++s) {
        const double sr = orc_uniform_double(&states[t]) * 4.0 - 2.0;
        const double si = orc_uniform_double(&states[t]) * 4.0 - 2.0;
        one_sample(d, it, P, c_fixed, p, sr, si, hist, n_omp > 0, &mine);
      }
    }
#pragma omp critical(phoenix_counters_sum)
    counters_add(&total, &mine);
  }
  counters_add(out, &total);
}
