/* power_reference.c -- CPU restatement of the Multibrot render (include/cudabrot_amd.h, "Multibrot step"), for the tests
 * only.  Plain C on the oracle's generator (oracle/liboracle.so), written from the definition, not from the kernels;
 * compiled by the tests with
 *   gcc -O2 -shared -fPIC -ffp-contract=off -mfma -fopenmp
 *   power_draw  one launch: samples_per_thread samples from each generator, every visited point plotted at P
 *   power_step  one step of one point
 * power_draw has an OpenMP variant (n_omp > 0: that many workers, atomic increments).
 * Degree 2 is test infrastructure: the canonical z^2 + c sequence of the reference, still without cardioid / bulb
 * rejection, which ties this driver to the oracle. */
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "buddha_oracle.h"

#define CHUNK 60           /* steps between the points the product kernel compares */
#define MAX_BOUNDARIES 512 /* chunk boundaries remembered per sample: max_iter up to 30720 */

typedef struct {
  uint64_t samples, rejected, never_escaped, too_fast, recorded, iterate_steps, replay_steps, increments;
  /* not a counter of the definition: samples whose orbit, at a multiple of CHUNK steps below max, is bit for bit at a
   * point it was at an earlier multiple of CHUNK */
  uint64_t chunk_repeats;
} power_counters;

/* One step z <- z^d + c; returns |z'|^2 as tested. */
double power_step(int d, double cr, double ci, double *r, double *i) {
  double nr, ni;
  if (d == 2) {
    const double ii = (*i) * (*i);
    const double t = fma(*r, *r, -ii);
    nr = cr + t;
    ni = fma((*r) + (*r), *i, ci);
  } else {
    double wr = *r, wi = *i;
    for (int n = 0; n < d - 1; ++n) {
      const double t = wi * (*i);
      const double pr = fma(wr, *r, -t);
      const double s = wi * (*r);
      const double pi = fma(wr, *i, s);
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

/* IncrementPixelCounter's test: 1 and the pixel if the point is on the canvas. */
static inline int pixel_of(const orc_dims *d, double re, double im, uint64_t *index) {
  if ((re < d->min_real) || (im < d->min_imag)) return 0;
  const int col = (int) ((re - d->min_real) / d->delta_real);
  const int row = (int) ((im - d->min_imag) / d->delta_imag);
  if (row < 0 || row >= d->h || col < 0 || col >= d->w) return 0;
  *index = (uint64_t) row * (uint64_t) d->w + (uint64_t) col;
  return 1;
}

static inline int same_bits(double a, double b) { return memcmp(&a, &b, sizeof(a)) == 0; }

static void one_sample(const orc_dims *d, const orc_iters *it, int degree, const double *P, double cr, double ci,
                       uint64_t *hist, int atomic, power_counters *c) {
  c->samples++;
  const int M = it->max_escape_iterations;
  double r = cr, i = ci;
  double br[MAX_BOUNDARIES], bi[MAX_BOUNDARIES];
  int boundaries = 0, repeated = 0;
  int k = M;
  for (int n = 0; n < M; ++n) {
    if (power_step(degree, cr, ci, &r, &i) > 4.0) {
      k = n;
      break;
    }
    if ((n + 1) % CHUNK == 0 && n + 1 < M && !repeated) { /* z_{n+1}, tested and not escaping */
      for (int b = 0; b < boundaries && !repeated; ++b) repeated = same_bits(r, br[b]) && same_bits(i, bi[b]);
      if (boundaries < MAX_BOUNDARIES) {
        br[boundaries] = r;
        bi[boundaries] = i;
        boundaries++;
      }
    }
  }
  if (repeated) c->chunk_repeats++;
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
    const double m = power_step(degree, cr, ci, &r, &i);
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

static void counters_add(power_counters *dst, const power_counters *src) {
  uint64_t *a = (uint64_t *) dst;
  const uint64_t *b = (const uint64_t *) src;
  for (size_t k = 0; k < sizeof(power_counters) / sizeof(uint64_t); ++k) a[k] += b[k];
}

/* samples_per_thread samples from each of states[0 .. n_threads), advancing them; four draws per sample. */
void power_draw(const orc_dims *d, uint64_t *hist, const orc_iters *it, int degree, const double *P, orc_xorwow *states,
                uint64_t n_threads, int samples_per_thread, power_counters *out, int n_omp) {
  power_counters total;
  memset(&total, 0, sizeof(total));
  const int workers = n_omp > 0 ? n_omp : 1;
#pragma omp parallel num_threads(workers) if (n_omp > 0)
  {
    power_counters c;
    memset(&c, 0, sizeof(c));
#pragma omp for schedule(dynamic, 16)
    for (int64_t t = 0; t < (int64_t) n_threads; t++) {
      for (int k = 0; k < samples_per_thread; ++k) {
        const double re = orc_uniform_double(&states[t]) * 4.0 - 2.0;
        const double im = orc_uniform_double(&states[t]) * 4.0 - 2.0;
        one_sample(d, it, degree, P, re, im, hist, n_omp > 0, &c);
      }
    }
#pragma omp critical(power_counters_sum)
    counters_add(&total, &c);
  }
  counters_add(out, &total);
}
