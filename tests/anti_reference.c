/* anti_reference.c -- CPU restatement of the anti-Buddhabrot (include/cudabrot_amd.h, CB_KERNEL_FLAG_ANTI), for the
 * tests only.  Plain C on the oracle's generator (oracle/liboracle.so); compiled by the tests with
 *   gcc -O2 -shared -fPIC -ffp-contract=off -mfma -fopenmp
 * Two modes that must agree bit for bit:
 *   mode 0  the definition: iterate to M, then replay z_1 .. z_M with weight 1;
 *   mode 1  cycle compression at chunk boundaries of 60 steps with the refined Brent save schedule (as draw_anti_kernel):
 *           transient z_1 .. z_{s-1} weight 1, cycle point z_{s+j} weight floor((M - s - j) / p) + 1.
 * Each with an OpenMP variant (n_omp > 0: that many workers, atomic increments). */
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "buddha_oracle.h"

typedef struct {
  uint64_t samples, rejected, never_escaped, too_fast, recorded, iterate_steps, replay_steps, increments,
      skipped_steps;
} anti_counters;

/* What mode 1 decided, per render (the census): how many samples had a cycle detected, how many of those at n == M (the
 * last step allowed), how many with (M - s) % p == 0 / != 0 (the edge of the weight split), the smallest q = (M - s) / p
 * and the largest p.  min_q and max_p are 0 while cycles == 0.  Tests use it to show that an M reaches the branch it is
 * meant to reach. */
typedef struct {
  uint64_t cycles, at_m, rem_zero, rem_nonzero, min_q, max_p;
} anti_census;

#define ANTI_CHUNK 60

static inline double step(double cr, double ci, double *r, double *i, int ship) {
  const double ii = (*i) * (*i);
  const double t = fma(*r, *r, -ii);
  const double nr = cr + t;
  const double ni = ship ? fma(__builtin_fabs(*r) + __builtin_fabs(*r), __builtin_fabs(*i), ci) : fma((*r) + (*r), *i, ci);
  *r = nr;
  *i = ni;
  return fma(ni, ni, nr * nr);
}

/* IncrementPixelCounter's binning with a weight; returns the weight if the point is on the canvas. */
static inline uint64_t add_point(const orc_dims *d, uint64_t *hist, double re, double im, uint64_t w, int atomic) {
  if ((re < d->min_real) || (im < d->min_imag)) return 0;
  const int col = (int) ((re - d->min_real) / d->delta_real);
  const int row = (int) ((im - d->min_imag) / d->delta_imag);
  if (row < 0 || row >= d->h || col < 0 || col >= d->w) return 0;
  uint64_t *p = hist + ((uint64_t) row * (uint64_t) d->w + (uint64_t) col);
  if (atomic) {
    __atomic_fetch_add(p, w, __ATOMIC_RELAXED);
  } else {
    *p += w;
  }
  return w;
}

static int brent_save(uint32_t chunks) {
  int top = 31 - __builtin_clz(chunks);
  return top < 1 || (chunks & ((1u << (top - 1)) - 1u)) == 0u;
}

static int same_bits(double a, double b) { return memcmp(&a, &b, sizeof(double)) == 0; }

static void census_add(anti_census *dst, const anti_census *src) {
  if (src->cycles > 0) {
    if (dst->cycles == 0 || src->min_q < dst->min_q) dst->min_q = src->min_q;
    if (src->max_p > dst->max_p) dst->max_p = src->max_p;
  }
  dst->cycles += src->cycles;
  dst->at_m += src->at_m;
  dst->rem_zero += src->rem_zero;
  dst->rem_nonzero += src->rem_nonzero;
}

/* One sample c; cs (may be NULL) gains what was decided about it. */
static void anti_sample(const orc_dims *d, uint64_t *hist, int max_iter, int ship, int mode, double cr, double ci,
                        int atomic, anti_counters *c, anti_census *cs) {
  const int M = max_iter > 0 ? max_iter : 0;
  double r = cr, i = ci, sr = 0.0, si = 0.0;
  int saved = 0, n = 0, s = M + 1, p = 0;
  c->samples++;
  for (int k = 1; k <= M; ++k) {
    if (step(cr, ci, &r, &i, ship) > 4.0) {
      c->too_fast++;
      c->iterate_steps += (uint64_t) k;
      return;
    }
    n = k;
    if (mode == 1 && k % ANTI_CHUNK == 0) {
      if (saved > 0 && same_bits(r, sr) && same_bits(i, si)) {
        s = saved;
        p = k - saved;
        break;
      }
      if (brent_save((uint32_t) (k / ANTI_CHUNK))) {
        sr = r;
        si = i;
        saved = k;
      }
    }
  }
  c->never_escaped++;
  c->recorded++;
  c->iterate_steps += (uint64_t) M;
  c->replay_steps += (uint64_t) M;
  const int end = p > 0 ? s - 1 + p : M;
  c->skipped_steps += (uint64_t) (M - n) + (uint64_t) (M - end);
  if (cs && p > 0) {
    const anti_census one = {1u, n == M, (M - s) % p == 0, (M - s) % p != 0, (uint64_t) ((M - s) / p), (uint64_t) p};
    census_add(cs, &one);
  }
  r = cr;
  i = ci;
  for (int j = 1; j <= end; ++j) {
    (void) step(cr, ci, &r, &i, ship);
    const uint64_t w = j < s ? 1u : (uint64_t) ((M - j) / p) + 1u;
    c->increments += add_point(d, hist, r, i, w, atomic);
  }
}

static void counters_add(anti_counters *dst, const anti_counters *src) {
  uint64_t *a = (uint64_t *) dst;
  const uint64_t *b = (const uint64_t *) src;
  for (size_t k = 0; k < sizeof(anti_counters) / sizeof(uint64_t); ++k) a[k] += b[k];
}

/* samples_per_thread samples from each of states[0 .. n_threads), advancing them; n_omp > 0: OpenMP.  census (may be
 * NULL) gains the census of these samples. */
void anti_draw(const orc_dims *d, uint64_t *hist, int max_iter, int ship, int mode, orc_xorwow *states,
               uint64_t n_threads, int samples_per_thread, anti_counters *out, int n_omp, anti_census *census) {
  anti_counters total;
  anti_census total_cs;
  memset(&total, 0, sizeof(total));
  memset(&total_cs, 0, sizeof(total_cs));
  const int workers = n_omp > 0 ? n_omp : 1;
#pragma omp parallel num_threads(workers) if (n_omp > 0)
  {
    anti_counters c;
    anti_census cs;
    memset(&c, 0, sizeof(c));
    memset(&cs, 0, sizeof(cs));
#pragma omp for schedule(dynamic, 16)
    for (int64_t t = 0; t < (int64_t) n_threads; t++) {
      for (int k = 0; k < samples_per_thread; ++k) {
        const double re = orc_uniform_double(&states[t]) * 4.0 - 2.0;
        const double im = orc_uniform_double(&states[t]) * 4.0 - 2.0;
        anti_sample(d, hist, max_iter, ship, mode, re, im, n_omp > 0, &c, &cs);
      }
    }
#pragma omp critical(anti_counters_sum)
    {
      counters_add(&total, &c);
      census_add(&total_cs, &cs);
    }
  }
  counters_add(out, &total);
  if (census) census_add(census, &total_cs);
}

/* Given starting points (hand-picked c), one after another. */
void anti_points(const orc_dims *d, uint64_t *hist, int max_iter, int ship, int mode, const double *re,
                 const double *im, uint64_t n, anti_counters *out, anti_census *census) {
  for (uint64_t k = 0; k < n; ++k) anti_sample(d, hist, max_iter, ship, mode, re[k], im[k], 0, out, census);
}
