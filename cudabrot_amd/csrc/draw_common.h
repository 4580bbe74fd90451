// draw_common.h -- pieces shared by all draw kernels: the asm step and the chunk helpers of draw_wave.hip and
// draw_wide.hip, the canvas, the generator's load and store.  What the kernels with one reference thread per lane share
// beyond that (kernels.hip, draw_anti.hip, draw_focus.hip, draw_plot.hip) is in draw_rounds.h.
#pragma once

#include "device_math.h"
#include "kernels.h"

namespace cb {

// draw_wave.hip and draw_wide.hip are compiled twice: as is, and with -DCB_BURNING_SHIP for the reference's
// RENDER_BURNING_SHIP variant (cudabrot.cu:15-17), where the cross term 2*real*imag of every step takes the
// magnitudes of its operands: a pair of |.| operand modifiers on one instruction of the step.
#ifdef CB_BURNING_SHIP
#define CB_AL "|"
#define CB_AR "|"
#else
#define CB_AL ""
#define CB_AR ""
#endif

// kChunk as text, for the asm blocks (VOP2 / VOPC e32: the chunk length may be a literal)
#define CB_CHUNK_S "60"
static_assert(kChunk == 60, "CB_CHUNK_S spells kChunk");

struct Orbit {
  double cr, ci, r, i;
};

// This lane's bit of a wave-uniform mask, as a predicate: the mask itself becomes the condition
// register (s_and_saveexec), no vector instruction.
__device__ __forceinline__ bool lane_in(unsigned long long mask) {
  return __builtin_amdgcn_inverse_ballot_w64(mask);
}
__device__ __forceinline__ unsigned long long uniform_u64(unsigned long long v) {
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t) v);
  const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t) (v >> 32));
  return ((unsigned long long) hi << 32) | lo;
}

// The kernel's arguments, read afresh: a scalar load from the argument segment at the point of use
// instead of a value held in (and spilled from) scalar registers since the kernel began.
typedef const DrawArgs __attribute__((address_space(4))) *KernelArgs;
__device__ __forceinline__ KernelArgs fresh_args() {
  KernelArgs p = (KernelArgs) __builtin_amdgcn_kernarg_segment_ptr();
  asm volatile("" : "+s"(p));
  return p;
}

// ---- one orbit per lane under EXEC (HEAD, MID, the last short chunk of LONG) -----------------------
//
// One z <- z^2 + c step on the lanes in EXEC, on DOUBLED coordinates, in the order of
// device_math.h's mandel_step2:
//   a = i*i; a = fma(r,r,-a); i = fma(r,i,ci); r = fma(a,0.5,cr); a = r*r; a = fma(i,i,a)
// then EXEC &= !(16.0 < a) (v_cmpx: a lane leaves at its escape, cudabrot.cu:336), after adding the
// number of lanes that execute the step to the scalar counter.  k16 is 16.0 in a scalar pair.
#define CB_STEP                                       \
  "s_bcnt1_i32_b64 %[tmp], exec\n\t"                  \
  "v_mul_f64 %[a], %[i], %[i]\n\t"                    \
  "s_add_u32 %[cnt], %[cnt], %[tmp]\n\t"              \
  "v_fma_f64 %[a], %[r], %[r], -%[a]\n\t"             \
  "v_fma_f64 %[i], " CB_AL "%[r]" CB_AR ", " CB_AL "%[i]" CB_AR ", %[ci]\n\t"             \
  "v_fma_f64 %[r], %[a], 0.5, %[cr]\n\t"              \
  "v_mul_f64 %[a], %[r], %[r]\n\t"                    \
  "v_fma_f64 %[a], %[i], %[i], %[a]\n\t"              \
  "v_cmpx_nlt_f64_e32 vcc, %[k16], %[a]\n\t"
// The step without |z|^2 and the test: MID re-derives HEAD's iterations, which are known not to escape.
#define CB_STEP_NOTEST                                \
  "v_mul_f64 %[a], %[i], %[i]\n\t"                    \
  "v_fma_f64 %[a], %[r], %[r], -%[a]\n\t"             \
  "v_fma_f64 %[i], " CB_AL "%[r]" CB_AR ", " CB_AL "%[i]" CB_AR ", %[ci]\n\t"             \
  "v_fma_f64 %[r], %[a], 0.5, %[cr]\n\t"

// n steps (wave-uniform run-time count) on the lanes of `mask`, leaving early once every lane has
// escaped.  Returns the lanes that escaped; r, i of the others advance by n iterations; lane_steps
// receives the executed lane-steps (a lane that escapes at its j-th step counts j).
__device__ __forceinline__ unsigned long long iterate_steps(unsigned long long mask, uint32_t n,
                                                            Orbit &o, uint32_t &lane_steps) {
  unsigned long long save, escaped;
  uint32_t cnt, tmp, ctr;
  double a;
  const double k16 = 16.0;
  asm volatile(
      "s_mov_b64 %[save], exec\n\t"
      "s_mov_b32 %[cnt], 0\n\t"
      "s_mov_b64 exec, %[mask]\n\t"
      "s_mov_b32 %[ctr], %[n]\n\t"
      "s_cmp_eq_u32 %[n], 0\n\t"
      "s_cbranch_scc1 2f\n\t"
      "1:\n\t"
      CB_STEP
      "s_cbranch_execz 2f\n\t"
      "s_sub_u32 %[ctr], %[ctr], 1\n\t"
      "s_cmp_lg_u32 %[ctr], 0\n\t"
      "s_cbranch_scc1 1b\n\t"
      "2:\n\t"
      "s_andn2_b64 %[esc], %[mask], exec\n\t"
      "s_mov_b64 exec, %[save]\n\t"
      "s_nop 4\n\t"
      : [r] "+v"(o.r), [i] "+v"(o.i), [a] "=&v"(a), [save] "=&s"(save),
        [esc] "=&s"(escaped), [cnt] "=&s"(cnt), [tmp] "=&s"(tmp), [ctr] "=&s"(ctr)
      : [mask] "s"(mask), [n] "s"(n), [cr] "v"(o.cr), [ci] "v"(o.ci), [k16] "s"(k16)
      : "vcc", "scc");
  lane_steps = cnt;
  return escaped;
}

// The exact decision for the lanes of `doubt`: did the orbit with starting point (cr, ci) escape during the
// kChunk iterations after its first `done` ones (lane-wise)?  Recomputed from z0 = c with the reference's
// test after every step (cudabrot.cu:326-337); the steps before the chunk passed that test when they were
// made.  Rare (draw_wave.hip, iterate_chunk2_sparse), so plain C++ under EXEC: same arithmetic as the asm
// (device_math.h).
__device__ __forceinline__ unsigned long long verify_chunk_escape(unsigned long long doubt, const Orbit &o,
                                                                  int done) {
  bool escaped = false;
  if (lane_in(doubt)) {
    double r = o.cr, i = o.ci;
    for (int k = 0; k < done; ++k) {
#ifdef CB_BURNING_SHIP
      (void) mandel_step2_ship(o.cr, o.ci, r, i);
#else
      (void) mandel_step2(o.cr, o.ci, r, i);
#endif
    }
    for (int k = 0; k < kChunk && !escaped; ++k) {
#ifdef CB_BURNING_SHIP
      escaped = mandel_step2_ship(o.cr, o.ci, r, i) > 16.0;
#else
      escaped = mandel_step2(o.cr, o.ci, r, i) > 16.0;
#endif
    }
  }
  return __ballot(escaped);
}

// The generator's five words rotate by one place per output (the HEAD stages keep them in place and track the
// rotation): logical word j of a generator whose words are rotated by ROT lives in field (j + ROT) % 5.
template <int K>
__device__ __forceinline__ uint32_t &xorwow_word(Xorwow &s) {
  static_assert(K >= 0 && K < 5, "five words");
  if constexpr (K == 0) return s.x0;
  if constexpr (K == 1) return s.x1;
  if constexpr (K == 2) return s.x2;
  if constexpr (K == 3) return s.x3;
  return s.x4;
}
// The generator words in logical order again (rot back to 0), for store_rng and the generic HEAD.
template <int ROT>
__device__ __forceinline__ Xorwow xorwow_unrotated(Xorwow &s) {
  Xorwow r;
  r.x0 = xorwow_word<(0 + ROT) % 5>(s);
  r.x1 = xorwow_word<(1 + ROT) % 5>(s);
  r.x2 = xorwow_word<(2 + ROT) % 5>(s);
  r.x3 = xorwow_word<(3 + ROT) % 5>(s);
  r.x4 = xorwow_word<(4 + ROT) % 5>(s);
  r.d = s.d;
  return r;
}

__device__ __forceinline__ Canvas make_canvas(const DrawArgs &a) {
  Canvas c;
  c.min_real = a.min_real;
  c.min_imag = a.min_imag;
  c.delta_real = a.delta_real;
  c.delta_imag = a.delta_imag;
  c.inv_delta_real = a.inv_delta_real;
  c.inv_delta_imag = a.inv_delta_imag;
  c.w = a.w;
  c.h = a.h;
  c.pow2_real = a.pow2_real;
  c.pow2_imag = a.pow2_imag;
  c.rcp_delta_real = a.rcp_delta_real;
  c.rcp_delta_imag = a.rcp_delta_imag;
  return c;
}

// Generator states live in six planes of n words (x0..x4, d): coalesced loads and stores.
__device__ __forceinline__ Xorwow load_rng(const uint32_t *states, uint32_t n, uint32_t tid) {
  Xorwow s;
  s.x0 = states[0 * (size_t) n + tid];
  s.x1 = states[1 * (size_t) n + tid];
  s.x2 = states[2 * (size_t) n + tid];
  s.x3 = states[3 * (size_t) n + tid];
  s.x4 = states[4 * (size_t) n + tid];
  s.d = states[5 * (size_t) n + tid];
  return s;
}

__device__ __forceinline__ void store_rng(uint32_t *states, uint32_t n, uint32_t tid,
                                          const Xorwow &s) {
  states[0 * (size_t) n + tid] = s.x0;
  states[1 * (size_t) n + tid] = s.x1;
  states[2 * (size_t) n + tid] = s.x2;
  states[3 * (size_t) n + tid] = s.x3;
  states[4 * (size_t) n + tid] = s.x4;
  states[5 * (size_t) n + tid] = s.d;
}

}  // namespace cb
