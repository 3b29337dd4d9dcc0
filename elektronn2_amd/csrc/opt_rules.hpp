// opt_rules.hpp -- the update rule of each optimiser, written ONCE: what happens to one element of
// the parameter arena.  arena_sweep (arena_ops.hip) calls apply() four times per float4 and once per
// element of the scalar tail, adam_pack_kernel (update_pack.hip) once per tile element, so the paths
// cannot drift apart: with -ffp-contract=off every operation below rounds once, in the order written.
//
// A rule carries
//   NS           the number of state arenas, in the order of the kernel's arguments
//   kCounter     whether the step counter t lives in hyper[4] and is published after the sweep
//   Rule(hyper)  the scalars of this step, from hyper = {lr, mom, beta2, wd, t, factor, -, arrivals}
//   mult(reg)    a segment's weight-decay multiplier -> the factor apply() takes
//   apply(p, g, st, mult)   p and st[NS] of one element, updated in place from the scaled gradient g
//   publish(hyper)          (kCounter) what the last work-group to arrive leaves for the next step
#pragma once
#include <hip/hip_runtime.h>

constexpr float kOptEps = 1e-5f;   // EPS_ADAM of the reference, INSIDE the roots

// Adam (optimiser.py:301-329 of the reference): bias factor sqrt(1 - b2^t) / (1 - mom^t), the L2 term
// outside the adaptive scaling.
struct AdamRule {
  static constexpr int NS = 2;             // m, s
  static constexpr bool kCounter = true;
  float lr, mom, b2, wd, t, fac;
  __device__ __forceinline__ explicit AdamRule(const float* hyper)
      : lr(hyper[0]), mom(hyper[1]), b2(hyper[2]), wd(hyper[3]), t(hyper[4] + 1.f),
        fac(sqrtf(1.f - powf(b2, t)) / (1.f - powf(mom, t))) {}
  __device__ __forceinline__ float mult(float reg) const { return reg * wd; }
  __device__ __forceinline__ void apply(float& p, float g, float (&st)[NS], float mult) const {
    const float nm = mom * st[0] + (1.f - mom) * g;
    const float ns = b2 * st[1] + (1.f - b2) * g * g;
    float dir = fac * nm / sqrtf(ns + kOptEps);
    if (mult != 0.f) dir += mult * p;
    p = p - lr * dir;
    st[0] = nm; st[1] = ns;
  }
  __device__ __forceinline__ void publish(float* hyper) const { hyper[4] = t; hyper[5] = fac; }
};

// SGD (optimiser.py:146-160): d' = g + mom d, p' = p - lr (d' + mult p).
struct SgdRule {
  static constexpr int NS = 1;             // d
  static constexpr bool kCounter = false;
  float lr, mom, wd;
  __device__ __forceinline__ explicit SgdRule(const float* hyper) : lr(hyper[0]), mom(hyper[1]), wd(hyper[3]) {}
  __device__ __forceinline__ float mult(float reg) const { return reg * wd; }
  __device__ __forceinline__ void apply(float& p, float g, float (&st)[NS], float mult) const {
    const float nd = g + mom * st[0];
    p = p - lr * (mult != 0.f ? nd + mult * p : nd);
    st[0] = nd;
  }
};

// AdaGrad (optimiser.py:168-214): h' = h + c g^2, p' = p - lr / sqrt(h') (g + wd r p).
// c = 2 at the first step (t_old == 0): the reference's init_func adds g^2 of the same batch once
// before its first step adds it again (optimiser.py:200-214), one launch here in place of a second
// forward / backward pass.  r = 1 where the segment has a multiplier at all: the reference has no
// apply_reg > 1 branch for AdaGrad (optimiser.py:187-189).  Where h' == 0 -- a gradient that has
// been exactly zero since the start -- the element is left as it is (the reference divides by
// sqrt(0)).  publish() leaves hyper[5] alone (e2hip.h).
struct AdaGradRule {
  static constexpr int NS = 1;             // h
  static constexpr bool kCounter = true;
  float lr, wd, t_old, c;
  __device__ __forceinline__ explicit AdaGradRule(const float* hyper)
      : lr(hyper[0]), wd(hyper[3]), t_old(hyper[4]), c(t_old == 0.f ? 2.f : 1.f) {}
  __device__ __forceinline__ float mult(float reg) const { return reg != 0.f ? wd : 0.f; }
  __device__ __forceinline__ void apply(float& p, float g, float (&st)[NS], float rw) const {
    const float nh = st[0] + c * (g * g);
    if (nh != 0.f) p = p - lr / sqrtf(nh) * (rw != 0.f ? g + rw * p : g);
    st[0] = nh;
  }
  __device__ __forceinline__ void publish(float* hyper) const { hyper[4] = t_old + 1.f; }
};

// AdaDelta (optimiser.py:222-264), eps inside both roots; the direction takes the OLD s and the
// OLD d, as the reference has it; the multiplier as in SgdRule.
struct AdaDeltaRule {
  static constexpr int NS = 2;             // s, d
  static constexpr bool kCounter = false;
  float lr, mom, wd;
  __device__ __forceinline__ explicit AdaDeltaRule(const float* hyper) : lr(hyper[0]), mom(hyper[1]), wd(hyper[3]) {}
  __device__ __forceinline__ float mult(float reg) const { return reg * wd; }
  __device__ __forceinline__ void apply(float& p, float g, float (&st)[NS], float mult) const {
    const float ns = mom * st[0] + (1.f - mom) * g * g;
    const float dir = g * sqrtf(st[1] + kOptEps) / sqrtf(st[0] + kOptEps);
    const float nd = mom * st[1] + (1.f - mom) * dir * dir;
    p = p - lr * (mult != 0.f ? dir + mult * p : dir);
    st[0] = ns; st[1] = nd;
  }
};
