// nll_w.hpp -- the weighted MultinoulliNLL (e2_nll_weights; loss.py:172-212, 261-347) of the
// fused classifier kernels, ncls a compile-time number (head.hip, tail.hip).
#pragma once
#include "common.hpp"

#ifndef E2_EPS_NLL
#define E2_EPS_NLL 1e-5f
#endif

// WT is a compile-time flag of the kernel bodies of head.hip / tail.hip: the unweighted kernels
// are the WT = false instantiations.  The masks and class weights of the work-group's batch item
// are read once (uniform addresses, e2_uniform_ld: scalar loads) into a few registers; the
// example weight of a position is read next to its target.
template <int NC>
struct HeadW {
  float up[NC];    // L[n][c] * w[c]: coefficient of -log(p_c + eps) where t == c
  float dn[NC];    // M[n][c] * w[c]: coefficient of -log(q_c + eps), every voxel
  float lab[NC];   // L[n][c]: what a voxel with t == c adds to the count
};
template <int NC>
__device__ __forceinline__ HeadW<NC> head_w_load(const NllW& wt, int n) {
  HeadW<NC> r;
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    const float wc = wt.cw ? e2_uniform_ld(wt.cw, c) : 1.f;
    r.lab[c] = wt.lab ? e2_uniform_ld(wt.lab, n * NC + c) : 1.f;
    r.up[c] = r.lab[c] * wc;
    r.dn[c] = wt.npr ? e2_uniform_ld(wt.npr, n * NC + c) * wc : 0.f;
  }
  return r;
}
// S * sum(M): the not-present part of n_tot, in closed form (one thread of the grid adds it)
__device__ __forceinline__ float head_w_count_dn(const NllW& wt, int n_items, int S) {
  float sm = 0.f;
  if (wt.npr)
    for (int i = 0; i < n_items; ++i) sm += e2_uniform_ld(wt.npr, i);
  return (float)S * sm;
}
// dlogits of one position from its probabilities: g_c = -[t == c] up_c e / (p_c + eps) + dn_c e /
// (q_c + eps) with q_c = 1 - p_c as the sum of the OTHER probabilities (no subtraction: f32 loses
// every digit of 1 - p_c where a not-present class saturates), dlogit_c = p_c (g_c q_c -
// sum_{k != c} g_k p_k).  ev = example weight * (1 / (n_tot + eps), or 1 in sum mode).
template <int NC>
__device__ __forceinline__ void head_w_dlogits(const HeadW<NC>& hw, const float (&pc)[NC], float tv,
                                               float ev, float (&d)[NC]) {
  float q[NC], h[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    q[c] = 0.f;
#pragma unroll
    for (int k = 0; k < NC; ++k)
      if (k != c) q[c] += pc[k];
    const float a = (tv == (float)c) ? hw.up[c] * ev : 0.f;
    const float g = -a / (pc[c] + E2_EPS_NLL) + (hw.dn[c] * ev) / (q[c] + E2_EPS_NLL);
    h[c] = g * pc[c];
    d[c] = g * q[c];
  }
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    float o = 0.f;
#pragma unroll
    for (int k = 0; k < NC; ++k)
      if (k != c) o += h[k];
    d[c] = pc[c] * (d[c] - o);
  }
}
// loss terms of one position from its exponentials ex_c = exp(logit_c - max), den = their sum:
// returns -up_t e log(p_t + eps) - sum_c dn_c e log(q_c + eps), q_c = (sum of the other ex) / den;
// *lab receives what the position adds to the count (L[n][t])
template <int NC>
__device__ __forceinline__ float head_w_loss(const HeadW<NC>& hw, const float (&ex)[NC], float den,
                                             float tv, float ev, float* lab) {
  float ls = 0.f;
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    if (tv == (float)c) { ls -= (hw.up[c] * ev) * logf(ex[c] / den + E2_EPS_NLL); *lab += hw.lab[c]; }
    if (hw.dn[c] != 0.f) {                 // (uniform over the work-group)
      float oth = 0.f;
#pragma unroll
      for (int k = 0; k < NC; ++k)
        if (k != c) oth += ex[k];
      ls -= (hw.dn[c] * ev) * logf(oth / den + E2_EPS_NLL);
    }
  }
  return ls;
}
