// nll_grouped.hip -- MultinoulliNLL over E independent softmaxes (Softmax(n_indep = E),
// loss.py:82-92; sparse targets, loss.py:275-285, 338-346) in ONE launch per direction:
// e2_softmax_nll_grouped_fwd / e2_softmax_nll_grouped_bwd (include/e2hip.h).
//
//   logits / probs / dlogits (n, E*k, d, h, w): group g owns features g*k .. g*k+k-1
//   target (n, E, d, h, w): float class ids of group g in feature g; negative, >= k and
//   non-integer ids are unlabelled
//   stats = {loss_sum, n_lab} over ALL groups: one normaliser, loss = loss_sum / (n_lab + 1e-5)
//
// The group is grid dimension y: work-group (bx, g, n) runs the per-thread body of the n_indep = 1
// kernels (softmax_nll_{fwd,bwd}_body.hpp, the same text that pointwise.hip compiles) on the
// k-feature slice of group g, so a thread owns one position of one group, x stays fastest across
// the lanes and every class plane is read and written coalesced; k and E are run-time numbers and
// nothing is indexed by them in registers.  The statistics keep the protocol of
// e2_softmax_nll_fwd: wave shuffle -> LDS -> one atomic pair per work-group, none for a zero
// partial sum.  A thread reads all it needs of its group before it writes it, and no other thread
// touches that position of that group: dlogits may alias probs.
#include "common.hpp"

namespace {

#define E2_EPS_NLL 1e-5f

// (View5 / vidx / block_sum256 as in pointwise.hip: the bodies below are written against them)
struct View5 {
  float* p;
  int n, c, d, h, w;
  long sn, sc, sd, sh;
};
inline View5 mk(const e2_tensor5* t) {
  return View5{t->ptr, t->n, t->c, t->d, t->h, t->w, (long)t->sn, (long)t->sc,
               (long)t->sd, (long)t->sh};
}
__device__ __forceinline__ long vidx(const View5& v, int n, int c, int z, int y, int x) {
  return (long)n * v.sn + (long)c * v.sc + (long)z * v.sd + (long)y * v.sh + x;
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;
}
// sum over a 256-thread block; result valid in thread 0
__device__ __forceinline__ float block_sum256(float v, float* red) {
  v = wave_sum(v);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) red[wave] = v;
  __syncthreads();
  float r = 0.f;
  if (threadIdx.x == 0) r = red[0] + red[1] + red[2] + red[3];
  __syncthreads();
  return r;
}

// the k-feature slice of group blockIdx.y (target: its one feature)
__device__ __forceinline__ View5 group_of(View5 v, int k) {
  v.p += (long)blockIdx.y * k * v.sc;
  v.c = k;
  return v;
}

// grid: (ceil(d*h*w / 256), E, n).  HAS_T = false: probabilities only, stats untouched.
template <bool HAS_T>
__global__ __launch_bounds__(256) void softmax_nll_grouped_fwd_kernel(View5 lg_all, View5 tg_all,
                                                                      View5 pr_all, int k,
                                                                      float* __restrict__ stats) {
  constexpr bool WT = false;
  const NllW wt{};
  const View5 lg = group_of(lg_all, k), pr = group_of(pr_all, k);
  const View5 tg = HAS_T ? group_of(tg_all, 1) : tg_all;
#include "softmax_nll_fwd_body.hpp"
}

// every group's work-groups see the same stats; loss_out / count_out are written by the first
// work-group of every group with the same value
__global__ __launch_bounds__(256) void softmax_nll_grouped_bwd_kernel(
    View5 pr_all, View5 tg_all, const float* __restrict__ stats, View5 dl_all, int k,
    float* __restrict__ loss_out, int sum_mode, float* __restrict__ count_out) {
  constexpr bool WT = false;
  const NllW wt{};
  const View5 pr = group_of(pr_all, k), dl = group_of(dl_all, k), tg = group_of(tg_all, 1);
#include "softmax_nll_bwd_body.hpp"
}

int check_view(const e2_tensor5* t, const char* name) {
  E2_REQUIRE(t && t->ptr, "%s: null tensor", name);
  E2_REQUIRE(t->n > 0 && t->c > 0 && t->d > 0 && t->h > 0 && t->w > 0,
             "%s: empty tensor (%d,%d,%d,%d,%d)", name, t->n, t->c, t->d, t->h, t->w);
  E2_REQUIRE(t->c < 65536 && t->n < 65536, "%s: n/c too large for grid", name);
  return 0;
}

bool same_extents(const e2_tensor5* a, const e2_tensor5* b) {
  return a->n == b->n && a->d == b->d && a->h == b->h && a->w == b->w;
}

}  // namespace

extern "C" int e2_softmax_nll_grouped_fwd(e2_ctx* ctx, const e2_tensor5* logits,
                                          const e2_tensor5* target, const e2_tensor5* probs,
                                          int n_indep, float* stats) {
  E2_REQUIRE(ctx, "softmax_nll_grouped_fwd: null context");
  E2_REQUIRE(n_indep >= 1, "softmax_nll_grouped_fwd: n_indep = %d", n_indep);
  if (int rc = check_view(logits, "softmax_nll_grouped_fwd logits")) return rc;
  if (int rc = check_view(probs, "softmax_nll_grouped_fwd probs")) return rc;
  E2_REQUIRE(logits->c % n_indep == 0,
             "softmax_nll_grouped_fwd: %d features do not split into %d softmaxes", logits->c,
             n_indep);
  E2_REQUIRE(probs->c == logits->c && same_extents(probs, logits),
             "softmax_nll_grouped_fwd: probs/logits shape mismatch");
  if (target) {
    E2_REQUIRE(stats, "softmax_nll_grouped_fwd: a target needs stats");
    if (int rc = check_view(target, "softmax_nll_grouped_fwd target")) return rc;
    E2_REQUIRE(target->c == n_indep && same_extents(target, logits),
               "softmax_nll_grouped_fwd: target must be (n,%d,d,h,w) matching logits, got "
               "(%d,%d,%d,%d,%d)", n_indep, target->n, target->c, target->d, target->h, target->w);
  }
  const View5 l = mk(logits), p = mk(probs);
  const long S = (long)l.d * l.h * l.w;
  E2_REQUIRE((S + 255) / 256 < (1L << 31), "softmax_nll_grouped_fwd: tensor too large");
  const dim3 grid((unsigned)((S + 255) / 256), (unsigned)n_indep, (unsigned)l.n);
  const int k = l.c / n_indep;
  if (target)
    hipLaunchKernelGGL(softmax_nll_grouped_fwd_kernel<true>, grid, dim3(256), 0, ctx->stream, l,
                       mk(target), p, k, stats);
  else
    hipLaunchKernelGGL(softmax_nll_grouped_fwd_kernel<false>, grid, dim3(256), 0, ctx->stream, l,
                       View5{}, p, k, (float*)nullptr);
  E2_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" int e2_softmax_nll_grouped_bwd(e2_ctx* ctx, const e2_tensor5* probs,
                                          const e2_tensor5* target, int n_indep,
                                          const float* stats, const e2_tensor5* dlogits,
                                          float* loss_out) {
  E2_REQUIRE(ctx && stats, "softmax_nll_grouped_bwd: null argument");
  E2_REQUIRE(n_indep >= 1, "softmax_nll_grouped_bwd: n_indep = %d", n_indep);
  if (int rc = check_view(probs, "softmax_nll_grouped_bwd probs")) return rc;
  if (int rc = check_view(target, "softmax_nll_grouped_bwd target")) return rc;
  if (int rc = check_view(dlogits, "softmax_nll_grouped_bwd dlogits")) return rc;
  E2_REQUIRE(probs->c % n_indep == 0,
             "softmax_nll_grouped_bwd: %d features do not split into %d softmaxes", probs->c,
             n_indep);
  E2_REQUIRE(dlogits->c == probs->c && same_extents(dlogits, probs),
             "softmax_nll_grouped_bwd: dlogits/probs shape mismatch");
  E2_REQUIRE(target->c == n_indep && same_extents(target, probs),
             "softmax_nll_grouped_bwd: target must be (n,%d,d,h,w) matching probs, got "
             "(%d,%d,%d,%d,%d)", n_indep, target->n, target->c, target->d, target->h, target->w);
  const View5 p = mk(probs), t = mk(target), d = mk(dlogits);
  const long S = (long)p.d * p.h * p.w;
  E2_REQUIRE((S + 255) / 256 < (1L << 31), "softmax_nll_grouped_bwd: tensor too large");
  const dim3 grid((unsigned)((S + 255) / 256), (unsigned)n_indep, (unsigned)p.n);
  hipLaunchKernelGGL(softmax_nll_grouped_bwd_kernel, grid, dim3(256), 0, ctx->stream, p, t, stats,
                     d, p.c / n_indep, loss_out, ctx->loss_sum_mode, ctx->loss_count_out);
  E2_CHECK_HIP(hipGetLastError());
  return 0;
}
