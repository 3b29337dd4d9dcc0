// softmax_nll.hip -- channel softmax + MultinoulliNLL with sparse targets (plain, weighted, and
// over several independent softmaxes in one launch) and the MALIS NLL.  Thread per position,
// x fastest across the lanes; the statistics go wave-shuffle -> LDS -> one atomic per work-group.
#include "stream_common.hpp"

#define E2_EPS_NLL 1e-5f

// ---------------------------------------------------------------------------
// channel softmax + MultinoulliNLL (sparse target), thread per position
// ---------------------------------------------------------------------------
// WT: the weighted form (e2_nll_weights; loss.py:172-212, 261-347), a compile-time variant: the
// unweighted kernels are the WT = false bodies.  With L = mask_class_labeled, M =
// mask_class_not_present, w = class weight, e = example weight:
//   loss sum += -[t == c] L w e log(p_c + eps) - M w e log(q_c + eps),  count += [t == c] L
// q_c = 1 - p_c is the sum of the OTHER classes' terms (f32 loses every digit of 1 - p_c where a
// not-present class saturates).  The masks and class weights sit at work-group-uniform addresses
// (scalar loads: e2_uniform_ld, common.hpp); the example weights are read next to the target.
// S * sum(M), the not-present part of the count, is added once by one thread of the grid.  The
// bodies are
// softmax_nll_{fwd,bwd}_body.hpp, compiled twice each (textual: a shared __device__ function
// changed the instructions of the unweighted kernels).
__global__ void softmax_nll_fwd_kernel(View5 lg, View5 tg, View5 pr,
                                       float* __restrict__ stats) {
  constexpr bool WT = false, HAS_T = true;
  const NllW wt{};
#include "softmax_nll_fwd_body.hpp"
}
__global__ void softmax_nll_fwd_w_kernel(View5 lg, View5 tg, View5 pr,
                                         float* __restrict__ stats, NllW wt) {
  constexpr bool WT = true, HAS_T = true;
#include "softmax_nll_fwd_body.hpp"
}

__global__ void softmax_nll_bwd_kernel(View5 pr, View5 tg, const float* __restrict__ stats,
                                       View5 dl, float* __restrict__ loss_out, int sum_mode,
                                       float* __restrict__ count_out) {
  constexpr bool WT = false, COEF = false;
  const NllW wt{};
#include "softmax_nll_bwd_body.hpp"
}
__global__ void softmax_nll_bwd_w_kernel(View5 pr, View5 tg, const float* __restrict__ stats,
                                         View5 dl, float* __restrict__ loss_out, int sum_mode,
                                         float* __restrict__ count_out, NllW wt) {
  constexpr bool WT = true, COEF = false;
#include "softmax_nll_bwd_body.hpp"
}

// ---------------------------------------------------------------------------
// MultinoulliNLL over E independent softmaxes (Softmax(n_indep = E), loss.py:82-92; sparse
// targets, loss.py:275-285, 338-346) in ONE launch per direction:
// e2_softmax_nll_grouped_fwd / e2_softmax_nll_grouped_bwd (include/e2hip.h).
// ---------------------------------------------------------------------------
//   logits / probs / dlogits (n, E*k, d, h, w): group g owns features g*k .. g*k+k-1
//   target (n, E, d, h, w): float class ids of group g in feature g; negative, >= k and
//   non-integer ids are unlabelled
//   stats = {loss_sum, n_lab} over ALL groups: one normaliser, loss = loss_sum / (n_lab + 1e-5)
//
// The group is grid dimension y: work-group (bx, g, n) runs the per-thread body of the n_indep = 1
// kernels above (softmax_nll_{fwd,bwd}_body.hpp, the same text) on the k-feature slice of group
// g, so a thread owns one position of one group, x stays fastest across the lanes and every class
// plane is read and written coalesced; k and E are run-time numbers and nothing is indexed by
// them in registers.  The statistics keep the protocol of e2_softmax_nll_fwd: wave shuffle -> LDS
// -> one atomic pair per work-group, none for a zero partial sum.  A thread reads all it needs of
// its group before it writes it, and no other thread touches that position of that group: dlogits
// may alias probs.

namespace {

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
  constexpr bool WT = false, COEF = false;
  const NllW wt{};
  const View5 pr = group_of(pr_all, k), dl = group_of(dl_all, k), tg = group_of(tg_all, 1);
#include "softmax_nll_bwd_body.hpp"
}

// ---------------------------------------------------------------------------
// K MultinoulliNLL terms under one AggregateLoss (loss.py:261-347 per term, 1357-1363 for the
// mix), each over a softmax of its own (n_indep = 1, sparse target): e2_nll_multi_fwd /
// e2_nll_mix / e2_nll_multi_bwd (include/e2hip.h).
// ---------------------------------------------------------------------------
// The term is grid dimension y over the same per-thread body: work-group (bx, j, n) handles 256
// positions of term j, whose three views arrive by value in the kernel arguments (work-group-
// uniform index: scalar loads, no register array).  The terms may differ in class count and in
// spatial size; grid.x covers the largest and the work-groups past a smaller term's positions
// leave at once.  stats = {S_0, N_0, S_1, N_1, ...}: every term has its own pair and so its own
// normaliser (unlike the groups above).
struct NllMultiV {
  View5 a[E2_MAX_LOSS_TERMS];     // forward: logits    backward: probs
  View5 t[E2_MAX_LOSS_TERMS];     // targets
  View5 b[E2_MAX_LOSS_TERMS];     // forward: probs     backward: dlogits
};

template <bool HAS_T>
__global__ __launch_bounds__(256) void nll_multi_fwd_kernel(NllMultiV v,
                                                            float* __restrict__ stats_all) {
  constexpr bool WT = false;
  const NllW wt{};
  const int j = blockIdx.y;
  const View5 lg = v.a[j], tg = v.t[j], pr = v.b[j];
  if (blockIdx.x * 256L >= (long)lg.d * lg.h * lg.w) return;      // (the whole work-group)
  float* const stats = stats_all + 2 * j;
#include "softmax_nll_fwd_body.hpp"
}

// one work-group: term values, counts, gradient coefficients and the total.  mix is read here,
// on the device: a captured launch follows its contents.
__global__ void nll_mix_kernel(int k, const float* __restrict__ stats,
                               const float* __restrict__ mix, float* __restrict__ coef,
                               float* __restrict__ term_loss, float* __restrict__ count,
                               float* __restrict__ loss_out) {
  const int j = threadIdx.x;
  __shared__ float part[E2_MAX_LOSS_TERMS];
  if (j < k) {
    const float S = stats[2 * j], N = stats[2 * j + 1], w = mix[j];
    const float L = S / (N + E2_EPS_NLL);
    term_loss[j] = L;
    count[j] = N;
    coef[j] = w / ((float)k * (N + E2_EPS_NLL));
    part[j] = w * L;
  }
  __syncthreads();
  if (j == 0) {
    float tot = 0.f;
    for (int i = 0; i < k; ++i) tot += part[i];      // (fixed order)
    loss_out[0] = tot / (float)k;
  }
}

// coef[j] = w_j / (K (N_j + eps)) takes the place of 1 / (n_lab + eps) in the body
__global__ __launch_bounds__(256) void nll_multi_bwd_kernel(NllMultiV v,
                                                            const float* __restrict__ coef) {
  constexpr bool WT = false, COEF = true;
  const NllW wt{};
  const int j = blockIdx.y;
  const View5 pr = v.a[j], tg = v.t[j], dl = v.b[j];
  const float* const stats = coef + j;
  float* const loss_out = nullptr;
  float* const count_out = nullptr;
  constexpr int sum_mode = 0;
#include "softmax_nll_bwd_body.hpp"
}

}  // namespace

// ---------------------------------------------------------------------------
// MALIS NLL (loss.py:560-690): probs (1, 2E, d,h,w) holds E independent 2-class
// softmaxes (channel 2e = "disconnected", 2e+1 = affinity).  With the MALIS counts
// P (pairs this edge should connect) and N (pairs it should keep apart):
//   loss = -sum(P log(p1+eps) + N log(p0+eps)) * norm[0],  norm[0] = 1/(n_tot+eps)
// and, the counts being constants (malisop.py:114-120: zero gradient),
//   dlogit_c = p_c (g_c - (p0 g0 + p1 g1)),  g1 = -P norm/(p1+eps), g0 = -N norm/(p0+eps)
// thread per (edge, position); loss_sum accumulates the normalised loss.
// ---------------------------------------------------------------------------
__global__ void malis_nll_kernel(View5 pr, const float* __restrict__ pos,
                                 const float* __restrict__ neg,
                                 const float* __restrict__ norm, View5 dl, int want_grad,
                                 float* __restrict__ loss_sum) {
  __shared__ float red[4];
  const long S = (long)pr.d * pr.h * pr.w;
  const long s = blockIdx.x * 256L + threadIdx.x;
  const int e = blockIdx.y;
  const float inv = norm[0];
  float l = 0.f;
  if (s < S) {
    const int x = (int)(s % pr.w);
    const long t = s / pr.w;
    const int y = (int)(t % pr.h), z = (int)(t / pr.h);
    const float* pp = pr.p + vidx(pr, 0, 2 * e, z, y, x);
    const float p0 = pp[0], p1 = pp[pr.sc];
    const float P = pos[(long)e * S + s], N = neg[(long)e * S + s];
    // xlogy0 (loss.py:26-28): 0 where the count is 0, whatever the logarithm
    if (P != 0.f) l -= P * logf(p1 + E2_EPS_NLL);
    if (N != 0.f) l -= N * logf(p0 + E2_EPS_NLL);
    if (want_grad) {
      const float g1 = -P * inv / (p1 + E2_EPS_NLL), g0 = -N * inv / (p0 + E2_EPS_NLL);
      const float m = p0 * g0 + p1 * g1;
      float* dp = dl.p + vidx(dl, 0, 2 * e, z, y, x);
      dp[0] = p0 * (g0 - m);
      dp[dl.sc] = p1 * (g1 - m);
    }
  }
  const float a = block_sum256(l * inv, red);
  if (threadIdx.x == 0 && a != 0.f) unsafeAtomicAdd(loss_sum, a);
}

// The argument checks of the plain, weighted and grouped entry points: two class-plane views of
// one size (a / b = logits / probs forward, probs / dlogits backward) whose features split into
// n_indep softmaxes and, where one is given, a target of n_indep features over the same positions.
static int nll_views_ok(const char* who, const e2_tensor5* a, const char* an, const e2_tensor5* b,
                        const char* bn, const e2_tensor5* target, int n_indep) {
  char name[96];
  E2_REQUIRE(n_indep >= 1, "%s: n_indep = %d", who, n_indep);
  snprintf(name, sizeof name, "%s %s", who, an);
  if (int rc = check_view(a, name)) return rc;
  snprintf(name, sizeof name, "%s %s", who, bn);
  if (int rc = check_view(b, name)) return rc;
  E2_REQUIRE(a->c % n_indep == 0, "%s: %d features do not split into %d softmaxes", who, a->c,
             n_indep);
  E2_REQUIRE(same_size(b, a), "%s: %s/%s shape mismatch: (%d,%d,%d,%d,%d) and (%d,%d,%d,%d,%d)",
             who, bn, an, b->n, b->c, b->d, b->h, b->w, a->n, a->c, a->d, a->h, a->w);
  if (target) {
    snprintf(name, sizeof name, "%s target", who);
    if (int rc = check_view(target, name)) return rc;
    E2_REQUIRE(target->c == n_indep && same_extents(target, a),
               "%s: target must be (n,%d,d,h,w) matching %s, got (%d,%d,%d,%d,%d)", who, n_indep,
               an, target->n, target->c, target->d, target->h, target->w);
  }
  return 0;
}

static int softmax_nll_fwd_impl(e2_ctx* ctx, const e2_tensor5* logits, const e2_tensor5* target,
                                const e2_tensor5* probs, float* stats, const e2_nll_weights* wts) {
  E2_REQUIRE(ctx && stats && target, "softmax_nll_fwd: null argument");
  if (int rc = nll_views_ok("softmax_nll_fwd", logits, "logits", probs, "probs", target, 1))
    return rc;
  View5 l = mk(logits), t = mk(target), p = mk(probs);
  const long S = (long)l.d * l.h * l.w;
  dim3 grid((unsigned)((S + 255) / 256), 1, (unsigned)l.n);
  if (wts) {
    NllW wt;
    if (int rc = e2i_nll_weights(wts, target, "softmax_nll_fwd_w", &wt)) return rc;
    hipLaunchKernelGGL(softmax_nll_fwd_w_kernel, grid, dim3(256), 0, ctx->stream, l, t, p, stats, wt);
  } else {
    hipLaunchKernelGGL(softmax_nll_fwd_kernel, grid, dim3(256), 0, ctx->stream, l, t, p, stats);
  }
  E2_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" int e2_softmax_nll_fwd(e2_ctx* ctx, const e2_tensor5* logits,
                                  const e2_tensor5* target, const e2_tensor5* probs,
                                  float* stats) {
  return softmax_nll_fwd_impl(ctx, logits, target, probs, stats, nullptr);
}

/* the weighted form (loss.py:261-347 with class_weights, example_weights, mask_class_labeled,
 * mask_class_not_present): stats[0] += sum_up + sum_dn, stats[1] += n_tot (include/e2hip.h) */
extern "C" int e2_softmax_nll_fwd_w(e2_ctx* ctx, const e2_tensor5* logits,
                                    const e2_tensor5* target, const e2_tensor5* probs,
                                    float* stats, const e2_nll_weights* wts) {
  return softmax_nll_fwd_impl(ctx, logits, target, probs, stats, wts);
}

static int softmax_nll_bwd_impl(e2_ctx* ctx, const e2_tensor5* probs, const e2_tensor5* target,
                                const float* stats, const e2_tensor5* dlogits, float* loss_out,
                                const e2_nll_weights* wts) {
  E2_REQUIRE(ctx && stats && target, "softmax_nll_bwd: null argument");
  if (int rc = nll_views_ok("softmax_nll_bwd", probs, "probs", dlogits, "dlogits", target, 1))
    return rc;
  View5 p = mk(probs), t = mk(target), d = mk(dlogits);
  const long S = (long)p.d * p.h * p.w;
  dim3 grid((unsigned)((S + 255) / 256), 1, (unsigned)p.n);
  if (wts) {
    NllW wt;
    E2_REQUIRE(dlogits->ptr != probs->ptr, "softmax_nll_bwd_w: dlogits must not alias probs");
    if (int rc = e2i_nll_weights(wts, target, "softmax_nll_bwd_w", &wt)) return rc;
    hipLaunchKernelGGL(softmax_nll_bwd_w_kernel, grid, dim3(256), 0, ctx->stream, p, t, stats, d,
                       loss_out, ctx->loss_sum_mode, ctx->loss_count_out, wt);
  } else {
    hipLaunchKernelGGL(softmax_nll_bwd_kernel, grid, dim3(256), 0, ctx->stream, p, t, stats, d,
                       loss_out, ctx->loss_sum_mode, ctx->loss_count_out);
  }
  E2_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" int e2_softmax_nll_bwd(e2_ctx* ctx, const e2_tensor5* probs,
                                  const e2_tensor5* target, const float* stats,
                                  const e2_tensor5* dlogits, float* loss_out) {
  return softmax_nll_bwd_impl(ctx, probs, target, stats, dlogits, loss_out, nullptr);
}

/* gradient of the weighted loss (loss.py:261-347; formulas in include/e2hip.h) */
extern "C" int e2_softmax_nll_bwd_w(e2_ctx* ctx, const e2_tensor5* probs,
                                    const e2_tensor5* target, const float* stats,
                                    const e2_tensor5* dlogits, float* loss_out,
                                    const e2_nll_weights* wts) {
  return softmax_nll_bwd_impl(ctx, probs, target, stats, dlogits, loss_out, wts);
}

extern "C" int e2_softmax_nll_grouped_fwd(e2_ctx* ctx, const e2_tensor5* logits,
                                          const e2_tensor5* target, const e2_tensor5* probs,
                                          int n_indep, float* stats) {
  E2_REQUIRE(ctx, "softmax_nll_grouped_fwd: null context");
  E2_REQUIRE(!target || stats, "softmax_nll_grouped_fwd: a target needs stats");
  if (int rc = nll_views_ok("softmax_nll_grouped_fwd", logits, "logits", probs, "probs", target,
                            n_indep))
    return rc;
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
  E2_REQUIRE(ctx && stats && target, "softmax_nll_grouped_bwd: null argument");
  if (int rc = nll_views_ok("softmax_nll_grouped_bwd", probs, "probs", dlogits, "dlogits", target,
                            n_indep))
    return rc;
  const View5 p = mk(probs), t = mk(target), d = mk(dlogits);
  const long S = (long)p.d * p.h * p.w;
  E2_REQUIRE((S + 255) / 256 < (1L << 31), "softmax_nll_grouped_bwd: tensor too large");
  const dim3 grid((unsigned)((S + 255) / 256), (unsigned)n_indep, (unsigned)p.n);
  hipLaunchKernelGGL(softmax_nll_grouped_bwd_kernel, grid, dim3(256), 0, ctx->stream, p, t, stats,
                     d, p.c / n_indep, loss_out, ctx->loss_sum_mode, ctx->loss_count_out);
  E2_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" int e2_malis_nll(e2_ctx* ctx, const e2_tensor5* probs, const float* pos,
                            const float* neg, const float* norm, const e2_tensor5* dlogits,
                            float* loss_sum) {
  E2_REQUIRE(ctx && pos && neg && norm && loss_sum, "malis_nll: null argument");
  if (int rc = check_view(probs, "malis_nll probs")) return rc;
  E2_REQUIRE(probs->n == 1 && probs->c >= 2 && probs->c % 2 == 0 && probs->c <= 2 * 65535,
             "malis_nll: probs must be (1, 2E, d, h, w)");
  View5 p = mk(probs), d = p;
  if (dlogits) {
    if (int rc = check_view(dlogits, "malis_nll dlogits")) return rc;
    E2_REQUIRE(dlogits->n == 1 && dlogits->c == probs->c && dlogits->d == probs->d &&
                   dlogits->h == probs->h && dlogits->w == probs->w,
               "malis_nll: dlogits/probs shape mismatch");
    d = mk(dlogits);
  }
  const long S = (long)p.d * p.h * p.w;
  dim3 grid((unsigned)((S + 255) / 256), (unsigned)(p.c / 2), 1);
  hipLaunchKernelGGL(malis_nll_kernel, grid, dim3(256), 0, ctx->stream, p, pos, neg, norm, d,
                     dlogits ? 1 : 0, loss_sum);
  E2_CHECK_HIP(hipGetLastError());
  return 0;
}

// ---- K NLL terms under one mix: the entry points ------------------------------------------
// (sum mode, e2_set_loss_grad_mode, has ONE count slot: K counts do not fit -- an error)
static int nll_multi_pack(e2_ctx* ctx, const char* who, int k, const e2_tensor5* const* a,
                          const char* an, const e2_tensor5* const* targets,
                          const e2_tensor5* const* b, const char* bn, bool need_targets,
                          NllMultiV* v, bool* has_t, long* s_max) {
  E2_REQUIRE(ctx, "%s: null context", who);
  E2_REQUIRE(!ctx->loss_sum_mode, "%s: not available in loss-gradient sum mode (one count slot "
             "cannot hold the terms' counts)", who);
  E2_REQUIRE(k >= 1 && k <= E2_MAX_LOSS_TERMS, "%s: %d terms, 1..%d are supported", who, k,
             E2_MAX_LOSS_TERMS);
  E2_REQUIRE(a && b, "%s: null argument", who);
  int n_t = 0;
  for (int j = 0; j < k; ++j) n_t += (targets && targets[j]) ? 1 : 0;
  E2_REQUIRE(n_t == 0 || n_t == k, "%s: %d of %d terms have a target (all or none)", who, n_t, k);
  E2_REQUIRE(n_t == k || !need_targets, "%s: null target", who);
  *has_t = n_t == k;
  *s_max = 0;
  for (int j = 0; j < k; ++j) {
    char name[96];
    snprintf(name, sizeof name, "%s[%d]", who, j);
    if (int rc = nll_views_ok(name, a[j], an, b[j], bn, *has_t ? targets[j] : nullptr, 1))
      return rc;
    E2_REQUIRE(a[j]->n == a[0]->n, "%s: term %d has batch %d, term 0 has %d", who, j, a[j]->n,
               a[0]->n);
    const long S = (long)a[j]->d * a[j]->h * a[j]->w;
    E2_REQUIRE((S + 255) / 256 < (1L << 31), "%s: tensor too large", who);
    *s_max = S > *s_max ? S : *s_max;
    v->a[j] = mk(a[j]);
    v->b[j] = mk(b[j]);
    v->t[j] = *has_t ? mk(targets[j]) : View5{};
  }
  return 0;
}

extern "C" int e2_nll_multi_fwd(e2_ctx* ctx, int k, const e2_tensor5* const* logits,
                                const e2_tensor5* const* targets,
                                const e2_tensor5* const* probs, float* stats) {
  NllMultiV v{};
  bool has_t;
  long s_max;
  if (int rc = nll_multi_pack(ctx, "nll_multi_fwd", k, logits, "logits", targets, probs, "probs",
                              false, &v, &has_t, &s_max))
    return rc;
  E2_REQUIRE(!has_t || stats, "nll_multi_fwd: targets need stats");
  const dim3 grid((unsigned)((s_max + 255) / 256), (unsigned)k, (unsigned)v.a[0].n);
  if (has_t)
    hipLaunchKernelGGL(nll_multi_fwd_kernel<true>, grid, dim3(256), 0, ctx->stream, v, stats);
  else
    hipLaunchKernelGGL(nll_multi_fwd_kernel<false>, grid, dim3(256), 0, ctx->stream, v,
                       (float*)nullptr);
  E2_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" int e2_nll_mix(e2_ctx* ctx, int k, const float* stats, const float* mixing_w,
                          float* coef, float* term_loss, float* count, float* loss_out) {
  E2_REQUIRE(ctx && stats && mixing_w && coef && term_loss && count && loss_out,
             "nll_mix: null argument");
  E2_REQUIRE(!ctx->loss_sum_mode, "nll_mix: not available in loss-gradient sum mode (one count "
             "slot cannot hold the terms' counts)");
  E2_REQUIRE(k >= 1 && k <= E2_MAX_LOSS_TERMS, "nll_mix: %d terms, 1..%d are supported", k,
             E2_MAX_LOSS_TERMS);
  hipLaunchKernelGGL(nll_mix_kernel, dim3(1), dim3(64), 0, ctx->stream, k, stats, mixing_w, coef,
                     term_loss, count, loss_out);
  E2_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" int e2_nll_multi_bwd(e2_ctx* ctx, int k, const e2_tensor5* const* probs,
                                const e2_tensor5* const* targets, const float* coef,
                                const e2_tensor5* const* dlogits) {
  NllMultiV v{};
  bool has_t;
  long s_max;
  if (int rc = nll_multi_pack(ctx, "nll_multi_bwd", k, probs, "probs", targets, dlogits,
                              "dlogits", true, &v, &has_t, &s_max))
    return rc;
  E2_REQUIRE(coef, "nll_multi_bwd: null coef");
  const dim3 grid((unsigned)((s_max + 255) / 256), (unsigned)k, (unsigned)v.a[0].n);
  hipLaunchKernelGGL(nll_multi_bwd_kernel, grid, dim3(256), 0, ctx->stream, v, coef);
  E2_CHECK_HIP(hipGetLastError());
  return 0;
}
