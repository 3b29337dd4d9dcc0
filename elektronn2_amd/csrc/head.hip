// head.hip -- the classifier head of the segmentation nets, fused:
//   1x1x1 conv to n_class <= 4 features, 'lin' (neural.py:662-712 with a (1,1,1)
//   kernel; examples/neuro3d*.py, unet3d_lite.py: nm.Conv(out, 2, (1,1,1),
//   activation_func='lin')) -> channel softmax (computations.py:175-176) ->
//   MultinoulliNLL with sparse targets (loss.py:261-347), and their gradients.
// As separate launches (split-K GEMM + memset, bias pass, softmax/NLL, lin-act
// backward, wgrad, dgrad) the head costs ~12 launch-latency-bound kernels for
// 0.01 GF; fused it is two streaming passes over the C-channel input:
//   forward : work-group = 64 positions x 4 channel quarters; partial logits (fp32 FMA
//             chains, coalesced reads, weight rows as scalar operands) meet in LDS,
//             softmax, probs out, loss sum and labelled count by atomics.
//   backward: work-group = tiles of 32 positions; dlogits from probs/target, the
//             input tile through LDS; thread ci accumulates dW[c][ci] over all its
//             tiles in registers (one atomic per (c,ci) per work-group at the
//             end), every thread writes its share of dx = W^T dlogits.
// Bound: HBM (read C*S*4 B; backward also writes C*S*4 B).
#include "stream_common.hpp"
#include "nll_w.hpp"
#include <algorithm>

#define E2_HEAD_MAXC 4

namespace {

struct HView {
  float* p;
  int n, c, d, h, w;
  long sn, sc, sd, sh;
};
HView hv(const e2_tensor5* t) {
  return HView{t->ptr, t->n, t->c, t->d, t->h, t->w, (long)t->sn, (long)t->sc, (long)t->sd,
               (long)t->sh};
}
__device__ __forceinline__ long hidx(const HView& v, int n, int z, int y, int x) {
  return (long)n * v.sn + (long)z * v.sd + (long)y * v.sh + x;
}

// The kernel bodies are head_fwd_body.hpp / head_bwd_body.hpp, each compiled twice: with WT = false
// as head_fwd_kernel / head_bwd_kernel and with WT = true (the weighted loss, nll_w.hpp) as
// head_fwd_w_kernel / head_bwd_w_kernel.  (Textual, not a shared __device__ function: passing the
// views on changed the instructions hipcc emits for the unweighted kernels.)
// ---- forward ---------------------------------------------------------------------
// work-group = 64 positions x 4 channel quarters (one wave each): the positions of a
// net's last layer are few (13,690 for C-lite@183), so the channel loop is split to
// put four times as many waves on the chip; partial logits meet in LDS.
template <int NC>
__global__ __launch_bounds__(256) void head_fwd_kernel(HView x, const float* __restrict__ w,
                                                       const float* __restrict__ bias,
                                                       HView tg, int has_target, HView pr,
                                                       float* __restrict__ stats) {
  constexpr bool WT = false;
  const NllW wt{};
#include "head_fwd_body.hpp"
}
template <int NC>
__global__ __launch_bounds__(256) void head_fwd_w_kernel(HView x, const float* __restrict__ w,
                                                         const float* __restrict__ bias,
                                                         HView tg, HView pr,
                                                         float* __restrict__ stats, NllW wt) {
  constexpr bool WT = true;
  constexpr int has_target = 1;
#include "head_fwd_body.hpp"
}

// ---- backward --------------------------------------------------------------------
constexpr int HT = 32;     // positions per tile

template <int NC>
__global__ __launch_bounds__(256) void head_bwd_kernel(HView x, const float* __restrict__ w,
                                                       HView pr, HView tg,
                                                       const float* __restrict__ stats,
                                                       HView dx, int want_dx, int accumulate,
                                                       float* __restrict__ part,
                                                       float* __restrict__ loss_out,
                                                       int tilesPerN, int nTiles, int sum_mode,
                                                       float* __restrict__ count_out) {
  constexpr bool WT = false;
  const NllW wt{};
#include "head_bwd_body.hpp"
}
template <int NC>
__global__ __launch_bounds__(256) void head_bwd_w_kernel(HView x, const float* __restrict__ w,
                                                         HView pr, HView tg,
                                                         const float* __restrict__ stats,
                                                         HView dx, int want_dx, int accumulate,
                                                         float* __restrict__ part,
                                                         float* __restrict__ loss_out,
                                                         int tilesPerN, int nTiles, int sum_mode,
                                                         float* __restrict__ count_out, NllW wt) {
  constexpr bool WT = true;
#include "head_bwd_body.hpp"
}

// dw[i] += sum_b part[b][i] (i < NC*C), dbias[c] += sum_b part[b][NC*C + c]
__global__ __launch_bounds__(256) void head_reduce_kernel(const float* __restrict__ part,
                                                          int nBlocks, int total, int nW,
                                                          float* dw, float* dbias) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int per = (nBlocks + gridDim.y - 1) / gridDim.y;
  const int b0 = blockIdx.y * per, b1 = min(b0 + per, nBlocks);
  float s = 0.f;
#pragma unroll 8
  for (int b = b0; b < b1; ++b) s += part[(long)b * total + idx];
  if (s != 0.f) unsafeAtomicAdd(idx < nW ? dw + idx : dbias + (idx - nW), s);
}

int head_check(const e2_tensor5* t, const char* name) {
  E2_REQUIRE(t && t->ptr, "%s: null tensor", name);
  E2_REQUIRE(t->n > 0 && t->c > 0 && t->d > 0 && t->h > 0 && t->w > 0 && t->n < 65536,
             "%s: bad shape (%d,%d,%d,%d,%d)", name, t->n, t->c, t->d, t->h, t->w);
  return 0;
}
bool same_sp(const e2_tensor5* a, const e2_tensor5* b) {
  return a->n == b->n && a->d == b->d && a->h == b->h && a->w == b->w;
}

}  // namespace

extern "C" int e2_head_supported(int cin, int ncls) {
  return ncls >= 2 && ncls <= E2_HEAD_MAXC && cin >= 1 && cin <= 512;
}

/* probs = softmax(W x + b) over the ncls channels; with a target also
 * stats[0] += sum(-log(p_target + 1e-5)), stats[1] += #labelled (zero stats first). */
static int head_fwd_impl(e2_ctx* ctx, const e2_tensor5* x, const float* w, const float* bias,
                         int ncls, const e2_tensor5* target, const e2_tensor5* probs,
                         float* stats, const e2_nll_weights* wts) {
  E2_REQUIRE(ctx && w && bias, "head_fwd: null argument");
  if (int rc = head_check(x, "head_fwd x")) return rc;
  if (int rc = head_check(probs, "head_fwd probs")) return rc;
  E2_REQUIRE(e2_head_supported(x->c, ncls), "head_fwd: unsupported cin=%d ncls=%d", x->c, ncls);
  E2_REQUIRE(probs->c == ncls && same_sp(x, probs), "head_fwd: probs shape mismatch");
  HView vt{};
  if (target) {
    if (int rc = head_check(target, "head_fwd target")) return rc;
    E2_REQUIRE(stats && target->c == 1 && same_sp(x, target), "head_fwd: target shape mismatch");
    vt = hv(target);
  }
  const long S = (long)x->d * x->h * x->w;
  E2_REQUIRE(S < (1L << 31), "head_fwd: channel too large");
  dim3 grid((unsigned)((S + 63) / 64), 1, (unsigned)x->n);
  if (wts) {
    E2_REQUIRE(target, "head_fwd_w: the weighted loss needs a target");
    NllW wt;
    if (int rc = e2i_nll_weights(wts, target, "head_fwd_w", &wt)) return rc;
#define E2_HFW(NC)                                                                       \
  hipLaunchKernelGGL((head_fwd_w_kernel<NC>), grid, dim3(256), 0, ctx->stream, hv(x), w, \
                     bias, vt, hv(probs), stats, wt)
    if (ncls == 2) E2_HFW(2); else if (ncls == 3) E2_HFW(3); else E2_HFW(4);
#undef E2_HFW
    E2_CHECK_HIP(hipGetLastError());
    return 0;
  }
#define E2_HF(NC)                                                                      \
  hipLaunchKernelGGL((head_fwd_kernel<NC>), grid, dim3(256), 0, ctx->stream, hv(x), w, \
                     bias, vt, target ? 1 : 0, hv(probs), stats)
  if (ncls == 2) E2_HF(2); else if (ncls == 3) E2_HF(3); else E2_HF(4);
#undef E2_HF
  E2_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" int e2_head_fwd(e2_ctx* ctx, const e2_tensor5* x, const float* w, const float* bias,
                           int ncls, const e2_tensor5* target, const e2_tensor5* probs,
                           float* stats) {
  return head_fwd_impl(ctx, x, w, bias, ncls, target, probs, stats, nullptr);
}

/* e2_head_fwd with the weighted loss (loss.py:261-347 with class_weights, example_weights,
 * mask_class_labeled, mask_class_not_present): stats[0] += sum_up + sum_dn, stats[1] += n_tot
 * (include/e2hip.h).  A target is required. */
extern "C" int e2_head_fwd_w(e2_ctx* ctx, const e2_tensor5* x, const float* w, const float* bias,
                             int ncls, const e2_tensor5* target, const e2_tensor5* probs,
                             float* stats, const e2_nll_weights* wts) {
  return head_fwd_impl(ctx, x, w, bias, ncls, target, probs, stats, wts);
}

static long head_grid(const e2_ctx* ctx, int n, long S) {
  const long nTiles = ((S + HT - 1) / HT) * n;
  return std::min<long>(nTiles, 2L * (ctx ? ctx->num_cu : 256));
}
extern "C" size_t e2_head_bwd_workspace_bytes(int n, int cin, int ncls, int d, int h, int w) {
  const long S = (long)d * h * w;
  const long blocks = std::min<long>(((S + HT - 1) / HT) * n, 2L * 1024);   // any CU count
  return sizeof(float) * (size_t)blocks * ((size_t)ncls * cin + ncls);
}

/* gradients of loss = stats[0]/(stats[1]+1e-5): dx (optional; accumulate_dx: +=),
 * dw[ncls*cin] and dbias[ncls] are ACCUMULATED (zero them first); loss_out optional.
 * ws: e2_head_bwd_workspace_bytes(n, cin, ncls, d, h, w) bytes. */
static int head_bwd_impl(e2_ctx* ctx, const e2_tensor5* x, const float* w,
                         const e2_tensor5* probs, const e2_tensor5* target,
                         const float* stats, const e2_tensor5* dx, int accumulate_dx,
                         float* dw, float* dbias, float* loss_out, void* ws,
                         size_t ws_bytes, const e2_nll_weights* wts) {
  E2_REQUIRE(ctx && w && stats && dw && dbias && ws, "head_bwd: null argument");
  if (int rc = head_check(x, "head_bwd x")) return rc;
  if (int rc = head_check(probs, "head_bwd probs")) return rc;
  if (int rc = head_check(target, "head_bwd target")) return rc;
  const int ncls = probs->c;
  E2_REQUIRE(e2_head_supported(x->c, ncls), "head_bwd: unsupported cin=%d ncls=%d", x->c, ncls);
  E2_REQUIRE(same_sp(x, probs) && same_sp(x, target) && target->c == 1,
             "head_bwd: shape mismatch");
  HView vdx{};
  if (dx) {
    if (int rc = head_check(dx, "head_bwd dx")) return rc;
    E2_REQUIRE(dx->c == x->c && same_sp(x, dx), "head_bwd: dx shape mismatch");
    vdx = hv(dx);
  }
  const long S = (long)x->d * x->h * x->w;
  E2_REQUIRE(S < (1L << 31) - 64, "head_bwd: channel too large");
  const long tilesPerN = (S + HT - 1) / HT;
  const long nTiles = tilesPerN * x->n;
  E2_REQUIRE(nTiles < (1L << 31), "head_bwd: too many tiles");
  const int grid = (int)head_grid(ctx, x->n, S);
  const int total = ncls * x->c + ncls;
  E2_REQUIRE(ws_bytes >= sizeof(float) * (size_t)grid * total, "head_bwd: workspace too small");
  float* part = (float*)ws;
  const size_t lds = sizeof(float) * ((size_t)ncls * HT + (size_t)x->c * (HT + 1));
#define E2_HB(NC)                                                                        \
  do {                                                                                   \
    static bool attr_done = false;                                                       \
    if (!attr_done) {                                                                    \
      E2_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&head_bwd_kernel<NC>), \
                                       hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024)); \
      attr_done = true;                                                                  \
    }                                                                                    \
    hipLaunchKernelGGL((head_bwd_kernel<NC>), dim3(grid), dim3(256), lds, ctx->stream,   \
                       hv(x), w, hv(probs), hv(target), stats, vdx, dx ? 1 : 0,          \
                       accumulate_dx, part, loss_out, (int)tilesPerN, (int)nTiles,       \
                       ctx->loss_sum_mode, ctx->loss_count_out);                         \
  } while (0)
#define E2_HBW(NC)                                                                       \
  do {                                                                                   \
    static bool attr_done = false;                                                       \
    if (!attr_done) {                                                                    \
      E2_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&head_bwd_w_kernel<NC>), \
                                       hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024)); \
      attr_done = true;                                                                  \
    }                                                                                    \
    hipLaunchKernelGGL((head_bwd_w_kernel<NC>), dim3(grid), dim3(256), lds, ctx->stream, \
                       hv(x), w, hv(probs), hv(target), stats, vdx, dx ? 1 : 0,          \
                       accumulate_dx, part, loss_out, (int)tilesPerN, (int)nTiles,       \
                       ctx->loss_sum_mode, ctx->loss_count_out, wt);                     \
  } while (0)
  if (wts) {
    NllW wt;
    if (int rc = e2i_nll_weights(wts, target, "head_bwd_w", &wt)) return rc;
    if (ncls == 2) E2_HBW(2); else if (ncls == 3) E2_HBW(3); else E2_HBW(4);
  } else {
    if (ncls == 2) E2_HB(2); else if (ncls == 3) E2_HB(3); else E2_HB(4);
  }
#undef E2_HB
#undef E2_HBW
  E2_CHECK_HIP(hipGetLastError());
  hipLaunchKernelGGL(head_reduce_kernel, dim3(e2_cdiv(total, 256), std::min(grid, 16)), dim3(256),
                     0, ctx->stream, part, grid, total, ncls * x->c, dw, dbias);
  E2_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" int e2_head_bwd(e2_ctx* ctx, const e2_tensor5* x, const float* w,
                           const e2_tensor5* probs, const e2_tensor5* target,
                           const float* stats, const e2_tensor5* dx, int accumulate_dx,
                           float* dw, float* dbias, float* loss_out, void* ws,
                           size_t ws_bytes) {
  return head_bwd_impl(ctx, x, w, probs, target, stats, dx, accumulate_dx, dw, dbias, loss_out, ws,
                       ws_bytes, nullptr);
}

/* e2_head_bwd for the weighted loss (loss.py:261-347; the gradient formula in include/e2hip.h):
 * stats as e2_head_fwd_w left them */
extern "C" int e2_head_bwd_w(e2_ctx* ctx, const e2_tensor5* x, const float* w,
                             const e2_tensor5* probs, const e2_tensor5* target,
                             const float* stats, const e2_tensor5* dx, int accumulate_dx,
                             float* dw, float* dbias, float* loss_out, void* ws,
                             size_t ws_bytes, const e2_nll_weights* wts) {
  return head_bwd_impl(ctx, x, w, probs, target, stats, dx, accumulate_dx, dw, dbias, loss_out, ws,
                       ws_bytes, wts);
}
