// multihead.hip -- K classifier heads on ONE trunk, fused (multi-task nets: one trunk, K softmax
// heads, K MultinoulliNLL terms under one AggregateLoss -- loss.py:261-347, 1357-1363):
//   head j: 1x1x1 'lin' conv to ncls_j features -> channel softmax -> sparse NLL, j < K <= 8,
//   sum ncls_j <= 16.  Run as K copies of head.hip the trunk activation is streamed K times
//   forward and K times backward, and the 2nd..K-th backward launch reads, modifies and writes
//   the trunk gradient.  Here every element of x is read once per direction and dx is written
//   once:
//   forward : work-group = 64 positions x 4 channel quarters as head.hip; ALL sum ncls logits
//             are formed in one pass (NT = the total rounded up to 4 / 8 / 12 / 16 accumulators,
//             indexed by compile-time numbers only; the weight rows of the K parameters are K
//             pointers resolved to one scalar row pointer per logit before the loop), the
//             partial logits meet in LDS, then wave q runs the softmax and the loss of heads q,
//             q + 4 over LDS: class counts and head boundaries are run-time numbers and index
//             LDS, never registers.
//   backward: work-group = tiles of 32 positions as head.hip; thread (position, head) writes its
//             head's dlogits = coef_j (...) to LDS, the input tile goes through LDS, thread ci
//             accumulates dW[c][ci] for all NT rows, every thread writes its share of
//             dx = sum_j W_j^T dlogits_j.  Per-work-group partial sums, then a reduce launch that
//             adds them into the K heads' own dw / dbias.
// coef_j = w_j / (K (N_j + 1e-5)) comes from e2_nll_mix.  f32 VALU in either mfma mode.
// Traffic: read cin*S*4 B per direction; backward also writes cin*S*4 B.  Measured (DESIGN.md
// finding 61) the pair runs far below the memory bound, about 0.3 TB/s: the backward's LDS-broadcast
// FMA loops limit it, as they limit head.hip.
#include "stream_common.hpp"
#include <algorithm>

#define E2_EPS_NLL 1e-5f
#define E2_MH_MAXK E2_MAX_LOSS_TERMS
#define E2_MH_MAXC 16

namespace {

struct MHeads {
  int k, tot;                          // heads, sum of their classes
  int c0[E2_MH_MAXK + 1];              // first logit of head j; c0[k] = tot
  const float* w[E2_MH_MAXK];          // (ncls_j, cin) dense
  const float* bias[E2_MH_MAXK];
  float* dw[E2_MH_MAXK];               // reduce launch only
  float* db[E2_MH_MAXK];
  View5 pr[E2_MH_MAXK];
  View5 tg[E2_MH_MAXK];
};

// row pointer of logit c (a compile-time number at every call): the head is found by comparing
// against the run-time boundaries, all work-group-uniform.  Logits past the total (padding up to
// NT) get the last real row: their values are never read.
__device__ __forceinline__ const float* mh_row(const MHeads& h, int c, int cin) {
  const int cc = min(c, h.tot - 1);
  const float* r = h.w[0];
  int base = 0;
#pragma unroll
  for (int j = 1; j < E2_MH_MAXK; ++j)
    if (j < h.k && cc >= h.c0[j]) { r = h.w[j]; base = h.c0[j]; }
  return r + (long)(cc - base) * cin;
}

template <int NT>
__global__ __launch_bounds__(256) void multihead_fwd_kernel(View5 x, MHeads h, int has_target,
                                                            float* __restrict__ stats) {
  __shared__ float part[4][NT][64];
  const int S = x.d * x.h * x.w;
  const int p = threadIdx.x & 63, cq = threadIdx.x >> 6;
  const int s = blockIdx.x * 64 + p;
  const int n = blockIdx.z;
  const bool valid = s < S;
  int xx = 0, y = 0, z = 0;
  if (valid) {
    xx = s % x.w;
    const int t = s / x.w;
    y = t % x.h; z = t / x.h;
  }
  const float* row[NT];
#pragma unroll
  for (int c = 0; c < NT; ++c) row[c] = mh_row(h, c, x.c);
  const int per = (x.c + 3) >> 2;
  const int c0 = cq * per, c1 = min(c0 + per, x.c);
  float acc[NT];
#pragma unroll
  for (int c = 0; c < NT; ++c) acc[c] = 0.f;
  if (valid) {
    const float* xp = x.p + vidx(x, n, 0, z, y, xx);
#pragma unroll 4
    for (int ci = c0; ci < c1; ++ci) {
      const float v = xp[(long)ci * x.sc];
#pragma unroll
      for (int c = 0; c < NT; ++c) acc[c] = fmaf(row[c][ci], v, acc[c]);
    }
  }
#pragma unroll
  for (int c = 0; c < NT; ++c) part[cq][c][p] = acc[c];
  __syncthreads();
  // wave cq: heads cq, cq + 4.  Thread (p, head) alone touches part[.][its classes][p].
  for (int jj = cq; jj < h.k; jj += 4) {
    const int j = __builtin_amdgcn_readfirstlane(jj);
    const int a = h.c0[j], b = h.c0[j + 1];
    float lsum = 0.f, nlab = 0.f;
    if (valid) {
      const float* bj = h.bias[j];
      float m = -INFINITY;
      for (int c = a; c < b; ++c) {
        const float v = ((part[0][c][p] + part[1][c][p]) + (part[2][c][p] + part[3][c][p])) +
                        bj[c - a];
        part[0][c][p] = v;
        m = fmaxf(m, v);
      }
      float den = 0.f;
      for (int c = a; c < b; ++c) den += expf(part[0][c][p] - m);
      const View5 pr = h.pr[j];
      float tv = -1.f;
      if (has_target) {
        const View5 tg = h.tg[j];
        tv = tg.p[vidx(tg, n, 0, z, y, xx)];
      }
      float* pp = pr.p + vidx(pr, n, 0, z, y, xx);
      for (int c = a; c < b; ++c) {
        const float pc = expf(part[0][c][p] - m) / den;
        pp[(long)(c - a) * pr.sc] = pc;
        if (tv == (float)(c - a)) { lsum -= logf(pc + E2_EPS_NLL); nlab += 1.f; }
      }
    }
    if (has_target) {
      const float sa = wave_sum(lsum);
      const float sb = wave_sum(nlab);
      if (p == 0) {
        if (sa != 0.f) unsafeAtomicAdd(stats + 2 * j, sa);
        if (sb != 0.f) unsafeAtomicAdd(stats + 2 * j + 1, sb);
      }
    }
  }
}

constexpr int MT = 32;     // positions per tile (backward)

template <int NT>
__global__ __launch_bounds__(256) void multihead_bwd_kernel(View5 x, MHeads h,
                                                            const float* __restrict__ coef,
                                                            View5 dx, int want_dx, int accumulate,
                                                            float* __restrict__ part,
                                                            int tilesPerN, int nTiles) {
  extern __shared__ float hs[];
  const int C = x.c;
  float* dl = hs;                         // [NT][MT]
  float* xs = hs + NT * MT;               // [C][MT + 1]
  const int tid = threadIdx.x;
  const int S = x.d * x.h * x.w;
  const int tot = h.tot;
  for (int i = tid; i < NT * MT; i += 256) dl[i] = 0.f;      // (the padding rows stay zero)
  const float* row[NT];
#pragma unroll
  for (int c = 0; c < NT; ++c) row[c] = mh_row(h, c, C);
  // thread ci < C (two rounds when C > 256) owns dW[c][ci]
  float aw[2][NT];
#pragma unroll
  for (int r = 0; r < 2; ++r)
#pragma unroll
    for (int c = 0; c < NT; ++c) aw[r][c] = 0.f;
  float ab = 0.f;                         // dbias partial of logit tid (threads 0..NT-1)
  const int p = tid & (MT - 1);
  const int hj = tid / MT;                // the head whose dlogits this thread writes (if < k)
  __syncthreads();

  for (int tile = blockIdx.x; tile < nTiles; tile += gridDim.x) {
    const int n = tile / tilesPerN;
    const int s0 = (tile - n * tilesPerN) * MT;
    const int np = min(MT, S - s0);
    int pz = 0, py = 0, px = 0;
    if (p < np) {
      const int s = s0 + p;
      px = s % x.w;
      const int t = s / x.w;
      py = t % x.h; pz = t / x.h;
    }
    // dlogits of the tile: thread (position p, head hj)
    if (hj < h.k) {
      const int a = h.c0[hj], b = h.c0[hj + 1];
      if (p < np) {
        const View5 pr = h.pr[hj], tg = h.tg[hj];
        const float tv = tg.p[vidx(tg, n, 0, pz, py, px)];
        const float* pp = pr.p + vidx(pr, n, 0, pz, py, px);
        float pt = 0.f;
        int tc = -1;
        for (int c = 0; c < b - a; ++c)
          if (tv == (float)c) { tc = c; pt = pp[(long)c * pr.sc]; }
        // dlogit_c = coef (-p_t / (p_t + eps)) ([c == t] - p_c)
        const float gpt = (tc >= 0) ? (-coef[hj] / (pt + E2_EPS_NLL)) * pt : 0.f;
        for (int c = 0; c < b - a; ++c)
          dl[(a + c) * MT + p] = gpt * ((c == tc ? 1.f : 0.f) - pp[(long)c * pr.sc]);
      } else {
        for (int c = a; c < b; ++c) dl[c * MT + p] = 0.f;
      }
    }
    // the input tile, coalesced: 256/MT channel rows of MT positions per pass
    {
      const long off = vidx(x, n, 0, pz, py, px);
      const bool pv = p < np;
#pragma unroll 8
      for (int ci = tid / MT; ci < C; ci += 256 / MT)
        xs[ci * (MT + 1) + p] = pv ? x.p[off + (long)ci * x.sc] : 0.f;
    }
    __syncthreads();
    if (tid < tot) {
      float sb = 0.f;
      for (int q = 0; q < MT; ++q) sb += dl[tid * MT + q];
      ab += sb;
    }
    // dW partial sums: thread = input channel
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      const int ci = tid + 256 * r;
      if (ci < C) {
        const float* xr = xs + ci * (MT + 1);
        for (int q = 0; q < MT; ++q) {
          const float v = xr[q];
#pragma unroll
          for (int c = 0; c < NT; ++c) aw[r][c] = fmaf(dl[c * MT + q], v, aw[r][c]);
        }
      }
    }
    // dx = sum_j W_j^T dlogits_j, written (or accumulated) coalesced, once
    if (want_dx) {
      if (p < np) {
        float* dp = dx.p + vidx(dx, n, 0, pz, py, px);
        float d[NT];
#pragma unroll
        for (int c = 0; c < NT; ++c) d[c] = dl[c * MT + p];
#pragma unroll 4
        for (int ci = tid / MT; ci < C; ci += 256 / MT) {
          float g = 0.f;
#pragma unroll
          for (int c = 0; c < NT; ++c)
            if (c < tot) g = fmaf(row[c][ci], d[c], g);
          float* q = dp + (long)ci * dx.sc;
          *q = accumulate ? (*q + g) : g;
        }
      }
    }
    __syncthreads();
  }
  // flush: this work-group's partial sums, part[block][tot*C + tot] (plain stores)
  float* mine = part + (long)blockIdx.x * ((long)tot * C + tot);
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    const int ci = tid + 256 * r;
    if (ci < C) {
#pragma unroll
      for (int c = 0; c < NT; ++c)
        if (c < tot) mine[(long)c * C + ci] = aw[r][c];
    }
  }
  if (tid < tot) mine[(long)tot * C + tid] = ab;
}

// dw_j[i] += sum_b part[b][c0_j*C + i], dbias_j[c] += sum_b part[b][tot*C + c0_j + c]
__global__ __launch_bounds__(256) void multihead_reduce_kernel(const float* __restrict__ part,
                                                               int nBlocks, int C, MHeads h) {
  const int total = h.tot * C + h.tot;
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int per = (nBlocks + gridDim.y - 1) / gridDim.y;
  const int b0 = blockIdx.y * per, b1 = min(b0 + per, nBlocks);
  float s = 0.f;
#pragma unroll 8
  for (int b = b0; b < b1; ++b) s += part[(long)b * total + idx];
  if (s == 0.f) return;
  const bool is_w = idx < h.tot * C;
  const int c = is_w ? idx / C : idx - h.tot * C;       // the logit
  float* dst = is_w ? h.dw[0] : h.db[0];
  int base = 0;
#pragma unroll
  for (int j = 1; j < E2_MH_MAXK; ++j)
    if (j < h.k && c >= h.c0[j]) { dst = is_w ? h.dw[j] : h.db[j]; base = h.c0[j]; }
  unsafeAtomicAdd(dst + (is_w ? (long)idx - (long)base * C : (long)(c - base)), s);
}

bool mh_same_sp(const e2_tensor5* a, const e2_tensor5* b) {
  return a->n == b->n && a->d == b->d && a->h == b->h && a->w == b->w;
}

}  // namespace

extern "C" int e2_multihead_supported(int cin, int k, const int* ncls) {
  if (!ncls || k < 2 || k > E2_MH_MAXK || cin < 1 || cin > 512) return 0;
  int tot = 0;
  for (int j = 0; j < k; ++j) {
    if (ncls[j] < 2) return 0;
    tot += ncls[j];
  }
  return tot <= E2_MH_MAXC;
}

// the checks the two entry points share; fills the heads' offsets and views
static int mh_pack(e2_ctx* ctx, const char* who, const e2_tensor5* x, int k, const float* const* w,
                   const int* ncls, const e2_tensor5* const* targets, bool need_targets,
                   const e2_tensor5* const* probs, MHeads* h, bool* has_t) {
  E2_REQUIRE(ctx, "%s: null context", who);
  E2_REQUIRE(!ctx->loss_sum_mode, "%s: not available in loss-gradient sum mode (one count slot "
             "cannot hold the heads' counts)", who);
  E2_REQUIRE(k >= 2 && k <= E2_MH_MAXK, "%s: %d heads, 2..%d are supported", who, k, E2_MH_MAXK);
  E2_REQUIRE(w && ncls && probs, "%s: null argument", who);
  char name[96];
  snprintf(name, sizeof name, "%s x", who);
  if (int rc = check_view(x, name)) return rc;
  E2_REQUIRE(e2_multihead_supported(x->c, k, ncls), "%s: unsupported cin=%d or class counts", who,
             x->c);
  int n_t = 0;
  for (int j = 0; j < k; ++j) n_t += (targets && targets[j]) ? 1 : 0;
  E2_REQUIRE(n_t == 0 || n_t == k, "%s: %d of %d heads have a target (all or none)", who, n_t, k);
  E2_REQUIRE(n_t == k || !need_targets, "%s: null target", who);
  *has_t = n_t == k;
  const long S = (long)x->d * x->h * x->w;
  E2_REQUIRE(S < (1L << 31) - 64, "%s: channel too large", who);
  h->k = k;
  int tot = 0;
  for (int j = 0; j < k; ++j) {
    E2_REQUIRE(w[j], "%s: null weights of head %d", who, j);
    snprintf(name, sizeof name, "%s probs[%d]", who, j);
    if (int rc = check_view(probs[j], name)) return rc;
    E2_REQUIRE(probs[j]->c == ncls[j] && mh_same_sp(x, probs[j]),
               "%s: probs[%d] is (%d,%d,%d,%d,%d), head %d needs (%d,%d,%d,%d,%d)", who, j,
               probs[j]->n, probs[j]->c, probs[j]->d, probs[j]->h, probs[j]->w, j, x->n, ncls[j],
               x->d, x->h, x->w);
    if (*has_t) {
      snprintf(name, sizeof name, "%s targets[%d]", who, j);
      if (int rc = check_view(targets[j], name)) return rc;
      E2_REQUIRE(targets[j]->c == 1 && mh_same_sp(x, targets[j]), "%s: targets[%d] shape mismatch",
                 who, j);
      h->tg[j] = mk(targets[j]);
    }
    h->c0[j] = tot;
    h->w[j] = w[j];
    h->pr[j] = mk(probs[j]);
    tot += ncls[j];
  }
  h->c0[k] = tot;
  h->tot = tot;
  return 0;
}

#define E2_MH_DISPATCH(tot, CALL)                 \
  do {                                            \
    if ((tot) <= 4) CALL(4);                      \
    else if ((tot) <= 8) CALL(8);                 \
    else if ((tot) <= 12) CALL(12);               \
    else CALL(16);                                \
  } while (0)

extern "C" int e2_multihead_fwd(e2_ctx* ctx, const e2_tensor5* x, int k, const float* const* w,
                                const float* const* bias, const int* ncls,
                                const e2_tensor5* const* targets,
                                const e2_tensor5* const* probs, float* stats) {
  MHeads h{};
  bool has_t;
  if (int rc = mh_pack(ctx, "multihead_fwd", x, k, w, ncls, targets, false, probs, &h, &has_t))
    return rc;
  E2_REQUIRE(bias, "multihead_fwd: null argument");
  for (int j = 0; j < k; ++j) {
    E2_REQUIRE(bias[j], "multihead_fwd: null bias of head %d", j);
    h.bias[j] = bias[j];
  }
  E2_REQUIRE(!has_t || stats, "multihead_fwd: targets need stats");
  const long S = (long)x->d * x->h * x->w;
  const dim3 grid((unsigned)((S + 63) / 64), 1, (unsigned)x->n);
#define E2_MHF(NT)                                                                            \
  hipLaunchKernelGGL((multihead_fwd_kernel<NT>), grid, dim3(256), 0, ctx->stream, mk(x), h,  \
                     has_t ? 1 : 0, stats)
  E2_MH_DISPATCH(h.tot, E2_MHF);
#undef E2_MHF
  E2_CHECK_HIP(hipGetLastError());
  return 0;
}

static long mh_tiles(int n, long S) { return ((S + MT - 1) / MT) * n; }

extern "C" size_t e2_multihead_bwd_workspace_bytes(int n, int cin, int sum_ncls, int d, int h,
                                                   int w) {
  if (n < 1 || cin < 1 || sum_ncls < 1 || d < 1 || h < 1 || w < 1) return 0;
  const long blocks = std::min<long>(mh_tiles(n, (long)d * h * w), 2L * 1024);   // any CU count
  return sizeof(float) * (size_t)blocks * ((size_t)sum_ncls * cin + sum_ncls);
}

extern "C" int e2_multihead_bwd(e2_ctx* ctx, const e2_tensor5* x, int k, const float* const* w,
                                const e2_tensor5* const* probs,
                                const e2_tensor5* const* targets, const float* coef,
                                const e2_tensor5* dx, int accumulate_dx, float* const* dw,
                                float* const* dbias, void* ws, size_t ws_bytes) {
  E2_REQUIRE(k >= 2 && k <= E2_MH_MAXK, "multihead_bwd: %d heads, 2..%d are supported", k,
             E2_MH_MAXK);
  E2_REQUIRE(probs, "multihead_bwd: null argument");
  int ncls[E2_MH_MAXK];
  for (int j = 0; j < k; ++j) {
    E2_REQUIRE(probs[j], "multihead_bwd: null probs of head %d", j);
    ncls[j] = probs[j]->c;
  }
  MHeads h{};
  bool has_t;
  if (int rc = mh_pack(ctx, "multihead_bwd", x, k, w, ncls, targets, true, probs, &h, &has_t))
    return rc;
  E2_REQUIRE(coef && dw && dbias && ws, "multihead_bwd: null argument");
  for (int j = 0; j < k; ++j) {
    E2_REQUIRE(dw[j] && dbias[j], "multihead_bwd: null gradient of head %d", j);
    h.dw[j] = dw[j];
    h.db[j] = dbias[j];
  }
  View5 vdx{};
  if (dx) {
    if (int rc = check_view(dx, "multihead_bwd dx")) return rc;
    E2_REQUIRE(dx->c == x->c && mh_same_sp(x, dx), "multihead_bwd: dx shape mismatch");
    vdx = mk(dx);
  }
  const long S = (long)x->d * x->h * x->w;
  const long tilesPerN = (S + MT - 1) / MT;
  const long nTiles = tilesPerN * x->n;
  E2_REQUIRE(nTiles < (1L << 31), "multihead_bwd: too many tiles");
  const int grid = (int)std::min<long>(nTiles, 2L * (ctx->num_cu > 0 ? ctx->num_cu : 256));
  const int total = h.tot * x->c + h.tot;
  E2_REQUIRE(ws_bytes >= sizeof(float) * (size_t)grid * total,
             "multihead_bwd: workspace too small");
  float* part = (float*)ws;
#define E2_MHB(NT)                                                                             \
  do {                                                                                         \
    static bool attr_done = false;                                                             \
    if (!attr_done) {                                                                          \
      E2_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&multihead_bwd_kernel<NT>), \
                                       hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024)); \
      attr_done = true;                                                                        \
    }                                                                                          \
    const size_t lds = sizeof(float) * ((size_t)NT * MT + (size_t)x->c * (MT + 1));            \
    hipLaunchKernelGGL((multihead_bwd_kernel<NT>), dim3(grid), dim3(256), lds, ctx->stream,    \
                       mk(x), h, coef, vdx, dx ? 1 : 0, accumulate_dx, part, (int)tilesPerN,   \
                       (int)nTiles);                                                           \
  } while (0)
  E2_MH_DISPATCH(h.tot, E2_MHB);
#undef E2_MHB
  E2_CHECK_HIP(hipGetLastError());
  hipLaunchKernelGGL(multihead_reduce_kernel, dim3(e2_cdiv(total, 256), std::min(grid, 16)),
                     dim3(256), 0, ctx->stream, part, grid, x->c, h);
  E2_CHECK_HIP(hipGetLastError());
  return 0;
}
