// bn_wide.hip -- batch normalisation + bias + relu / lin for conv-sized tensors
// (e2_batchnorm_wide_fwd / _bwd; neural.py:352-378 Perceptron, 681-711 Conv).  The arithmetic is that
// of csrc/dense_bn.hip (population std + 1e-6, out = act(a (x - mean) + b) with a = gamma / std,
// relu'(0) = 0.5, the gradient through the batch statistics in train mode); the split of the work is
// not: dense_bn.hip gives a channel to ONE work-group, which is right for config 1 and leaves 32
// work-groups on 256 CUs at (1, 32, 116, 132, 132).
//
// A channel is cut into G slabs of whole rows (a row: the w contiguous floats at one (n, z, y)); the
// grid is C x G work-groups of 256 threads.  An item is a quad, four consecutive x of one row, moved
// as one 16-byte access where the row piece is whole and 16-byte aligned in the view, element by
// element at row ends and on misaligned views.  A tile is 256 x 4 quads: thread t owns the quads
// t, t + 256, t + 512, t + 768 of the tile, 16 floats in registers, four loads in flight.
//
//   forward, train:  stats (C x G)  -> per slab: count, f32 sum S, pivot K (the mean of its first tile),
//                                      D = sum_t n_t (m_t - K), Q = sum_t [M2_t + n_t (m_t - K)^2]
//                                      where per tile S_t, m_t = S_t / n_t and M2_t = sum (x - m_t)^2
//                                      come from the SAME registers (one read of x)
//                    finish (C)     -> mean = (S_0 + S_1 + ...) / cnt, the second moment about that
//                                      mean from Q_g - 2 dl D_g + n_g dl^2 with dl = mean - K_g;
//                                      save, running statistics
//                    apply (C x G)  -> out = act(a (x - mean) + b)
//   forward, predict: apply alone, from run_mean / run_std
//   backward:        sums (C x G)   -> per slab: sum dpre, sum dpre xhat
//                    dx (C x G)     -> every work-group adds the G pairs in slab order; slab 0 does
//                                      dgamma += / dbias += ; dx = a (dpre - m_d - xhat m_dx std / (std - 1e-6))
//
// No atomics and no memset: every workspace word that is read was stored by the launch before it, in
// an order that depends on (n, c, d, h, w, G) alone -- not on strides, alignment or the device.  The
// quad geometry is relative to the row start, so the 16-byte and the element path put every value
// into the same register and the same place of every sum.  No variance is taken as E[x^2] - mean^2
// at the channel's scale: squares are taken about a tile's own mean, the parallel-axis terms about a
// pivot inside the data.
#include "stream_common.hpp"

namespace {

constexpr unsigned BNW_TILE = 1024;        // quads per tile: 256 threads x 4
constexpr int BNW_PART = 8;                // floats per slab record of the forward (5 used)
constexpr int BNW_WG_PER_CU = 4;           // auto rule: work-groups wanted per CU ...
constexpr int BNW_CUS = 256;               // ... of an MI355X, whatever device runs (results must not depend on it)
constexpr int BNW_AUTO_CAP = 64;           // ... at most this many slabs per channel
constexpr long BNW_MIN_SLAB = 8192;        // ... none below two tiles' worth of elements
constexpr int BNW_LIMIT = 1024;            // slabs a caller may ask for (and never more than rows)

typedef float bnw_f4 __attribute__((ext_vector_type(4)));

// rows = n * d * h of w floats each; slab g owns base + (g < rem) rows from g * base + min(g, rem)
struct BnwGeo {
  unsigned w, quads, h, dh, base, rem;
  FastDiv dq, ddh, dhh;
};

__device__ __forceinline__ void slab_of(const BnwGeo& p, unsigned g, unsigned& row0, unsigned& items) {
  row0 = g * p.base + min(g, p.rem);
  items = (p.base + (g < p.rem ? 1u : 0u)) * p.quads;
}
// item i of the slab that starts at row0: offset of its first element in `v`, elements it holds
__device__ __forceinline__ unsigned quad_of(const BnwGeo& p, unsigned row0, unsigned i,
                                            int& n, int& z, int& y, int& x0) {
  const unsigned rl = fdiv(i, p.dq);
  const unsigned row = row0 + rl;
  const unsigned nn = fdiv(row, p.ddh);
  const unsigned r2 = row - nn * p.dh;
  const unsigned zz = fdiv(r2, p.dhh);
  n = (int)nn; z = (int)zz; y = (int)(r2 - zz * p.h); x0 = (int)((i - rl * p.quads) << 2);
  return min(4u, p.w - (unsigned)x0);
}
// elements in the items [0, i) of a slab
__device__ __forceinline__ unsigned elems_before(const BnwGeo& p, unsigned i) {
  const unsigned rl = fdiv(i, p.dq);
  return rl * p.w + min((i - rl * p.quads) << 2, p.w);
}

__device__ __forceinline__ void load4(const float* s, unsigned nv, float (&v)[4]) {
  if (nv == 4u && (((uintptr_t)s) & 15) == 0) {
    const bnw_f4 t = *reinterpret_cast<const bnw_f4*>(s);
    v[0] = t[0]; v[1] = t[1]; v[2] = t[2]; v[3] = t[3];
  } else {
#pragma unroll
    for (unsigned e = 0; e < 4; ++e) v[e] = e < nv ? s[e] : 0.f;
  }
}
__device__ __forceinline__ void store4(float* d, unsigned nv, const float (&v)[4]) {
  if (nv == 4u && (((uintptr_t)d) & 15) == 0) {
    bnw_f4 t;
    t[0] = v[0]; t[1] = v[1]; t[2] = v[2]; t[3] = v[3];
    *reinterpret_cast<bnw_f4*>(d) = t;
  } else {
#pragma unroll
    for (unsigned e = 0; e < 4; ++e)
      if (e < nv) d[e] = v[e];
  }
}

// sum over the work-group, the same tree every time, valid in every thread.  One barrier: the
// callers alternate between two `red` arrays, so a value is read before its array is written again.
__device__ __forceinline__ float block_sum_all(float v, float* red) {
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

template <int ACT>
__device__ __forceinline__ float slope_of(float pre) {
  if (ACT == E2_ACT_RELU) return (pre > 0.f) ? 1.f : ((pre == 0.f) ? 0.5f : 0.f);
  return 1.f;
}

// ---- forward: statistics of one slab ----------------------------------------------------------------
__global__ __launch_bounds__(256) void e2bnw_stats_kernel(View5 x, BnwGeo p, float* ws, int G) {
  __shared__ float red_a[4], red_b[4];
  const unsigned c = blockIdx.x, g = blockIdx.y;
  unsigned row0, items;
  slab_of(p, g, row0, items);
  float S = 0.f, Q = 0.f, D = 0.f, K = 0.f;
  unsigned cnt = 0;
  for (unsigned t0 = 0; t0 < items; t0 += BNW_TILE) {
    float v[4][4];
    unsigned nv[4];
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const unsigned i = t0 + k * 256u + threadIdx.x;
      nv[k] = 0;
      v[k][0] = v[k][1] = v[k][2] = v[k][3] = 0.f;
      if (i < items) {
        int n, z, y, x0;
        nv[k] = quad_of(p, row0, i, n, z, y, x0);
        load4(x.p + vidx(x, n, (int)c, z, y, x0), nv[k], v[k]);
      }
      s += (v[k][0] + v[k][1]) + (v[k][2] + v[k][3]);
    }
    const unsigned nt = elems_before(p, min(t0 + BNW_TILE, items)) - elems_before(p, t0);
    const float fn = (float)nt;                                  // <= 4096: exact
    const float St = block_sum_all(s, red_a);
    const float mt = St / fn;
    float q = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
      for (unsigned e = 0; e < 4; ++e) {
        const float d = v[k][e] - mt;
        q += e < nv[k] ? d * d : 0.f;
      }
    const float Qt = block_sum_all(q, red_b);
    if (t0 == 0) K = mt;
    const float dk = mt - K;
    S += St;
    D += fn * dk;
    Q += Qt + fn * dk * dk;
    cnt += nt;
  }
  if (threadIdx.x == 0) {
    float* o = ws + ((long)c * G + g) * BNW_PART;
    o[0] = __uint_as_float(cnt);
    o[1] = S; o[2] = Q; o[3] = K; o[4] = D;
  }
}

// ---- forward: the G records of a channel -> mean, std (+ 1e-6) -----------------------------------------
__global__ __launch_bounds__(64) void e2bnw_finish_kernel(const float* ws, int C, int G, float fcnt,
                                                          float* run_mean, float* run_std, int update,
                                                          float* stats, float* save) {
  const int c = blockIdx.x * 64 + threadIdx.x;
  if (c >= C) return;
  const float* r = ws + (long)c * G * BNW_PART;
  float S = 0.f;
  for (int g = 0; g < G; ++g) S += r[g * BNW_PART + 1];
  const float mean = S / fcnt;
  float M2 = 0.f;
  for (int g = 0; g < G; ++g) {
    const float* o = r + g * BNW_PART;
    const float ng = (float)__float_as_uint(o[0]);
    const float dl = mean - o[3];
    M2 += o[2] + dl * (ng * dl - 2.f * o[4]);          // sum (x - mean)^2 of the slab, about its pivot
  }
  const float sd = sqrtf(fmaxf(M2, 0.f) / fcnt) + 1e-6f;
  if (update) {
    run_mean[c] = 0.9995f * run_mean[c] + 0.0005f * mean;
    run_std[c] = 0.9995f * run_std[c] + 0.0005f * sd;
  }
  stats[c] = mean; stats[C + c] = sd;
  if (save) { save[c] = mean; save[C + c] = sd; }
}

// ---- forward: out = act(a (x - mean) + b) -------------------------------------------------------------
template <int ACT>
__global__ __launch_bounds__(256) void e2bnw_apply_kernel(View5 x, View5 out, BnwGeo p, const float* gamma,
                                                          const float* bias, const float* mean_of,
                                                          const float* std_of, float* save) {
  const unsigned c = blockIdx.x, g = blockIdx.y;
  unsigned row0, items;
  slab_of(p, g, row0, items);
  const float mean = mean_of[c], sd = std_of[c];
  if (save && g == 0 && threadIdx.x == 0) { save[c] = mean; save[x.c + c] = sd; }   // (predict mode)
  const float a = gamma[c] / sd, b = bias[c];
  for (unsigned t0 = 0; t0 < items; t0 += BNW_TILE) {
    float v[4][4];
    unsigned nv[4];
    long off[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const unsigned i = t0 + k * 256u + threadIdx.x;
      nv[k] = 0;
      if (i < items) {
        int n, z, y, x0;
        nv[k] = quad_of(p, row0, i, n, z, y, x0);
        load4(x.p + vidx(x, n, (int)c, z, y, x0), nv[k], v[k]);
        off[k] = vidx(out, n, (int)c, z, y, x0);
      }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (nv[k] == 0) continue;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float r = a * (v[k][e] - mean) + b;
        v[k][e] = ACT == E2_ACT_RELU ? fmaxf(r, 0.f) : r;
      }
      store4(out.p + off[k], nv[k], v[k]);
    }
  }
}

// ---- backward: sum dpre, sum dpre xhat of one slab ----------------------------------------------------
template <int ACT>
__global__ __launch_bounds__(256) void e2bnw_bwd_sums_kernel(View5 dout, View5 x, BnwGeo p,
                                                             const float* gamma, const float* bias,
                                                             const float* save, float* ws, int G) {
  __shared__ float red_a[4], red_b[4];
  const unsigned c = blockIdx.x, g = blockIdx.y;
  unsigned row0, items;
  slab_of(p, g, row0, items);
  const float mean = save[c], sd = save[x.c + c];
  const float a = gamma[c] / sd, b = bias[c];
  float s1 = 0.f, s2 = 0.f;
  for (unsigned t0 = 0; t0 < items; t0 += BNW_TILE) {
    float xv[4][4], dv[4][4];
    unsigned nv[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const unsigned i = t0 + k * 256u + threadIdx.x;
      nv[k] = 0;
      if (i < items) {
        int n, z, y, x0;
        nv[k] = quad_of(p, row0, i, n, z, y, x0);
        load4(x.p + vidx(x, n, (int)c, z, y, x0), nv[k], xv[k]);
        load4(dout.p + vidx(dout, n, (int)c, z, y, x0), nv[k], dv[k]);
      }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
      for (unsigned e = 0; e < 4; ++e)
        if (e < nv[k]) {
          const float xc = xv[k][e] - mean;
          const float d = dv[k][e] * slope_of<ACT>(a * xc + b);     // pre as the forward computed it
          s1 += d;
          s2 += d * (xc / sd);
        }
  }
  const float t1 = block_sum_all(s1, red_a);
  const float t2 = block_sum_all(s2, red_b);
  if (threadIdx.x == 0) {
    float* o = ws + ((long)c * G + g) * 2;
    o[0] = t1; o[1] = t2;
  }
}

// ---- backward: the G pairs of a channel; dgamma, dbias (slab 0); dx -----------------------------------
template <int ACT>
__global__ __launch_bounds__(256) void e2bnw_bwd_dx_kernel(View5 dout, View5 x, View5 dx, BnwGeo p,
                                                           const float* gamma, const float* bias,
                                                           const float* save, const float* ws, int G,
                                                           float fcnt, int train, float* dgamma,
                                                           float* dbias) {
  const unsigned c = blockIdx.x, g = blockIdx.y;
  float sum_d = 0.f, sum_dx = 0.f;
  const float* r = ws + (long)c * G * 2;
  for (int q = 0; q < G; ++q) { sum_d += r[2 * q]; sum_dx += r[2 * q + 1]; }
  if (g == 0 && threadIdx.x == 0) {
    if (dbias) dbias[c] += sum_d;
    if (dgamma) dgamma[c] += sum_dx;
  }
  if (!dx.p) return;
  unsigned row0, items;
  slab_of(p, g, row0, items);
  const float mean = save[c], sd = save[x.c + c];
  const float a = gamma[c] / sd, b = bias[c];
  const float m_d = train ? sum_d / fcnt : 0.f;
  const float s0 = sd - 1e-6f;                               // the bare standard deviation
  const float m_dx = (train && s0 > 0.f) ? (sum_dx / fcnt) * (sd / s0) : 0.f;
  for (unsigned t0 = 0; t0 < items; t0 += BNW_TILE) {
    float xv[4][4], dv[4][4];
    unsigned nv[4];
    long off[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const unsigned i = t0 + k * 256u + threadIdx.x;
      nv[k] = 0;
      if (i < items) {
        int n, z, y, x0;
        nv[k] = quad_of(p, row0, i, n, z, y, x0);
        load4(x.p + vidx(x, n, (int)c, z, y, x0), nv[k], xv[k]);
        load4(dout.p + vidx(dout, n, (int)c, z, y, x0), nv[k], dv[k]);
        off[k] = vidx(dx, n, (int)c, z, y, x0);
      }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (nv[k] == 0) continue;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float xc = xv[k][e] - mean;
        const float d = dv[k][e] * slope_of<ACT>(a * xc + b);
        dv[k][e] = a * (d - m_d - (xc / sd) * m_dx);
      }
      store4(dx.p + off[k], nv[k], dv[k]);
    }
  }
}

// ---- host: the slab rule -------------------------------------------------------------------------------
struct BnwChoice {
  int slabs, rows_per, limit;
  long rows;
  BnwGeo geo;
};

// splits = 0: enough slabs for BNW_WG_PER_CU work-groups on each of 256 CUs, at most BNW_AUTO_CAP,
// none smaller than BNW_MIN_SLAB elements; splits >= 1: that many (the caller checks the limit)
static int bnw_choose(const char* who, int n, int c, int d, int h, int w, int splits, BnwChoice* out) {
  E2_REQUIRE(n > 0 && c > 0 && d > 0 && h > 0 && w > 0 && splits >= 0,
             "%s: bad shape (%d,%d,%d,%d,%d) or splits %d", who, n, c, d, h, w, splits);
  const long rows = (long)n * d * h, quads = (w + 3) / 4;
  E2_REQUIRE(rows * quads < (1L << 31) && rows * (long)w < (1L << 31), "%s: channel too large", who);
  const int limit = (int)(rows < BNW_LIMIT ? rows : BNW_LIMIT);
  int G = splits;
  if (G == 0) {
    const long want = (BNW_WG_PER_CU * BNW_CUS + c - 1) / c, fit = rows * w / BNW_MIN_SLAB;
    long g = want < BNW_AUTO_CAP ? want : BNW_AUTO_CAP;
    g = g < fit ? g : fit;
    g = g < limit ? g : limit;
    G = (int)(g < 1 ? 1 : g);
  }
  E2_REQUIRE(G <= limit, "%s: %d splits asked for, a channel of %ld rows allows at most %d", who, G,
             rows, limit);
  out->slabs = G; out->limit = limit; out->rows = rows;
  BnwGeo& p = out->geo;
  p.w = (unsigned)w; p.quads = (unsigned)quads; p.h = (unsigned)h; p.dh = (unsigned)(d * h);
  p.base = (unsigned)(rows / G); p.rem = (unsigned)(rows % G);
  p.dq = mk_div(p.quads); p.ddh = mk_div(p.dh); p.dhh = mk_div(p.h);
  out->rows_per = (int)(p.base + (p.rem ? 1 : 0));
  return 0;
}
static size_t bnw_fwd_floats(int c, int G) { return (size_t)c * G * BNW_PART + 2 * (size_t)c; }
static size_t bnw_bwd_floats(int c, int G) { return (size_t)c * G * 2; }

}  // namespace

extern "C" int e2_batchnorm_wide_choice(int n, int c, int d, int h, int w, int splits, int* out4) {
  E2_REQUIRE(out4, "batchnorm_wide_choice: null argument");
  BnwChoice ch;
  if (int rc = bnw_choose("batchnorm_wide_choice", n, c, d, h, w, splits, &ch)) return rc;
  out4[0] = ch.slabs; out4[1] = ch.rows_per; out4[2] = c * ch.slabs; out4[3] = ch.limit;
  return 0;
}

extern "C" size_t e2_batchnorm_wide_workspace_bytes(int n, int c, int d, int h, int w, int splits) {
  BnwChoice ch;
  if (bnw_choose("batchnorm_wide_workspace_bytes", n, c, d, h, w, splits, &ch)) return 0;
  const size_t f = bnw_fwd_floats(c, ch.slabs), b = bnw_bwd_floats(c, ch.slabs);
  return sizeof(float) * (f > b ? f : b);
}

extern "C" int e2_batchnorm_wide_fwd(e2_ctx* ctx, const e2_tensor5* x, const float* gamma,
                                     const float* bias, float* run_mean, float* run_std, int train,
                                     int update_running, int act, const e2_tensor5* out, float* save,
                                     int splits, void* ws, size_t ws_bytes) {
  const char* who = "batchnorm_wide_fwd";
  E2_REQUIRE(ctx && gamma && bias, "%s: null argument", who);
  if (int rc = check_view(x, "batchnorm_wide_fwd x")) return rc;
  if (int rc = check_view(out, "batchnorm_wide_fwd out")) return rc;
  E2_REQUIRE(same_size(x, out), "%s: x / out shape mismatch", who);
  E2_REQUIRE(act == E2_ACT_LIN || act == E2_ACT_RELU, "%s: bad act %d", who, act);
  E2_REQUIRE(train || (run_mean && run_std), "%s: predict mode needs the stored statistics", who);
  E2_REQUIRE(!update_running || (train && run_mean && run_std),
             "%s: running statistics are updated in train mode only", who);
  BnwChoice ch;
  if (int rc = bnw_choose(who, x->n, x->c, x->d, x->h, x->w, splits, &ch)) return rc;
  const int C = x->c, G = ch.slabs;
  const dim3 grid((unsigned)C, (unsigned)G), block(256);
  const View5 vx = mk(x), vo = mk(out);
  const float* mean_of = run_mean;
  const float* std_of = run_std;
  if (train) {
    const size_t need = sizeof(float) * bnw_fwd_floats(C, G);
    E2_REQUIRE(ws && ws_bytes >= need, "%s: %d slabs of %d channels need a workspace of %zu bytes, got %zu",
               who, G, C, need, ws ? ws_bytes : (size_t)0);
    float* part = (float*)ws;
    float* stats = part + (size_t)C * G * BNW_PART;
    hipLaunchKernelGGL(e2bnw_stats_kernel, grid, block, 0, ctx->stream, vx, ch.geo, part, G);
    hipLaunchKernelGGL(e2bnw_finish_kernel, dim3((unsigned)((C + 63) / 64)), dim3(64), 0, ctx->stream,
                       part, C, G, (float)(ch.rows * x->w), run_mean, run_std, update_running ? 1 : 0,
                       stats, save);
    mean_of = stats; std_of = stats + C;
    save = nullptr;                                   // (written by the finish)
  }
  if (act == E2_ACT_RELU)
    hipLaunchKernelGGL(e2bnw_apply_kernel<E2_ACT_RELU>, grid, block, 0, ctx->stream, vx, vo, ch.geo,
                       gamma, bias, mean_of, std_of, save);
  else
    hipLaunchKernelGGL(e2bnw_apply_kernel<E2_ACT_LIN>, grid, block, 0, ctx->stream, vx, vo, ch.geo,
                       gamma, bias, mean_of, std_of, save);
  E2_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" int e2_batchnorm_wide_bwd(e2_ctx* ctx, const e2_tensor5* dout, const e2_tensor5* x,
                                     const float* gamma, const float* bias, const float* save,
                                     int train, int act, const e2_tensor5* dx, float* dgamma,
                                     float* dbias, int splits, void* ws, size_t ws_bytes) {
  const char* who = "batchnorm_wide_bwd";
  E2_REQUIRE(ctx && gamma && bias && save, "%s: null argument", who);
  if (int rc = check_view(dout, "batchnorm_wide_bwd dout")) return rc;
  if (int rc = check_view(x, "batchnorm_wide_bwd x")) return rc;
  E2_REQUIRE(same_size(x, dout), "%s: x / dout shape mismatch", who);
  E2_REQUIRE(act == E2_ACT_LIN || act == E2_ACT_RELU, "%s: bad act %d", who, act);
  View5 vdx{nullptr, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  if (dx) {
    if (int rc = check_view(dx, "batchnorm_wide_bwd dx")) return rc;
    E2_REQUIRE(same_size(x, dx), "%s: x / dx shape mismatch", who);
    vdx = mk(dx);
  }
  BnwChoice ch;
  if (int rc = bnw_choose(who, x->n, x->c, x->d, x->h, x->w, splits, &ch)) return rc;
  const int C = x->c, G = ch.slabs;
  const size_t need = sizeof(float) * bnw_bwd_floats(C, G);
  E2_REQUIRE(ws && ws_bytes >= need, "%s: %d slabs of %d channels need a workspace of %zu bytes, got %zu",
             who, G, C, need, ws ? ws_bytes : (size_t)0);
  float* part = (float*)ws;
  const dim3 grid((unsigned)C, (unsigned)G), block(256);
  const dim3 grid_dx((unsigned)C, dx ? (unsigned)G : 1u);      // without dx: the channel's one writer
  const View5 vg = mk(dout), vx = mk(x);
  const float fcnt = (float)(ch.rows * x->w);
  if (act == E2_ACT_RELU) {
    hipLaunchKernelGGL(e2bnw_bwd_sums_kernel<E2_ACT_RELU>, grid, block, 0, ctx->stream, vg, vx, ch.geo,
                       gamma, bias, save, part, G);
    hipLaunchKernelGGL(e2bnw_bwd_dx_kernel<E2_ACT_RELU>, grid_dx, block, 0, ctx->stream, vg, vx, vdx,
                       ch.geo, gamma, bias, save, part, G, fcnt, train ? 1 : 0, dgamma, dbias);
  } else {
    hipLaunchKernelGGL(e2bnw_bwd_sums_kernel<E2_ACT_LIN>, grid, block, 0, ctx->stream, vg, vx, ch.geo,
                       gamma, bias, save, part, G);
    hipLaunchKernelGGL(e2bnw_bwd_dx_kernel<E2_ACT_LIN>, grid_dx, block, 0, ctx->stream, vg, vx, vdx,
                       ch.geo, gamma, bias, save, part, G, fcnt, train ? 1 : 0, dgamma, dbias);
  }
  E2_CHECK_HIP(hipGetLastError());
  return 0;
}
