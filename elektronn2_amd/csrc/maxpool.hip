// maxpool.hip -- max-pool + bias + activation (forward and backward), stand-alone max-pool, the
// backward of the fused conv + bias + activation, and the depth-to-space pass of UpConv's backward.
// All are W-contiguous (coalesced) streaming kernels bound by HBM; reductions go
// wave-shuffle -> LDS -> one atomic per work-group.
#include "stream_common.hpp"

// ---------------------------------------------------------------------------
// max-pool (+bias +act) forward:  out = act(max_window(y) + b[c])
// grid: (chunks of the (z,y,x) output range, c, n); 32-bit index math with
// magic-number division; each thread walks its chunk with stride 256.
// ---------------------------------------------------------------------------

template <bool HAS_BIAS>
__global__ __launch_bounds__(256) void pool_fwd_kernel(View5 y, const float* __restrict__ bias,
                                                       int pz, int py, int px, int act,
                                                       View5 out, FastDiv dw, FastDiv dh,
                                                       unsigned chunk) {
  const unsigned S = (unsigned)out.d * out.h * out.w;
  const unsigned s0 = blockIdx.x * chunk;
  const unsigned s1 = min(s0 + chunk, S);
  const int c = blockIdx.y, n = blockIdx.z;
  const float bv = HAS_BIAS ? bias[c] : 0.f;
  const float* ybase = y.p + (long)n * y.sn + (long)c * y.sc;
  float* obase = out.p + (long)n * out.sn + (long)c * out.sc;
  for (unsigned s = s0 + threadIdx.x; s < s1; s += 256) {
    const unsigned t = fdiv(s, dw);
    const unsigned xo = s - t * out.w;
    const unsigned zo = fdiv(t, dh);
    const unsigned yo = t - zo * out.h;
    const float* src = ybase + (long)(zo * pz) * y.sd + (long)(yo * py) * y.sh + xo * px;
    float m = src[0];
    for (int a = 0; a < pz; ++a)
      for (int b = 0; b < py; ++b) {
        const float* row = src + a * y.sd + b * y.sh;
        for (int e = 0; e < px; ++e) m = fmaxf(m, row[e]);
      }
    float v = m + bv;
    if (act == E2_ACT_RELU) v = fmaxf(v, 0.f);
    obase[(long)zo * out.sd + (long)yo * out.sh + xo] = v;
  }
}

// backward: dy[window] = (y == max) ? dout * act'(max + b) : 0 ; dbias += sum
template <bool HAS_BIAS>
__global__ __launch_bounds__(256) void pool_bwd_kernel(View5 dout, View5 y,
                                                       const float* __restrict__ bias, int pz,
                                                       int py, int px, int act, View5 dy,
                                                       float* __restrict__ dbias,
                                                       int accumulate, FastDiv dw,
                                                       FastDiv dh, unsigned chunk) {
  __shared__ float red[4];
  const unsigned S = (unsigned)dout.d * dout.h * dout.w;
  const unsigned s0 = blockIdx.x * chunk;
  const unsigned s1 = min(s0 + chunk, S);
  const int c = blockIdx.y, n = blockIdx.z;
  const float bv = HAS_BIAS ? bias[c] : 0.f;
  const float* ybase = y.p + (long)n * y.sn + (long)c * y.sc;
  const float* gbase = dout.p + (long)n * dout.sn + (long)c * dout.sc;
  float* dbase = dy.p + (long)n * dy.sn + (long)c * dy.sc;
  float gsum = 0.f;
  for (unsigned s = s0 + threadIdx.x; s < s1; s += 256) {
    const unsigned t = fdiv(s, dw);
    const unsigned xo = s - t * dout.w;
    const unsigned zo = fdiv(t, dh);
    const unsigned yo = t - zo * dout.h;
    const float* src = ybase + (long)(zo * pz) * y.sd + (long)(yo * py) * y.sh + xo * px;
    float m = src[0];
    for (int a = 0; a < pz; ++a)
      for (int b = 0; b < py; ++b) {
        const float* row = src + a * y.sd + b * y.sh;
        for (int e = 0; e < px; ++e) m = fmaxf(m, row[e]);
      }
    float g = gbase[(long)zo * dout.sd + (long)yo * dout.sh + xo];
    if (act == E2_ACT_RELU) {
      const float pre = m + bv;
      g *= (pre > 0.f) ? 1.f : ((pre == 0.f) ? 0.5f : 0.f);
    }
    gsum += g;
    float* dst = dbase + (long)(zo * pz) * dy.sd + (long)(yo * py) * dy.sh + xo * px;
    for (int a = 0; a < pz; ++a)
      for (int b = 0; b < py; ++b) {
        const float* row = src + a * y.sd + b * y.sh;
        float* drow = dst + a * dy.sd + b * dy.sh;
        for (int e = 0; e < px; ++e) {
          const float v = (row[e] == m) ? g : 0.f;
          drow[e] = accumulate ? (drow[e] + v) : v;
        }
      }
  }
  if (dbias != nullptr) {
    const float tot = block_sum256(gsum, red);
    if (threadIdx.x == 0 && tot != 0.f) unsafeAtomicAdd(dbias + c, tot);
  }
}

// Fixed-window forms of the two kernels above for the pool shapes of the BASELINE nets
// ((1,2,2), (2,1,1), (2,2,2), and (1,1,1) = bias + activation of a layer that does not
// pool): a thread owns FOUR consecutive input x (16-byte row accesses, any alignment) =
// 4 / PX pooled outputs; the window lives in registers (read once), the loops are
// compile-time.  (The one-output-per-thread forms with 4- and 8-byte accesses ran at
// 2.2-3.1 TB/s.)
typedef float pw_f4 __attribute__((ext_vector_type(4), aligned(4)));
typedef float pw_f2 __attribute__((ext_vector_type(2), aligned(4)));
// nv valid elements of a row piece (the others read as `pad`)
__device__ __forceinline__ void pw_load4(const float* row, int nv, float pad, float (&w)[4]) {
  if (nv == 4) {
    const pw_f4 v = *reinterpret_cast<const pw_f4*>(row);
    w[0] = v[0]; w[1] = v[1]; w[2] = v[2]; w[3] = v[3];
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) w[e] = e < nv ? row[e] : pad;
  }
}
__device__ __forceinline__ void pw_store4(float* row, int nv, const float (&v)[4]) {
  if (nv == 4) {
    const pw_f4 o = {v[0], v[1], v[2], v[3]};
    *reinterpret_cast<pw_f4*>(row) = o;
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) if (e < nv) row[e] = v[e];
  }
}
template <int NO>
__device__ __forceinline__ void pw_loadN(const float* p, int nv, float (&g)[NO]) {
  if (nv == NO) {
    if constexpr (NO == 4) {
      const pw_f4 v = *reinterpret_cast<const pw_f4*>(p);
      g[0] = v[0]; g[1] = v[1]; g[2] = v[2]; g[3] = v[3];
    } else {
      const pw_f2 v = *reinterpret_cast<const pw_f2*>(p);
      g[0] = v[0]; g[1] = v[1];
    }
  } else {
#pragma unroll
    for (int e = 0; e < NO; ++e) g[e] = e < nv ? p[e] : 0.f;
  }
}
template <int NO>
__device__ __forceinline__ void pw_storeN(float* p, int nv, const float (&g)[NO]) {
  if (nv == NO) {
    if constexpr (NO == 4) {
      const pw_f4 o = {g[0], g[1], g[2], g[3]};
      *reinterpret_cast<pw_f4*>(p) = o;
    } else {
      const pw_f2 o = {g[0], g[1]};
      *reinterpret_cast<pw_f2*>(p) = o;
    }
  } else {
#pragma unroll
    for (int e = 0; e < NO; ++e) if (e < nv) p[e] = g[e];
  }
}
constexpr int kMaxParts = 8;      // split-K partial-sum slabs a consumer adds up (e2hip.h)
template <int PZ, int PY, int PX, bool HAS_BIAS>
__global__ __launch_bounds__(256) void pool_fwd_fixed_kernel(View5 y, const float* __restrict__ bias,
                                                             int act, View5 out, FastDiv dvw,
                                                             FastDiv dh, unsigned chunk,
                                                             int nparts, long pstride) {
  static_assert(PX == 1 || PX == 2, "x windows of 1 or 2");
  constexpr int NO = 4 / PX;                                  // pooled outputs per thread
  const unsigned VW = ((unsigned)out.w + NO - 1) / NO;        // pieces per output row
  const unsigned S = (unsigned)out.d * out.h * VW;
  const unsigned s0 = blockIdx.x * chunk;
  const unsigned s1 = min(s0 + chunk, S);
  const int c = blockIdx.y, n = blockIdx.z;
  const float bv = HAS_BIAS ? bias[c] : 0.f;
  float* ybase = y.p + (long)n * y.sn + (long)c * y.sc;
  float* __restrict__ obase = out.p + (long)n * out.sn + (long)c * out.sc;
#pragma unroll 2
  for (unsigned s = s0 + threadIdx.x; s < s1; s += 256) {
    const unsigned t = fdiv(s, dvw);
    const unsigned xo = (s - t * VW) * NO;
    const unsigned zo = fdiv(t, dh);
    const unsigned yo = t - zo * out.h;
    const int nvo = min(NO, out.w - (int)xo);
    float* src = ybase + (long)(zo * PZ) * y.sd + (long)(yo * PY) * y.sh + xo * PX;
    float m[NO];
#pragma unroll
    for (int j = 0; j < NO; ++j) m[j] = -INFINITY;
#pragma unroll
    for (int a = 0; a < PZ; ++a)
#pragma unroll
      for (int b = 0; b < PY; ++b) {
        float w[4];
        float* row = src + a * y.sd + b * y.sh;
        pw_load4(row, nvo * PX, 0.f, w);
        if (nparts > 1) {      // split-K partial sums: add them up, leave the sum in part 0
          // (all parts requested before the first add: a load per loop trip cost the
          // launches of neuro3d's 0.5-2 MB layers 8 dependent round trips, 5.8 us each)
          float u[kMaxParts - 1][4];
#pragma unroll
          for (int q = 1; q < kMaxParts; ++q)
            if (q < nparts) pw_load4(row + q * pstride, nvo * PX, 0.f, u[q - 1]);
#pragma unroll
          for (int q = 1; q < kMaxParts; ++q)
            if (q < nparts) {
#pragma unroll
              for (int e = 0; e < 4; ++e) w[e] += u[q - 1][e];
            }
          pw_store4(row, nvo * PX, w);
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) m[e / PX] = fmaxf(m[e / PX], w[e]);
      }
    float v[NO];
#pragma unroll
    for (int j = 0; j < NO; ++j) {
      v[j] = m[j] + bv;
      if (act == E2_ACT_RELU) v[j] = fmaxf(v[j], 0.f);
    }
    pw_storeN<NO>(obase + (long)zo * out.sd + (long)yo * out.sh + xo, nvo, v);
  }
}
template <int PZ, int PY, int PX, bool HAS_BIAS>
__global__ __launch_bounds__(256) void pool_bwd_fixed_kernel(View5 dout, View5 y,
                                                             const float* __restrict__ bias,
                                                             int act, View5 dy,
                                                             float* __restrict__ dbias,
                                                             int accumulate, FastDiv dvw,
                                                             FastDiv dh, unsigned chunk,
                                                             int gparts, long gstride) {
  static_assert(PX == 1 || PX == 2, "x windows of 1 or 2");
  constexpr int NO = 4 / PX;
  __shared__ float red[4];
  const unsigned VW = ((unsigned)dout.w + NO - 1) / NO;
  const unsigned S = (unsigned)dout.d * dout.h * VW;
  const unsigned s0 = blockIdx.x * chunk;
  const unsigned s1 = min(s0 + chunk, S);
  const int c = blockIdx.y, n = blockIdx.z;
  const float bv = HAS_BIAS ? bias[c] : 0.f;
  const float* __restrict__ ybase = y.p + (long)n * y.sn + (long)c * y.sc;
  const float* __restrict__ gbase = dout.p + (long)n * dout.sn + (long)c * dout.sc;
  float* __restrict__ dbase = dy.p + (long)n * dy.sn + (long)c * dy.sc;
  float gsum = 0.f;
#pragma unroll 2
  for (unsigned s = s0 + threadIdx.x; s < s1; s += 256) {
    const unsigned t = fdiv(s, dvw);
    const unsigned xo = (s - t * VW) * NO;
    const unsigned zo = fdiv(t, dh);
    const unsigned yo = t - zo * dout.h;
    const int nvo = min(NO, dout.w - (int)xo);
    const int nvi = nvo * PX;
    const float* src = ybase + (long)(zo * PZ) * y.sd + (long)(yo * PY) * y.sh + xo * PX;
    float w[PZ][PY][4];
    float m[NO];
#pragma unroll
    for (int j = 0; j < NO; ++j) m[j] = -INFINITY;
#pragma unroll
    for (int a = 0; a < PZ; ++a)
#pragma unroll
      for (int b = 0; b < PY; ++b) {
        pw_load4(src + a * y.sd + b * y.sh, nvi, 0.f, w[a][b]);
#pragma unroll
        for (int e = 0; e < 4; ++e) m[e / PX] = fmaxf(m[e / PX], w[a][b][e]);
      }
    float g[NO];
    pw_loadN<NO>(gbase + (long)zo * dout.sd + (long)yo * dout.sh + xo, nvo, g);
    if (gparts > 1) {                       // dout arrives as split-K partial sums
      float u[kMaxParts - 1][NO];
#pragma unroll
      for (int q = 1; q < kMaxParts; ++q)
        if (q < gparts)
          pw_loadN<NO>(gbase + q * gstride + (long)zo * dout.sd + (long)yo * dout.sh + xo, nvo, u[q - 1]);
#pragma unroll
      for (int q = 1; q < kMaxParts; ++q)
        if (q < gparts) {
#pragma unroll
          for (int j = 0; j < NO; ++j) g[j] += u[q - 1][j];
        }
    }
#pragma unroll
    for (int j = 0; j < NO; ++j) {
      if (act == E2_ACT_RELU) {
        const float pre = m[j] + bv;
        g[j] *= (pre > 0.f) ? 1.f : ((pre == 0.f) ? 0.5f : 0.f);
      }
      if (j < nvo) gsum += g[j];
    }
    float* dst = dbase + (long)(zo * PZ) * dy.sd + (long)(yo * PY) * dy.sh + xo * PX;
#pragma unroll
    for (int a = 0; a < PZ; ++a)
#pragma unroll
      for (int b = 0; b < PY; ++b) {
        float* drow = dst + a * dy.sd + b * dy.sh;
        float v[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = (w[a][b][e] == m[e / PX]) ? g[e / PX] : 0.f;
        if (accumulate) {
          float old[4];
          pw_load4(drow, nvi, 0.f, old);
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] += old[e];
        }
        pw_store4(drow, nvi, v);
      }
  }
  if (dbias != nullptr) {
    const float tot = block_sum256(gsum, red);
    if (threadIdx.x == 0 && tot != 0.f) unsafeAtomicAdd(dbias + c, tot);
  }
}

// backward of the FUSED conv+bias+act forward (no pooling): dy = dout * act'(out),
// relu' read off the activated output: > 0 -> 1, +0.0 -> 0.5 (pre-activation was
// exactly 0), -0.0 -> 0 (it was negative; see e2_conv3d_fwd_packed_act); dbias += sum
// (four consecutive x per thread, 16-byte accesses -- the scalar form ran at 2.9 TB/s)
__global__ __launch_bounds__(256) void act_bwd_out_kernel(View5 dout, View5 out, int act,
                                                          View5 dy, float* __restrict__ dbias,
                                                          FastDiv dvw, FastDiv dh,
                                                          unsigned chunk, int gparts,
                                                          long gstride) {
  __shared__ float red[4];
  const unsigned VW = (unsigned)(dout.w + 3) >> 2;            // 4-element pieces per row
  const unsigned S = (unsigned)dout.d * dout.h * VW;
  const unsigned s0 = blockIdx.x * chunk;
  const unsigned s1 = min(s0 + chunk, S);
  const int c = blockIdx.y, n = blockIdx.z;
  const float* obase = out.p + (long)n * out.sn + (long)c * out.sc;
  const float* gbase = dout.p + (long)n * dout.sn + (long)c * dout.sc;
  float* dbase = dy.p + (long)n * dy.sn + (long)c * dy.sc;
  float gsum = 0.f;
  for (unsigned s = s0 + threadIdx.x; s < s1; s += 256) {
    const unsigned t = fdiv(s, dvw);
    const unsigned xo = (s - t * VW) << 2;
    const unsigned zo = fdiv(t, dh);
    const unsigned yo = t - zo * dout.h;
    const float* gp = gbase + (long)zo * dout.sd + (long)yo * dout.sh + xo;
    const float* op = obase + (long)zo * out.sd + (long)yo * out.sh + xo;
    float* dp = dbase + (long)zo * dy.sd + (long)yo * dy.sh + xo;
    const int nv = min(4, dout.w - (int)xo);
    float g[4], o[4];
    if (nv == 4) {
      const pw_f4 gv = *reinterpret_cast<const pw_f4*>(gp);
      const pw_f4 ov = *reinterpret_cast<const pw_f4*>(op);
#pragma unroll
      for (int e = 0; e < 4; ++e) { g[e] = gv[e]; o[e] = ov[e]; }
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) { g[e] = e < nv ? gp[e] : 0.f; o[e] = e < nv ? op[e] : 1.f; }
    }
    if (gparts > 1) {                       // dout arrives as split-K partial sums
      float u[kMaxParts - 1][4];
#pragma unroll
      for (int q = 1; q < kMaxParts; ++q)
        if (q < gparts) pw_load4(gp + q * gstride, nv, 0.f, u[q - 1]);
#pragma unroll
      for (int q = 1; q < kMaxParts; ++q)
        if (q < gparts) {
#pragma unroll
          for (int e = 0; e < 4; ++e) g[e] += u[q - 1][e];
        }
    }
    if (act == E2_ACT_RELU) {
#pragma unroll
      for (int e = 0; e < 4; ++e) g[e] *= (o[e] > 0.f) ? 1.f : (__builtin_signbit(o[e]) ? 0.f : 0.5f);
    }
    gsum += (g[0] + g[1]) + (g[2] + g[3]);
    if (nv == 4) {
      pw_f4 v = {g[0], g[1], g[2], g[3]};
      *reinterpret_cast<pw_f4*>(dp) = v;
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) if (e < nv) dp[e] = g[e];
    }
  }
  if (dbias != nullptr) {
    const float tot = block_sum256(gsum, red);
    if (threadIdx.x == 0 && tot != 0.f) unsafeAtomicAdd(dbias + c, tot);
  }
}

// ---------------------------------------------------------------------------
// UpConv helpers: dpre in space-to-depth layout
//   s2d[n][co*R + r][z][y][x] = dout[n][co][pz*z+rz][py*y+ry][px*x+rx] * act'(yout)
// one thread per dout element (reads coalesced), dbias[co] += sum
// ---------------------------------------------------------------------------
__global__ void upconv_dpre_s2d_kernel(View5 dout, View5 yout, int pz, int py, int px,
                                       int act, float* __restrict__ s2d,
                                       float* __restrict__ dbias, FastDiv dw, FastDiv dh,
                                       FastDiv dpz, FastDiv dpy, FastDiv dpx, unsigned chunk) {
  // 32-bit index math with magic-number division (the 64-bit % and / of the first
  // version made this kernel ALU-bound at ~0.7 TB/s), a chunk of positions per work-group
  __shared__ float red[4];
  const unsigned S = (unsigned)dout.d * dout.h * dout.w;
  const unsigned s0 = blockIdx.x * chunk;
  const unsigned s1 = min(s0 + chunk, S);
  const int c = blockIdx.y, n = blockIdx.z;
  const unsigned R = pz * py * px;
  const unsigned di = dout.d / pz, hi = dout.h / py, wi = dout.w / px;
  const float* gb = dout.p + (long)n * dout.sn + (long)c * dout.sc;
  const float* ob = yout.p + (long)n * yout.sn + (long)c * yout.sc;
  float* sb = s2d + ((long)n * dout.c + c) * (long)R * di * hi * wi;
  float gsum = 0.f;
  for (unsigned s = s0 + threadIdx.x; s < s1; s += 256) {
    const unsigned t = fdiv(s, dw);
    const unsigned x = s - t * dout.w;
    const unsigned z = fdiv(t, dh);
    const unsigned y = t - z * dout.h;
    float g = gb[(long)z * dout.sd + (long)y * dout.sh + x];
    if (act == E2_ACT_RELU) {
      const float o = ob[(long)z * yout.sd + (long)y * yout.sh + x];
      g = (o > 0.f) ? g : 0.f;
    }
    const unsigned zi = fdiv(z, dpz), rz = z - zi * pz;
    const unsigned yi = fdiv(y, dpy), ry = y - yi * py;
    const unsigned xi = fdiv(x, dpx), rx = x - xi * px;
    const unsigned r = (rz * py + ry) * px + rx;
    sb[((long)r * di + zi) * (hi * wi) + yi * wi + xi] = g;
    gsum += g;
  }
  if (dbias != nullptr) {
    const float tot = block_sum256(gsum, red);
    if (threadIdx.x == 0 && tot != 0.f) unsafeAtomicAdd(dbias + c, tot);
  }
}

// outputs per work-group: enough groups to fill the chip (>= ~2048), at most
// 4096 per group so that per-channel reductions need few atomics
static unsigned pw_chunk(const View5& v) {
  const long S = (long)v.d * v.h * v.w;
  long per = (S * v.c * v.n) / 2048;
  per = ((per + 255) / 256) * 256;
  if (per < 256) per = 256;
  if (per > 4096) per = 4096;
  return (unsigned)per;
}
static dim3 grid_chunked(const View5& v, unsigned chunk) {
  const long S = (long)v.d * v.h * v.w;
  return dim3((unsigned)((S + chunk - 1) / chunk), (unsigned)v.c, (unsigned)v.n);
}

// the grid of the fixed-window kernels counts pieces of 4 input x (4 / PX outputs)
template <int PZ, int PY, int PX>
static void launch_pool_fwd_fixed(e2_ctx* ctx, const View5& vy, const float* bias, int act,
                                  const View5& vo, int nparts = 1, long pstride = 0) {
  View5 vq = vo; vq.w = (vo.w + 4 / PX - 1) / (4 / PX);
  const unsigned chunk = pw_chunk(vq);
  const dim3 g = grid_chunked(vq, chunk);
  const FastDiv dvw = mk_div(vq.w), dh = mk_div(vo.h);
  if (bias)
    hipLaunchKernelGGL((pool_fwd_fixed_kernel<PZ, PY, PX, true>), g, dim3(256), 0, ctx->stream,
                       vy, bias, act, vo, dvw, dh, chunk, nparts, pstride);
  else
    hipLaunchKernelGGL((pool_fwd_fixed_kernel<PZ, PY, PX, false>), g, dim3(256), 0, ctx->stream,
                       vy, bias, act, vo, dvw, dh, chunk, nparts, pstride);
}
template <int PZ, int PY, int PX>
static void launch_pool_bwd_fixed(e2_ctx* ctx, const View5& vd, const View5& vy, const float* bias,
                                  int act, const View5& vdy, float* dbias, int accumulate,
                                  int gparts = 1, long gstride = 0) {
  View5 vq = vd; vq.w = (vd.w + 4 / PX - 1) / (4 / PX);
  const unsigned chunk = pw_chunk(vq);
  const dim3 g = grid_chunked(vq, chunk);
  const FastDiv dvw = mk_div(vq.w), dh = mk_div(vd.h);
  if (bias)
    hipLaunchKernelGGL((pool_bwd_fixed_kernel<PZ, PY, PX, true>), g, dim3(256), 0, ctx->stream,
                       vd, vy, bias, act, vdy, dbias, accumulate, dvw, dh, chunk, gparts, gstride);
  else
    hipLaunchKernelGGL((pool_bwd_fixed_kernel<PZ, PY, PX, false>), g, dim3(256), 0, ctx->stream,
                       vd, vy, bias, act, vdy, dbias, accumulate, dvw, dh, chunk, gparts, gstride);
}

static int pool_shapes_ok(const e2_tensor5* big, const e2_tensor5* small, int pz, int py,
                          int px, const char* name) {
  E2_REQUIRE(pz >= 1 && py >= 1 && px >= 1, "%s: pool factors must be >= 1", name);
  E2_REQUIRE(big->n == small->n && big->c == small->c, "%s: n/c mismatch", name);
  E2_REQUIRE(big->d / pz == small->d && big->h / py == small->h && big->w / px == small->w,
             "%s: pooled shape mismatch: (%d,%d,%d)/(%d,%d,%d) != (%d,%d,%d)", name,
             big->d, big->h, big->w, pz, py, px, small->d, small->h, small->w);
  return 0;
}

static int pool_fwd_impl(e2_ctx* ctx, const e2_tensor5* y, const float* bias, int pz, int py,
                         int px, int act, const e2_tensor5* out, int nparts, int64_t pstride);
extern "C" int e2_pool_bias_act_fwd(e2_ctx* ctx, const e2_tensor5* y, const float* bias,
                                    int pz, int py, int px, int act,
                                    const e2_tensor5* out) {
  return pool_fwd_impl(ctx, y, bias, pz, py, px, act, out, 1, 0);
}
extern "C" int e2_pool_bias_act_fwd_parts(e2_ctx* ctx, const e2_tensor5* y, int64_t part_stride,
                                          int nparts, const float* bias, int pz, int py, int px,
                                          int act, const e2_tensor5* out) {
  E2_REQUIRE(nparts >= 1 && nparts <= kMaxParts && (nparts == 1 || part_stride > 0),
             "pool_bias_act_fwd_parts: bad parts (1 .. %d)", kMaxParts);
  return pool_fwd_impl(ctx, y, bias, pz, py, px, act, out, nparts, part_stride);
}
static int pool_fwd_impl(e2_ctx* ctx, const e2_tensor5* y, const float* bias, int pz, int py,
                         int px, int act, const e2_tensor5* out, int nparts, int64_t pstride) {
  E2_REQUIRE(ctx, "pool_bias_act_fwd: null ctx");
  if (int rc = check_view(y, "pool_bias_act_fwd y")) return rc;
  if (int rc = check_view(out, "pool_bias_act_fwd out")) return rc;
  if (int rc = pool_shapes_ok(y, out, pz, py, px, "pool_bias_act_fwd")) return rc;
  E2_REQUIRE(act == E2_ACT_LIN || act == E2_ACT_RELU, "pool_bias_act_fwd: bad act %d", act);
  View5 vy = mk(y), vo = mk(out);
  E2_REQUIRE((long)vo.d * vo.h * vo.w < (1L << 31), "pool_bias_act_fwd: channel too large");
  const FastDiv dw = mk_div(vo.w), dh = mk_div(vo.h);
  const unsigned chunk = pw_chunk(vo);
  const int pcode = pz * 100 + py * 10 + px;
  E2_REQUIRE(nparts == 1 || pcode == 122 || pcode == 211 || pcode == 222 || pcode == 111,
             "pool_bias_act_fwd_parts: partial sums are added up by the fixed-window kernels "
             "((1,1,1), (1,2,2), (2,1,1), (2,2,2)) only");
  if (pcode == 122) launch_pool_fwd_fixed<1, 2, 2>(ctx, vy, bias, act, vo, nparts, (long)pstride);
  else if (pcode == 211) launch_pool_fwd_fixed<2, 1, 1>(ctx, vy, bias, act, vo, nparts, (long)pstride);
  else if (pcode == 222) launch_pool_fwd_fixed<2, 2, 2>(ctx, vy, bias, act, vo, nparts, (long)pstride);
  else if (pcode == 111) launch_pool_fwd_fixed<1, 1, 1>(ctx, vy, bias, act, vo, nparts, (long)pstride);
  else if (bias)
    hipLaunchKernelGGL((pool_fwd_kernel<true>), grid_chunked(vo, chunk), dim3(256), 0,
                       ctx->stream, vy, bias, pz, py, px, act, vo, dw, dh, chunk);
  else
    hipLaunchKernelGGL((pool_fwd_kernel<false>), grid_chunked(vo, chunk), dim3(256), 0,
                       ctx->stream, vy, bias, pz, py, px, act, vo, dw, dh, chunk);
  E2_CHECK_HIP(hipGetLastError());
  return 0;
}

static int pool_bwd_common(e2_ctx* ctx, const e2_tensor5* dout, const e2_tensor5* y,
                           const float* bias, int pz, int py, int px, int act,
                           const e2_tensor5* dy, float* dbias, int accumulate,
                           int gparts = 1, int64_t gstride = 0) {
  if (int rc = check_view(dout, "pool_bwd dout")) return rc;
  if (int rc = check_view(y, "pool_bwd y")) return rc;
  if (int rc = check_view(dy, "pool_bwd dy")) return rc;
  if (int rc = pool_shapes_ok(y, dout, pz, py, px, "pool_bwd")) return rc;
  E2_REQUIRE(same_size(dy, y), "pool_bwd: dy/y shape mismatch");
  // floor semantics: rows/cols beyond the pooled extent receive no gradient
  if (!accumulate && (y->d % pz || y->h % py || y->w % px)) {
    if (int rc = e2i_fill_view(ctx, dy, 0.f)) return rc;
  }
  View5 vd = mk(dout), vy = mk(y), vdy = mk(dy);
  E2_REQUIRE((long)vd.d * vd.h * vd.w < (1L << 31), "pool_bwd: channel too large");
  const FastDiv dw = mk_div(vd.w), dh = mk_div(vd.h);
  const unsigned chunk = pw_chunk(vd);
  const int pcode = pz * 100 + py * 10 + px;
  E2_REQUIRE(gparts == 1 || pcode == 122 || pcode == 211 || pcode == 222 || pcode == 111,
             "pool_bias_act_bwd_parts: partial sums are added up by the fixed-window kernels only");
  if (pcode == 122)
    launch_pool_bwd_fixed<1, 2, 2>(ctx, vd, vy, bias, act, vdy, dbias, accumulate, gparts, (long)gstride);
  else if (pcode == 211)
    launch_pool_bwd_fixed<2, 1, 1>(ctx, vd, vy, bias, act, vdy, dbias, accumulate, gparts, (long)gstride);
  else if (pcode == 222)
    launch_pool_bwd_fixed<2, 2, 2>(ctx, vd, vy, bias, act, vdy, dbias, accumulate, gparts, (long)gstride);
  else if (pcode == 111)
    launch_pool_bwd_fixed<1, 1, 1>(ctx, vd, vy, bias, act, vdy, dbias, accumulate, gparts, (long)gstride);
  else if (bias)
    hipLaunchKernelGGL((pool_bwd_kernel<true>), grid_chunked(vd, chunk), dim3(256), 0,
                       ctx->stream, vd, vy, bias, pz, py, px, act, vdy, dbias, accumulate, dw,
                       dh, chunk);
  else
    hipLaunchKernelGGL((pool_bwd_kernel<false>), grid_chunked(vd, chunk), dim3(256), 0,
                       ctx->stream, vd, vy, bias, pz, py, px, act, vdy, dbias, accumulate, dw,
                       dh, chunk);
  E2_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" int e2_pool_bias_act_bwd(e2_ctx* ctx, const e2_tensor5* dout,
                                    const e2_tensor5* y, const float* bias, int pz, int py,
                                    int px, int act, const e2_tensor5* dy, float* dbias) {
  E2_REQUIRE(ctx, "pool_bias_act_bwd: null ctx");
  E2_REQUIRE(act == E2_ACT_LIN || act == E2_ACT_RELU, "pool_bias_act_bwd: bad act %d", act);
  return pool_bwd_common(ctx, dout, y, bias, pz, py, px, act, dy, dbias, 0);
}

extern "C" int e2_pool_bias_act_bwd_parts(e2_ctx* ctx, const e2_tensor5* dout,
                                          int64_t dout_part_stride, int dout_parts,
                                          const e2_tensor5* y, const float* bias, int pz, int py,
                                          int px, int act, const e2_tensor5* dy, float* dbias) {
  E2_REQUIRE(ctx, "pool_bias_act_bwd_parts: null ctx");
  E2_REQUIRE(act == E2_ACT_LIN || act == E2_ACT_RELU, "pool_bias_act_bwd_parts: bad act %d", act);
  E2_REQUIRE(dout_parts >= 1 && dout_parts <= kMaxParts && (dout_parts == 1 || dout_part_stride > 0),
             "pool_bias_act_bwd_parts: bad parts (1 .. %d)", kMaxParts);
  return pool_bwd_common(ctx, dout, y, bias, pz, py, px, act, dy, dbias, 0, dout_parts,
                         dout_part_stride);
}

static int act_bwd_out_impl(e2_ctx* ctx, const e2_tensor5* dout, const e2_tensor5* out, int act,
                            const e2_tensor5* dy, float* dbias, int gparts, int64_t gstride);
extern "C" int e2_bias_act_bwd_out(e2_ctx* ctx, const e2_tensor5* dout, const e2_tensor5* out,
                                   int act, const e2_tensor5* dy, float* dbias) {
  return act_bwd_out_impl(ctx, dout, out, act, dy, dbias, 1, 0);
}
extern "C" int e2_bias_act_bwd_out_parts(e2_ctx* ctx, const e2_tensor5* dout,
                                         int64_t dout_part_stride, int dout_parts,
                                         const e2_tensor5* out, int act, const e2_tensor5* dy,
                                         float* dbias) {
  E2_REQUIRE(dout_parts >= 1 && dout_parts <= kMaxParts && (dout_parts == 1 || dout_part_stride > 0),
             "bias_act_bwd_out_parts: bad parts (1 .. %d)", kMaxParts);
  return act_bwd_out_impl(ctx, dout, out, act, dy, dbias, dout_parts, dout_part_stride);
}
static int act_bwd_out_impl(e2_ctx* ctx, const e2_tensor5* dout, const e2_tensor5* out, int act,
                            const e2_tensor5* dy, float* dbias, int gparts, int64_t gstride) {
  E2_REQUIRE(ctx, "bias_act_bwd_out: null ctx");
  E2_REQUIRE(act == E2_ACT_LIN || act == E2_ACT_RELU, "bias_act_bwd_out: bad act %d", act);
  if (int rc = check_view(dout, "bias_act_bwd_out dout")) return rc;
  if (int rc = check_view(out, "bias_act_bwd_out out")) return rc;
  if (int rc = check_view(dy, "bias_act_bwd_out dy")) return rc;
  E2_REQUIRE(same_size(dout, out) && same_size(dy, out), "bias_act_bwd_out: shape mismatch");
  View5 vd = mk(dout), vo = mk(out), vdy = mk(dy);
  E2_REQUIRE((long)vd.d * vd.h * vd.w < (1L << 31), "bias_act_bwd_out: channel too large");
  View5 vq = vd; vq.w = (vd.w + 3) / 4;                 // the grid counts 4-element pieces
  const FastDiv dvw = mk_div(vq.w), dh = mk_div(vd.h);
  const unsigned chunk = pw_chunk(vq);
  hipLaunchKernelGGL(act_bwd_out_kernel, grid_chunked(vq, chunk), dim3(256), 0, ctx->stream, vd,
                     vo, act, vdy, dbias, dvw, dh, chunk, gparts, (long)gstride);
  E2_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" int e2_maxpool3d_fwd(e2_ctx* ctx, const e2_tensor5* x, int pz, int py, int px,
                                const e2_tensor5* out) {
  return e2_pool_bias_act_fwd(ctx, x, nullptr, pz, py, px, E2_ACT_LIN, out);
}

extern "C" int e2_maxpool3d_bwd(e2_ctx* ctx, const e2_tensor5* dout, const e2_tensor5* x,
                                int pz, int py, int px, const e2_tensor5* dx,
                                int accumulate) {
  E2_REQUIRE(ctx, "maxpool3d_bwd: null ctx");
  return pool_bwd_common(ctx, dout, x, nullptr, pz, py, px, E2_ACT_LIN, dx, nullptr,
                         accumulate);
}

int e2i_upconv_dpre_s2d(e2_ctx* ctx, const e2_tensor5* dout, const e2_tensor5* yout, int pz,
                        int py, int px, int act, float* s2d, float* dbias) {
  View5 vd = mk(dout), vy = mk(yout);
  E2_REQUIRE((long)vd.d * vd.h * vd.w < (1L << 31), "upconv_dpre_s2d: channel too large");
  const unsigned chunk = pw_chunk(vd);
  hipLaunchKernelGGL(upconv_dpre_s2d_kernel, grid_chunked(vd, chunk), dim3(256), 0,
                     ctx->stream, vd, vy, pz, py, px, act, s2d, dbias, mk_div(vd.w),
                     mk_div(vd.h), mk_div(pz), mk_div(py), mk_div(px), chunk);
  E2_CHECK_HIP(hipGetLastError());
  return 0;
}
