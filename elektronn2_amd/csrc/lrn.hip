// lrn.hip -- local response normalisation (e2_lrn_fwd / e2_lrn_bwd): the device side of the LRN
// node (neural.py:2043-2181 of the reference).
//
//   q = k + alpha * m          out = x * q^(-beta)
//   SPATIAL  m[n, c, p] = (1 / (fz fy fx)) * sum of x[n, c, p + o]^2 over the box o in [-f/2, f/2]
//            per axis; positions outside the tensor add 0, the divisor is the whole box (the
//            reference's 'same' conv of x^2 with an identity-over-features averaging filter, which
//            is never built here)
//   CHANNEL  m[n, c, p] = (1 / f) * sum over o in [-f/2, f/2] of x[n, clamp(c + o, 0, C - 1), p]^2
//            (the edge feature is replicated, neural.py:2152-2176)
//
// Backward, with t = dout * x * q^(-beta-1) and N the window size:
//
//   dx_i = dout_i * q_i^(-beta)  -  (2 alpha beta / N) * x_i * sum_j mult(i, j) * t_j
//
// SPATIAL: j over the same box around i, mult = 1, t = 0 outside.  CHANNEL: j over the features at
// the same (n, p), mult(i, j) = the number of o in [-f/2, f/2] with clamp(j + o, 0, C - 1) == i (the
// replicated edge makes it > 1 at features 0 and C - 1).  Two launches: a pointwise pass writes t
// into `tmp` (one powf per element, not one per window element), a GATHER over the window of t
// forms dx -- no atomics, the same bits every run.  Windows are walked in ascending (z, y, x) or
// feature order and added up in f32.
//
// alpha, k and beta are DEVICE scalars read when the kernels run: a captured launch follows later
// changes of their contents.
//
// Geometry of act.hip / pool.hip: a work-group stays inside one (n, c), a thread owns FOUR
// consecutive x of one row and moves them as one 16-byte access where that row piece is 16-byte
// aligned in the view at hand, element by element at row ends and on misaligned views.  The span
// of a source row a spatial window needs is walked in pieces cut where the SOURCE row is 16-byte
// aligned.  Spatial axes that are dense in every view are collapsed on the host where no window
// runs along them (always in the channel mode and the pointwise pass).  Nothing outside out / q /
// tmp / dx is written, nothing outside the views is read.  Pure streams: no LDS, no workspace.
#include "stream_common.hpp"

namespace {

// strides of one view after the host's collapse: batch, feature, outer row axis, inner row axis
struct LrnS {
  long n, c, r1, r0;
};

struct LrnP {
  const float* g;               // dout                         (bwd)
  const float* x;
  const float* q;               // k + alpha m as the forward kept it   (bwd)
  const float* t;               // tmp, read by the gather      (bwd, second launch)
  float* o;                     // fwd: out    bwd: tmp (first launch), dx (second launch)
  float* qo;                    // fwd: q, may be null
  LrnS sg, sx, sq, st, so;
  unsigned w, r0, r1, C;        // row length, extents of the two row axes, features
  unsigned quads;               // ceil(w / 4)
  unsigned items;               // r1 * r0 * quads  (< 2^31)
  unsigned chunk;               // items per work-group, a multiple of 256
  FastDiv dq, dr0;
  int h1, h0, hw;               // SPATIAL: half windows along r1, r0, w;  CHANNEL: h1 = half window
  const float* alpha;
  const float* k;
  const float* beta;
  float inv_n;                  // 1 / window size
  int accumulate;
};

typedef float lrn_f4 __attribute__((ext_vector_type(4)));

// nv <= 4 floats at p: one 16-byte load where that is whole and aligned; the rest reads as 0
__device__ __forceinline__ lrn_f4 ld4(const float* p, unsigned nv) {
  if (nv == 4u && (((uintptr_t)p) & 15) == 0) return *reinterpret_cast<const lrn_f4*>(p);
  lrn_f4 r = {0.f, 0.f, 0.f, 0.f};
  for (unsigned e = 0; e < nv; ++e) r[e] = p[e];
  return r;
}
__device__ __forceinline__ void st4(float* p, unsigned nv, lrn_f4 v) {
  if (nv == 4u && (((uintptr_t)p) & 15) == 0) {
    *reinterpret_cast<lrn_f4*>(p) = v;
    return;
  }
  for (unsigned e = 0; e < nv; ++e) p[e] = v[e];
}

// acc[e] = sum over the box around (i1, i0, x0 + e), cut to the tensor, of s (SQ: of s^2), for
// e < nv; sbase is the (n, c) block of the source
template <bool SQ>
__device__ __forceinline__ void box_sum(const LrnP& p, const float* sbase, const LrnS& ss,
                                        unsigned i1, unsigned i0, unsigned x0, unsigned nv,
                                        float acc[4]) {
  const int u0 = max((int)x0 - p.hw, 0), u1 = min((int)(x0 + nv) + p.hw, (int)p.w);
  const int a0 = max((int)i1 - p.h1, 0), a1 = min((int)i1 + p.h1, (int)p.r1 - 1);
  const int b0 = max((int)i0 - p.h0, 0), b1 = min((int)i0 + p.h0, (int)p.r0 - 1);
  const unsigned span = 2u * (unsigned)p.hw;
  for (int a = a0; a <= a1; ++a) {
    for (int b = b0; b <= b1; ++b) {
      const float* srow = sbase + (long)a * ss.r1 + (long)b * ss.r0;
      const int ms = (int)((((uintptr_t)srow) >> 2) & 3);
      for (int ua = u0 - ((ms + u0) & 3); ua < u1; ua += 4) {
        lrn_f4 r;
        if (ua >= 0 && ua + 4 <= (int)p.w) {
          r = *reinterpret_cast<const lrn_f4*>(srow + ua);
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int u = ua + j;
            r[j] = (u >= u0 && u < u1) ? srow[u] : 0.f;
          }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int u = ua + j;
          const float v = SQ ? r[j] * r[j] : r[j];
#pragma unroll
          for (int e = 0; e < 4; ++e)       // |u - (x0 + e)| <= hw
            if ((unsigned)(u - (int)x0 - e + p.hw) <= span) acc[e] += v;
        }
      }
    }
  }
}

// the row piece of item s: row axes (i1, i0), first column x0, nv elements
__device__ __forceinline__ void item_of(const LrnP& p, unsigned s, unsigned* i1, unsigned* i0,
                                        unsigned* x0, unsigned* nv) {
  const unsigned row = fdiv(s, p.dq);
  *x0 = (s - row * p.quads) << 2;
  *i1 = fdiv(row, p.dr0);
  *i0 = row - *i1 * p.r0;
  *nv = min(4u, p.w - *x0);
}
__device__ __forceinline__ long at(const LrnS& s, unsigned n, unsigned c, unsigned i1, unsigned i0,
                                   unsigned x0) {
  return (long)n * s.n + (long)c * s.c + (long)i1 * s.r1 + (long)i0 * s.r0 + x0;
}

// (the kernels below keep the strides of up to five views in scalar registers: 7 waves per SIMD
// where that takes more than 96 of them -- pinning 8 spills them into vector lanes)
// the number of o in [-h, h] with clamp(j + o, 0, C1) == i, for |i - j| <= h: o == i - j, and every
// o below it at feature 0, every o above it at feature C1
__device__ __forceinline__ float lrn_mult(int i, int j, int h, int C1) {
  const int olo = i == 0 ? -h : i - j;
  const int ohi = i == C1 ? h : i - j;
  return (float)(ohi - olo + 1);
}

template <int MODE>
__global__ __launch_bounds__(256) void e2lrn_fwd_kernel(LrnP p) {
  const unsigned s0 = blockIdx.x * p.chunk;
  const unsigned s1 = min(s0 + p.chunk, p.items);
  const unsigned c = blockIdx.y, n = blockIdx.z;
  const float alpha = e2_uniform_ld(p.alpha, 0), kk = e2_uniform_ld(p.k, 0);
  const float nbeta = -e2_uniform_ld(p.beta, 0);
  for (unsigned s = s0 + threadIdx.x; s < s1; s += 256) {
    unsigned i1, i0, x0, nv;
    item_of(p, s, &i1, &i0, &x0, &nv);
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    if (MODE == E2_LRN_SPATIAL) {
      box_sum<true>(p, p.x + (long)n * p.sx.n + (long)c * p.sx.c, p.sx, i1, i0, x0, nv, acc);
    } else {
      // feature j is met by lrn_mult(j, c) of the offsets (more than one at the replicated edges)
      const int C1 = (int)p.C - 1, i = (int)c, h = p.h1;
      for (int j = max(i - h, 0); j <= min(i + h, C1); ++j) {
        const float mult = lrn_mult(j, i, h, C1);
        const lrn_f4 v = ld4(p.x + at(p.sx, n, (unsigned)j, i1, i0, x0), nv);
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[e] += mult * (v[e] * v[e]);
      }
    }
    const lrn_f4 xc = ld4(p.x + at(p.sx, n, c, i1, i0, x0), nv);
    lrn_f4 qv, r;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      qv[e] = kk + alpha * (acc[e] * p.inv_n);
      r[e] = xc[e] * powf(qv[e], nbeta);
    }
    st4(p.o + at(p.so, n, c, i1, i0, x0), nv, r);
    if (p.qo != nullptr) st4(p.qo + at(p.sq, n, c, i1, i0, x0), nv, qv);
  }
}

// t = dout * x * q^(-beta-1)
__global__ __launch_bounds__(256) void e2lrn_bwd_t_kernel(LrnP p) {
  const unsigned s0 = blockIdx.x * p.chunk;
  const unsigned s1 = min(s0 + p.chunk, p.items);
  const unsigned c = blockIdx.y, n = blockIdx.z;
  const float e1 = -e2_uniform_ld(p.beta, 0) - 1.f;
  for (unsigned s = s0 + threadIdx.x; s < s1; s += 256) {
    unsigned i1, i0, x0, nv;
    item_of(p, s, &i1, &i0, &x0, &nv);
    const lrn_f4 g = ld4(p.g + at(p.sg, n, c, i1, i0, x0), nv);
    const lrn_f4 xc = ld4(p.x + at(p.sx, n, c, i1, i0, x0), nv);
    lrn_f4 q = ld4(p.q + at(p.sq, n, c, i1, i0, x0), nv);
    lrn_f4 r;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if ((unsigned)e >= nv) q[e] = 1.f;
      r[e] = g[e] * xc[e] * powf(q[e], e1);
    }
    st4(p.o + at(p.so, n, c, i1, i0, x0), nv, r);
  }
}

// dx (+)= dout * q^(-beta) - (2 alpha beta / N) * x * (sum of mult * t over the window)
template <int MODE>
__global__ __launch_bounds__(256) void e2lrn_bwd_dx_kernel(LrnP p) {
  const unsigned s0 = blockIdx.x * p.chunk;
  const unsigned s1 = min(s0 + p.chunk, p.items);
  const unsigned c = blockIdx.y, n = blockIdx.z;
  const float beta = e2_uniform_ld(p.beta, 0);
  const float coef = 2.f * e2_uniform_ld(p.alpha, 0) * beta * p.inv_n;
  for (unsigned s = s0 + threadIdx.x; s < s1; s += 256) {
    unsigned i1, i0, x0, nv;
    item_of(p, s, &i1, &i0, &x0, &nv);
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    if (MODE == E2_LRN_SPATIAL) {
      box_sum<false>(p, p.t + (long)n * p.st.n + (long)c * p.st.c, p.st, i1, i0, x0, nv, acc);
    } else {
      const int C1 = (int)p.C - 1, i = (int)c, h = p.h1;
      for (int j = max(i - h, 0); j <= min(i + h, C1); ++j) {
        const float mult = lrn_mult(i, j, h, C1);
        const lrn_f4 v = ld4(p.t + at(p.st, n, (unsigned)j, i1, i0, x0), nv);
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[e] += mult * v[e];
      }
    }
    // (read behind the gather: fewer values live across its loops)
    const lrn_f4 g = ld4(p.g + at(p.sg, n, c, i1, i0, x0), nv);
    const lrn_f4 xc = ld4(p.x + at(p.sx, n, c, i1, i0, x0), nv);
    lrn_f4 q = ld4(p.q + at(p.sq, n, c, i1, i0, x0), nv);
    float* dst = p.o + at(p.so, n, c, i1, i0, x0);
    lrn_f4 r;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if ((unsigned)e >= nv) q[e] = 1.f;
      r[e] = g[e] * powf(q[e], -beta) - coef * xc[e] * acc[e];
    }
    if (p.accumulate) {
      const lrn_f4 old = ld4(dst, nv);
#pragma unroll
      for (int e = 0; e < 4; ++e) r[e] = old[e] + r[e];
    }
    st4(dst, nv, r);
  }
}

// What the launches of one entry point share.  v: the views (nv of them, identical sizes),
// f: the window along (d, h, w) -- (1, 1, 1) where nothing is windowed in space.  Collapses the
// spatial axes that are dense in every view and carry no window, fills the extents of p and the
// strides s[k] of view k.
int lrn_geometry(e2_ctx* ctx, const e2_tensor5* const* v, int nv, LrnS* s, const int* f, LrnP& p,
                 dim3& grid, const char* who) {
  const e2_tensor5* t = v[0];
  unsigned long long w = (unsigned long long)t->w, r0 = (unsigned long long)t->h,
                     r1 = (unsigned long long)t->d;
  E2_REQUIRE(r1 * r0 * w < (1ull << 31), "%s: a channel of (%d,%d,%d,%d,%d) holds 2^31 elements or more",
             who, t->n, t->c, t->d, t->h, t->w);
  // (32-bit index math: extent + half window stays below 2^31)
  E2_REQUIRE(t->d < (1 << 28) && t->h < (1 << 28) && t->w < (1 << 28), "%s: feature map too large", who);
  // a window reaches no further than the axis: beyond 2 * extent - 1 it holds the same elements
  // (along an axis of extent 1 nothing but the element itself)
  int f1 = (int)min((unsigned long long)f[0], 2 * r1 - 1), f0 = (int)min((unsigned long long)f[1], 2 * r0 - 1),
      fw = (int)min((unsigned long long)f[2], 2 * w - 1);
  for (int k = 0; k < nv; ++k) {
    s[k].n = (long)v[k]->sn; s[k].c = (long)v[k]->sc; s[k].r1 = (long)v[k]->sd; s[k].r0 = (long)v[k]->sh;
  }
  // the inner row axis joins w where there is one row, or the rows follow each other without a
  // gap in every view and no window runs along either axis; then the outer one likewise
  for (int pass = 0; pass < 2; ++pass) {
    bool join = r0 == 1 || (f0 == 1 && fw == 1);
    for (int k = 0; k < nv; ++k) join = join && (r0 == 1 || s[k].r0 == (long)w);
    if (!join) break;
    w *= r0; r0 = r1; r1 = 1;
    f0 = f1; f1 = 1;
    for (int k = 0; k < nv; ++k) { s[k].r0 = s[k].r1; s[k].r1 = 0; }
  }
  const unsigned long long quads = (w + 3) / 4, items = r1 * r0 * quads;
  p.w = (unsigned)w; p.r0 = (unsigned)r0; p.r1 = (unsigned)r1; p.C = (unsigned)t->c;
  p.quads = (unsigned)quads; p.items = (unsigned)items;
  p.dq = mk_div(p.quads); p.dr0 = mk_div(p.r0);
  p.h1 = f1 / 2; p.h0 = f0 / 2; p.hw = fw / 2;
  p.chunk = stream_chunk(ctx, (unsigned long long)t->n * t->c, items, 8, 8);
  grid = dim3((unsigned)((items + p.chunk - 1) / p.chunk), (unsigned)t->c, (unsigned)t->n);
  return 0;
}

int lrn_window_ok(const char* who, int mode, int fz, int fy, int fx) {
  E2_REQUIRE(mode == E2_LRN_SPATIAL || mode == E2_LRN_CHANNEL,
             "%s: unknown mode %d (0 spatial, 1 channel)", who, mode);
  E2_REQUIRE(fz >= 1 && fy >= 1 && fx >= 1 && (fz & 1) && (fy & 1) && (fx & 1),
             "%s: window %d,%d,%d: every extent must be odd and >= 1", who, fz, fy, fx);
  E2_REQUIRE(mode == E2_LRN_SPATIAL || (fy == 1 && fx == 1),
             "%s: the channel mode takes its window in fz (fy = fx = 1), not %d,%d,%d", who, fz, fy, fx);
  return 0;
}

}  // namespace

extern "C" int e2_lrn_fwd(e2_ctx* ctx, const e2_tensor5* x, int mode, int fz, int fy, int fx,
                          const float* alpha, const float* k, const float* beta,
                          const e2_tensor5* q, const e2_tensor5* out) {
  const char* who = "e2_lrn_fwd";
  E2_REQUIRE(ctx, "%s: null ctx", who);
  E2_REQUIRE(alpha && k && beta, "%s: null alpha / k / beta", who);
  if (int rc = check_view(x, "e2_lrn_fwd x")) return rc;
  if (int rc = check_view(out, "e2_lrn_fwd out")) return rc;
  if (q != nullptr) {
    if (int rc = check_view(q, "e2_lrn_fwd q")) return rc;
  }
  E2_REQUIRE(same_size(x, out) && (q == nullptr || same_size(x, q)), "%s: size mismatch", who);
  if (int rc = lrn_window_ok(who, mode, fz, fy, fx)) return rc;
  // (other threads read the neighbours of an element after its owner has written it)
  E2_REQUIRE(out->ptr != x->ptr, "%s: out may not alias x", who);
  E2_REQUIRE(q == nullptr || (q->ptr != x->ptr && q->ptr != out->ptr),
             "%s: q may not alias x or out", who);
  LrnP p = LrnP{};
  dim3 grid;
  const e2_tensor5* v[3] = {x, out, q};
  LrnS s[3];
  const int fs[3] = {fz, fy, fx}, f1[3] = {1, 1, 1};
  if (int rc = lrn_geometry(ctx, v, q ? 3 : 2, s, mode == E2_LRN_SPATIAL ? fs : f1, p, grid, who))
    return rc;
  p.x = x->ptr; p.o = out->ptr; p.qo = q ? q->ptr : nullptr;
  p.sx = s[0]; p.so = s[1]; p.sq = q ? s[2] : LrnS{};
  p.alpha = alpha; p.k = k; p.beta = beta;
  if (mode == E2_LRN_SPATIAL) {
    p.inv_n = (float)(1.0 / ((double)fz * fy * fx));
    hipLaunchKernelGGL((e2lrn_fwd_kernel<E2_LRN_SPATIAL>), grid, dim3(256), 0, ctx->stream, p);
  } else {
    p.h1 = fz / 2;
    p.inv_n = 1.0f / (float)fz;
    hipLaunchKernelGGL((e2lrn_fwd_kernel<E2_LRN_CHANNEL>), grid, dim3(256), 0, ctx->stream, p);
  }
  E2_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" int e2_lrn_bwd(e2_ctx* ctx, const e2_tensor5* dout, const e2_tensor5* x,
                          const e2_tensor5* q, int mode, int fz, int fy, int fx,
                          const float* alpha, const float* beta, const e2_tensor5* tmp,
                          const e2_tensor5* dx, int accumulate) {
  const char* who = "e2_lrn_bwd";
  E2_REQUIRE(ctx, "%s: null ctx", who);
  E2_REQUIRE(alpha && beta, "%s: null alpha / beta", who);
  if (int rc = check_view(dout, "e2_lrn_bwd dout")) return rc;
  if (int rc = check_view(x, "e2_lrn_bwd x")) return rc;
  if (int rc = check_view(q, "e2_lrn_bwd q")) return rc;
  if (int rc = check_view(tmp, "e2_lrn_bwd tmp")) return rc;
  if (int rc = check_view(dx, "e2_lrn_bwd dx")) return rc;
  E2_REQUIRE(same_size(dout, x) && same_size(dout, q) && same_size(dout, tmp) && same_size(dout, dx),
             "%s: size mismatch", who);
  if (int rc = lrn_window_ok(who, mode, fz, fy, fx)) return rc;
  // (the gather reads neighbours)
  E2_REQUIRE(dx->ptr != dout->ptr, "%s: dx may not alias dout", who);
  E2_REQUIRE(tmp->ptr != dout->ptr && tmp->ptr != x->ptr && tmp->ptr != q->ptr && tmp->ptr != dx->ptr,
             "%s: tmp may not alias dout, x, q or dx", who);
  const e2_tensor5* v[5] = {dout, x, q, tmp, dx};
  LrnS s[5];
  const int fs[3] = {fz, fy, fx}, f1[3] = {1, 1, 1};
  // ---- t = dout * x * q^(-beta-1), pointwise
  {
    LrnP p = LrnP{};
    dim3 grid;
    if (int rc = lrn_geometry(ctx, v, 4, s, f1, p, grid, who)) return rc;
    p.g = dout->ptr; p.x = x->ptr; p.q = q->ptr; p.o = tmp->ptr;
    p.sg = s[0]; p.sx = s[1]; p.sq = s[2]; p.so = s[3];
    p.beta = beta;
    hipLaunchKernelGGL(e2lrn_bwd_t_kernel, grid, dim3(256), 0, ctx->stream, p);
    E2_CHECK_HIP(hipGetLastError());
  }
  // ---- the gather over the window of t
  LrnP p = LrnP{};
  dim3 grid;
  if (int rc = lrn_geometry(ctx, v, 5, s, mode == E2_LRN_SPATIAL ? fs : f1, p, grid, who)) return rc;
  p.g = dout->ptr; p.x = x->ptr; p.q = q->ptr; p.t = tmp->ptr; p.o = dx->ptr;
  p.sg = s[0]; p.sx = s[1]; p.sq = s[2]; p.st = s[3]; p.so = s[4];
  p.alpha = alpha; p.beta = beta;
  p.accumulate = accumulate ? 1 : 0;
  if (mode == E2_LRN_SPATIAL) {
    p.inv_n = (float)(1.0 / ((double)fz * fy * fx));
    hipLaunchKernelGGL((e2lrn_bwd_dx_kernel<E2_LRN_SPATIAL>), grid, dim3(256), 0, ctx->stream, p);
  } else {
    p.h1 = fz / 2;
    p.inv_n = 1.0f / (float)fz;
    hipLaunchKernelGGL((e2lrn_bwd_dx_kernel<E2_LRN_CHANNEL>), grid, dim3(256), 0, ctx->stream, p);
  }
  E2_CHECK_HIP(hipGetLastError());
  return 0;
}
