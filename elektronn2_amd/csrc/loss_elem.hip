// loss_elem.hip -- element-wise losses on strided 5-D views and their mix (e2_loss_fwd /
// e2_loss_mix / e2_loss_bwd; loss.py:829-887 GaussianNLL, 953-1011 BinaryNLL, 1014-1101
// SquaredLoss, 1215-1276 AbsLoss, 1346-1363 AggregateLoss).
//
//   p prediction, t target, d = t - p, EPS = 1e-5, masked = |t + 666| <= 1e-8 + 666e-5 (T.isclose
//   with Theano's defaults; NaN is not masked), n_lab = unmasked elements, n_tot = all elements
//
//   kind        element loss l (unmasked)                                  term value L
//   SQUARED     0.5 d^2 g c   g = [|d| >= margin]  c = sc / (|t| + sc)     S1/(n_lab+1) - margin S2/n_tot
//   ABS         |d| g c                            c = sc |t| + 1          (S1 = sum l, S2 = sum c; the
//                                                                           second part only with a margin)
//   BINARY_NLL  -xlogy0(t, p+EPS) - xlogy0(1-t, 1-p+EPS)  [- xlogy0(t, t+EPS) - xlogy0(1-t, 1-t+EPS)]
//                                                                          S1/(n_lab+1)
//   GAUSS_NLL   0.5 log(2 pi) + log s + 0.5 ((t - mu) / s)^2, no mask      S1/n_tot
//
// The element-wise array of the reference is never written.  The forward kernel leaves ONE row
// (S1, n_lab, S2, 0) per work-group in a slab -- a plain 16-byte store, no atomics: the whole grid
// has one destination, and atomics of many work-groups on one address serialise (act.hip, the note
// at e2_act_bwd).  The mix kernel (one work-group) sums the slabs of all terms in a fixed order in
// double, so the loss is bit-reproducible and the slab needs no zero fill; it writes every
// term's value, its labelled count, the gradient coefficient coef[k] = w_k / (K (n_lab_k + 1))
// (GAUSS: w_k / (K n_tot)) and the total (1/K) sum_k w_k L_k.  The backward kernel reads its
// coefficient, margin and scale_correction from device memory when it runs.
//
// BetaNLL (loss.py:890-950) runs through the same kernel templates under an internal kind with
// entry points of its own (e2_beta_nll_fwd / e2_beta_nll_bwd, at the end of this file): the public
// enum, e2_loss_term and e2_loss_mix do not change; in the mix it is a GAUSS_NLL-kind row.
//
// Geometry as in act.hip: a thread owns FOUR consecutive x of one row and moves them as one
// 16-byte access where that piece is 16-byte aligned in every view, element by element at row ends
// and on misaligned views; axes that are dense in all views are collapsed on the host (here also
// the feature and batch axes: there is no bias, a work-group need not stay inside one (n, c)).
// Nothing outside a view is read or written.  Kind and options are template parameters.
#include "stream_common.hpp"

namespace {

#define E2_LOSS_EPS 1e-5f
#define E2_LOSS_MASK_TOL (1e-8f + 666e-5f)
#define E2_HALF_LOG_2PI 0.91893853320467274178f

// BetaNLL runs through the same kernel templates under a kind of its own that is NOT part of the
// public enum: e2_loss_term, e2_loss_fwd / e2_loss_bwd and e2_loss_mix do not know it (the mix
// gets a GAUSS_NLL-kind descriptor for it: the same plain mean over n_tot)
#define E2I_LOSS_BETA_NLL 4
// kinds with a second prediction view (GAUSS: sigma, BETA: the concentration)
#define E2I_TWO_PRED(KIND) ((KIND) == E2_LOSS_GAUSS_NLL || (KIND) == E2I_LOSS_BETA_NLL)

typedef float loss_f4 __attribute__((ext_vector_type(4)));

// strides of the (up to) four axes that stay outside the collapsed row, innermost first
struct LView {
  long s[4];
};

struct LossP {
  const float* pred;            // prediction (GAUSS: mu)
  const float* sig;             // GAUSS only
  const float* tgt;
  float* dpred;                 // bwd outputs; either may be null
  float* dsig;
  LView vp, vs, vt, vdp, vds;
  unsigned w;                   // row length after the collapse
  unsigned quads;               // ceil(w / 4)
  unsigned items;               // rows * quads  (< 2^31)
  unsigned e0, e1, e2;          // extents of the three inner outside axes
  FastDiv dq, d0, d1, d2;
  const float* margin;          // device scalars, read when the kernel runs
  const float* sc;
  const float* coef;
  float* partials;              // fwd: [gridDim.x][4]
};

struct Pos {
  unsigned i0, i1, i2, i3, x0;
};
__device__ __forceinline__ Pos locate(const LossP& p, unsigned s) {
  Pos q;
  const unsigned row = fdiv(s, p.dq);
  q.x0 = (s - row * p.quads) << 2;
  const unsigned r1 = fdiv(row, p.d0);
  q.i0 = row - r1 * p.e0;
  const unsigned r2 = fdiv(r1, p.d1);
  q.i1 = r1 - r2 * p.e1;
  q.i3 = fdiv(r2, p.d2);
  q.i2 = r2 - q.i3 * p.e2;
  return q;
}
__device__ __forceinline__ long voff(const LView& v, const Pos& q) {
  return (long)q.i0 * v.s[0] + (long)q.i1 * v.s[1] + (long)q.i2 * v.s[2] + (long)q.i3 * v.s[3] +
         (long)q.x0;
}

__device__ __forceinline__ bool masked(float t) { return fabsf(t + 666.0f) <= E2_LOSS_MASK_TOL; }
__device__ __forceinline__ float xlogy0(float x, float y) { return x == 0.f ? 0.f : x * logf(y); }

// psi(x) = d/dx log Gamma(x) in f32, which the device math library does not have: the recurrence
// psi(x) = psi(x + 1) - 1/x up to an argument of at least 6 (five steps from the domain's x > 1; the
// loop is bounded, so no argument can hold a thread), then the asymptotic series, whose first
// dropped term is 1 / (132 x^10) < 1.3e-10 there
__device__ __forceinline__ float digammaf(float x) {
  float r = 0.f;
  for (int i = 0; i < 6 && x < 6.f; ++i) {
    r -= 1.f / x;
    x += 1.f;
  }
  const float i1 = 1.f / x, i2 = i1 * i1;
  const float ser = i2 * (1.f / 12.f - i2 * (1.f / 120.f - i2 * (1.f / 252.f - i2 * (1.f / 240.f))));
  return r + (logf(x) - 0.5f * i1 - ser);
}

// BetaNLL (loss.py:936-950): m mode, c concentration, x target, a = m (c - 2) + 1,
// b = (1 - m)(c - 2) + 1:
//   l = -[lgamma(a + b) - lgamma(a) - lgamma(b) + (a - 1) log(x + EPS) + (b - 1) log(1 - x + EPS)]
//       + softplus(-c)
// Domain c > 2, 0 < m < 1 (a, b > 1).  Outside it the formula is followed as far as lgammaf goes;
// nothing is guarded.
__device__ __forceinline__ float beta_nll(float m, float c, float x) {
  const float a = m * (c - 2.f) + 1.f, b = (1.f - m) * (c - 2.f) + 1.f;
  const float lx = logf(x + E2_LOSS_EPS), l1x = logf(1.f - x + E2_LOSS_EPS);
  const float p = lgammaf(a + b) - lgammaf(a) - lgammaf(b) + (a - 1.f) * lx + (b - 1.f) * l1x;
  return -p + log1pf(expf(-c));
}
//   dl/dm = (c - 2) [psi(a) - psi(b) - log(x + EPS) + log(1 - x + EPS)]
//   dl/dc = -psi(a + b) + m psi(a) + (1 - m) psi(b) - m log(x + EPS) - (1 - m) log(1 - x + EPS)
//           - sigmoid(-c)
__device__ __forceinline__ void beta_grad(float m, float c, float x, float& gm, float& gc) {
  const float a = m * (c - 2.f) + 1.f, b = (1.f - m) * (c - 2.f) + 1.f;
  const float lx = logf(x + E2_LOSS_EPS), l1x = logf(1.f - x + E2_LOSS_EPS);
  const float pa = digammaf(a), pb = digammaf(b);
  gm = (c - 2.f) * ((pa - pb) - lx + l1x);
  gc = -digammaf(a + b) + m * (pa - lx) + (1.f - m) * (pb - l1x) - 1.f / (1.f + expf(c));
}

// one element of the forward sums.  FLAG: subtract_label_entropy (BINARY), sig_is_log (GAUSS)
template <int KIND, bool MARGIN, bool SC, bool FLAG>
__device__ __forceinline__ void fwd_elem(float pv, float sv, float tv, float m, float sc, float& s1,
                                         float& nl, float& s2) {
  if (KIND == E2I_LOSS_BETA_NLL) {
    s1 += beta_nll(pv, sv, tv);
    nl += 1.f;
    return;
  }
  if (KIND == E2_LOSS_GAUSS_NLL) {
    const float s = FLAG ? expf(sv) : sv;
    const float ls = FLAG ? sv : logf(sv);
    const float z = (tv - pv) / s;
    s1 += E2_HALF_LOG_2PI + ls + 0.5f * (z * z);
    nl += 1.f;
    return;
  }
  if (masked(tv)) return;
  nl += 1.f;
  if (KIND == E2_LOSS_BINARY_NLL) {
    float l = -xlogy0(tv, pv + E2_LOSS_EPS) - xlogy0(1.f - tv, 1.f - pv + E2_LOSS_EPS);
    if (FLAG) l += -xlogy0(tv, tv + E2_LOSS_EPS) - xlogy0(1.f - tv, 1.f - tv + E2_LOSS_EPS);
    s1 += l;
    return;
  }
  const float d = tv - pv, ad = fabsf(d);
  float c = 1.f;
  if (SC) c = KIND == E2_LOSS_SQUARED ? sc / (fabsf(tv) + sc) : sc * fabsf(tv) + 1.f;
  float l = KIND == E2_LOSS_SQUARED ? 0.5f * (d * d) : ad;
  if (MARGIN) {
    l = ad >= m ? l : 0.f;
    s2 += c;
  }
  s1 += l * c;
}

template <int KIND, bool MARGIN, bool SC, bool FLAG>
__global__ __launch_bounds__(256) void e2loss_fwd_kernel(LossP p) {
  __shared__ float red[4][3];
  const float m = MARGIN ? e2_uniform_ld(p.margin, 0) : 0.f;
  const float sc = SC ? e2_uniform_ld(p.sc, 0) : 0.f;
  float s1 = 0.f, nl = 0.f, s2 = 0.f;
  const unsigned step = gridDim.x * 256u;
  for (unsigned s = blockIdx.x * 256u + threadIdx.x; s < p.items; s += step) {
    const Pos q = locate(p, s);
    const float* pp = p.pred + voff(p.vp, q);
    const float* tp = p.tgt + voff(p.vt, q);
    const float* sp = E2I_TWO_PRED(KIND) ? p.sig + voff(p.vs, q) : pp;
    if (q.x0 + 4u <= p.w && ((((uintptr_t)pp) | ((uintptr_t)tp) | ((uintptr_t)sp)) & 15) == 0) {
      const loss_f4 pv = *reinterpret_cast<const loss_f4*>(pp);
      const loss_f4 tv = *reinterpret_cast<const loss_f4*>(tp);
      loss_f4 sv = pv;
      if (E2I_TWO_PRED(KIND)) sv = *reinterpret_cast<const loss_f4*>(sp);
      fwd_elem<KIND, MARGIN, SC, FLAG>(pv[0], sv[0], tv[0], m, sc, s1, nl, s2);
      fwd_elem<KIND, MARGIN, SC, FLAG>(pv[1], sv[1], tv[1], m, sc, s1, nl, s2);
      fwd_elem<KIND, MARGIN, SC, FLAG>(pv[2], sv[2], tv[2], m, sc, s1, nl, s2);
      fwd_elem<KIND, MARGIN, SC, FLAG>(pv[3], sv[3], tv[3], m, sc, s1, nl, s2);
    } else {
      const unsigned nv = min(4u, p.w - q.x0);
      for (unsigned e = 0; e < nv; ++e)
        fwd_elem<KIND, MARGIN, SC, FLAG>(pp[e], sp[e], tp[e], m, sc, s1, nl, s2);
    }
  }
  s1 = wave_sum(s1);
  nl = wave_sum(nl);
  s2 = wave_sum(s2);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) { red[wave][0] = s1; red[wave][1] = nl; red[wave][2] = s2; }
  __syncthreads();
  if (threadIdx.x == 0) {
    loss_f4 r;
    r[0] = (red[0][0] + red[1][0]) + (red[2][0] + red[3][0]);
    r[1] = (red[0][1] + red[1][1]) + (red[2][1] + red[3][1]);
    r[2] = (red[0][2] + red[1][2]) + (red[2][2] + red[3][2]);
    r[3] = 0.f;
    *reinterpret_cast<loss_f4*>(p.partials + 4l * blockIdx.x) = r;
  }
}

// d(term)/d(pred) (and /d(sig)) of one element, times the coefficient
template <int KIND, bool MARGIN, bool SC, bool FLAG>
__device__ __forceinline__ void bwd_elem(float pv, float sv, float tv, float m, float sc, float co,
                                         float& gp, float& gs) {
  gs = 0.f;
  if (KIND == E2I_LOSS_BETA_NLL) {
    beta_grad(pv, sv, tv, gp, gs);
    gp *= co;
    gs *= co;
    return;
  }
  if (KIND == E2_LOSS_GAUSS_NLL) {
    const float s = FLAG ? expf(sv) : sv;
    const float z = (tv - pv) / s;
    gp = -(z / s) * co;
    gs = FLAG ? (1.f - z * z) * co : ((1.f - z * z) / s) * co;
    return;
  }
  gp = 0.f;
  if (masked(tv)) return;
  if (KIND == E2_LOSS_BINARY_NLL) {
    const float u = 1.f - tv;
    const float a = tv == 0.f ? 0.f : tv / (pv + E2_LOSS_EPS);
    const float b = u == 0.f ? 0.f : u / (1.f - pv + E2_LOSS_EPS);
    gp = (b - a) * co;
    return;
  }
  const float d = tv - pv, ad = fabsf(d);
  float c = 1.f;
  if (SC) c = KIND == E2_LOSS_SQUARED ? sc / (fabsf(tv) + sc) : sc * fabsf(tv) + 1.f;
  float g = KIND == E2_LOSS_SQUARED ? -d : (d > 0.f ? -1.f : (d < 0.f ? 1.f : 0.f));
  if (MARGIN) g = ad >= m ? g : 0.f;
  gp = (g * c) * co;
}

template <int KIND, bool MARGIN, bool SC, bool FLAG, bool ACC>
__global__ __launch_bounds__(256) void e2loss_bwd_kernel(LossP p) {
  const float m = MARGIN ? e2_uniform_ld(p.margin, 0) : 0.f;
  const float sc = SC ? e2_uniform_ld(p.sc, 0) : 0.f;
  const float co = e2_uniform_ld(p.coef, 0);
  const bool wp = p.dpred != nullptr, ws = E2I_TWO_PRED(KIND) && p.dsig != nullptr;
  const unsigned step = gridDim.x * 256u;
  for (unsigned s = blockIdx.x * 256u + threadIdx.x; s < p.items; s += step) {
    const Pos q = locate(p, s);
    const float* pp = p.pred + voff(p.vp, q);
    const float* tp = p.tgt + voff(p.vt, q);
    const float* sp = E2I_TWO_PRED(KIND) ? p.sig + voff(p.vs, q) : pp;
    float* dp = wp ? p.dpred + voff(p.vdp, q) : nullptr;
    float* ds = ws ? p.dsig + voff(p.vds, q) : nullptr;
    const uintptr_t al = ((uintptr_t)pp) | ((uintptr_t)tp) | ((uintptr_t)sp) | ((uintptr_t)dp) |
                         ((uintptr_t)ds);
    if (q.x0 + 4u <= p.w && (al & 15) == 0) {
      const loss_f4 pv = *reinterpret_cast<const loss_f4*>(pp);
      const loss_f4 tv = *reinterpret_cast<const loss_f4*>(tp);
      loss_f4 sv = pv;
      if (E2I_TWO_PRED(KIND)) sv = *reinterpret_cast<const loss_f4*>(sp);
      float p0, p1, p2, p3, g0, g1, g2, g3;
      bwd_elem<KIND, MARGIN, SC, FLAG>(pv[0], sv[0], tv[0], m, sc, co, p0, g0);
      bwd_elem<KIND, MARGIN, SC, FLAG>(pv[1], sv[1], tv[1], m, sc, co, p1, g1);
      bwd_elem<KIND, MARGIN, SC, FLAG>(pv[2], sv[2], tv[2], m, sc, co, p2, g2);
      bwd_elem<KIND, MARGIN, SC, FLAG>(pv[3], sv[3], tv[3], m, sc, co, p3, g3);
      loss_f4 gp, gs;
      gp[0] = p0; gp[1] = p1; gp[2] = p2; gp[3] = p3;
      gs[0] = g0; gs[1] = g1; gs[2] = g2; gs[3] = g3;
      if (wp) {
        if (ACC) gp += *reinterpret_cast<const loss_f4*>(dp);
        *reinterpret_cast<loss_f4*>(dp) = gp;
      }
      if (ws) {
        if (ACC) gs += *reinterpret_cast<const loss_f4*>(ds);
        *reinterpret_cast<loss_f4*>(ds) = gs;
      }
    } else {
      const unsigned nv = min(4u, p.w - q.x0);
      for (unsigned e = 0; e < nv; ++e) {
        float gp, gs;
        bwd_elem<KIND, MARGIN, SC, FLAG>(pp[e], sp[e], tp[e], m, sc, co, gp, gs);
        if (wp) dp[e] = ACC ? dp[e] + gp : gp;
        if (ws) ds[e] = ACC ? ds[e] + gs : gs;
      }
    }
  }
}

struct MixTerm {
  const float* partials;        // [rows][4]
  const float* margin;          // device scalar or null
  unsigned rows;
  int kind;
  double n_tot;
};
struct MixP {
  int k;
  MixTerm t[E2_MAX_LOSS_TERMS];
  const float* mix;             // [k] device
  float* coef;
  float* term_loss;
  float* count;
  float* loss_out;
};

// one work-group: per term, every thread sums its rows (r = tid, tid + 256, ...) in double, a
// fixed tree through LDS joins them -- the same order in every run
__global__ __launch_bounds__(256) void e2loss_mix_kernel(MixP p) {
  __shared__ double red[3][256];
  const unsigned tid = threadIdx.x;
  double total = 0.0;
#pragma unroll
  for (int k = 0; k < E2_MAX_LOSS_TERMS; ++k) {
    if (k < p.k) {
      const MixTerm t = p.t[k];
      double a = 0.0, b = 0.0, c = 0.0;
      for (unsigned r = tid; r < t.rows; r += 256u) {
        const loss_f4 v = *reinterpret_cast<const loss_f4*>(t.partials + 4l * r);
        a += (double)v[0];
        b += (double)v[1];
        c += (double)v[2];
      }
      red[0][tid] = a; red[1][tid] = b; red[2][tid] = c;
      __syncthreads();
      for (unsigned o = 128; o > 0; o >>= 1) {
        if (tid < o) {
          red[0][tid] += red[0][tid + o];
          red[1][tid] += red[1][tid + o];
          red[2][tid] += red[2][tid + o];
        }
        __syncthreads();
      }
      if (tid == 0) {
        const double s1 = red[0][0], nlab = red[1][0], s2 = red[2][0];
        const double w = (double)p.mix[k], K = (double)p.k;
        double L, den;
        if (t.kind == E2_LOSS_GAUSS_NLL) {
          den = t.n_tot;
          L = s1 / den;
        } else {
          den = nlab + 1.0;
          L = s1 / den;
          if (t.margin != nullptr) L -= (double)t.margin[0] * s2 / t.n_tot;
        }
        p.term_loss[k] = (float)L;
        p.coef[k] = (float)(w / (K * den));
        p.count[k] = (float)nlab;
        total += w * L;
      }
      __syncthreads();
    }
  }
  if (tid == 0) p.loss_out[0] = (float)(total / (double)p.k);
}

// work-groups of a launch over this many elements: 2048 elements (two quads per thread) each, at
// most `cap`; the kernels grid-stride beyond
unsigned loss_wgs(unsigned long long n_elem, unsigned cap) {
  const unsigned long long g = (n_elem + 2047ull) / 2048ull;
  return (unsigned)(g < 1 ? 1 : (g > cap ? cap : g));
}
#define E2_LOSS_FWD_CAP 1024u      /* the mix launch reads at most 16 KB per term */
#define E2_LOSS_BWD_CAP 2048u

// collapse over the views v[0..nv): w absorbs every next axis (h, d, c, n) whose stride equals the
// row length so far in ALL views; the axes left over keep their strides
int loss_geometry(const e2_tensor5* const* v, int nv, LossP& p, LView* const* lv, const char* who) {
  const e2_tensor5* t = v[0];
  E2_REQUIRE(t->n > 0 && t->c > 0 && t->d > 0 && t->h > 0 && t->w > 0,
             "%s: empty tensor (%d,%d,%d,%d,%d)", who, t->n, t->c, t->d, t->h, t->w);
  unsigned long long ext[4] = {(unsigned long long)t->h, (unsigned long long)t->d,
                               (unsigned long long)t->c, (unsigned long long)t->n};
  long st[5][4];
  for (int k = 0; k < nv; ++k) {
    st[k][0] = (long)v[k]->sh; st[k][1] = (long)v[k]->sd;
    st[k][2] = (long)v[k]->sc; st[k][3] = (long)v[k]->sn;
  }
  unsigned long long w = (unsigned long long)t->w;
  int first = 0;                     // first axis that stays outside the row
  while (first < 4) {
    bool join = true;
    for (int k = 0; k < nv; ++k) join = join && (ext[first] == 1 || st[k][first] == (long)w);
    if (!join || w * ext[first] >= (1ull << 31)) break;
    w *= ext[first];
    ++first;
  }
  unsigned long long e[4] = {1, 1, 1, 1}, rows = 1;
  for (int a = first; a < 4; ++a) { e[a - first] = ext[a]; rows *= ext[a]; }
  const unsigned long long quads = (w + 3) / 4, items = rows * quads;
  E2_REQUIRE(w < (1ull << 31) && items < (1ull << 31), "%s: tensor too large", who);
  for (int k = 0; k < nv; ++k)
    for (int a = 0; a < 4; ++a) lv[k]->s[a] = a + first < 4 ? st[k][a + first] : 0;
  p.w = (unsigned)w; p.quads = (unsigned)quads; p.items = (unsigned)items;
  p.e0 = (unsigned)e[0]; p.e1 = (unsigned)e[1]; p.e2 = (unsigned)e[2];
  p.dq = mk_div(p.quads); p.d0 = mk_div(p.e0); p.d1 = mk_div(p.e1); p.d2 = mk_div(p.e2);
  return 0;
}

unsigned long long n_elem(const e2_tensor5* t) {
  return (unsigned long long)t->n * t->c * t->d * t->h * t->w;
}

bool kind_ok(int k) { return k >= E2_LOSS_SQUARED && k <= E2_LOSS_GAUSS_NLL; }
bool has_margin(const e2_loss_term* t) {
  return (t->kind == E2_LOSS_SQUARED || t->kind == E2_LOSS_ABS) && t->margin != nullptr;
}
bool has_sc(const e2_loss_term* t) {
  return (t->kind == E2_LOSS_SQUARED || t->kind == E2_LOSS_ABS) && t->scale_correction != nullptr;
}

template <int KIND, bool MARGIN, bool SC, bool FLAG>
void launch_fwd(e2_ctx* ctx, unsigned wgs, const LossP& p) {
  hipLaunchKernelGGL((e2loss_fwd_kernel<KIND, MARGIN, SC, FLAG>), dim3(wgs), dim3(256), 0,
                     ctx->stream, p);
}
template <int KIND, bool MARGIN, bool SC, bool FLAG>
void launch_bwd(e2_ctx* ctx, unsigned wgs, const LossP& p, bool acc) {
  if (acc)
    hipLaunchKernelGGL((e2loss_bwd_kernel<KIND, MARGIN, SC, FLAG, true>), dim3(wgs), dim3(256), 0,
                       ctx->stream, p);
  else
    hipLaunchKernelGGL((e2loss_bwd_kernel<KIND, MARGIN, SC, FLAG, false>), dim3(wgs), dim3(256), 0,
                       ctx->stream, p);
}
template <int KIND>
void launch_fwd_ms(e2_ctx* ctx, unsigned wgs, const LossP& p, bool m, bool s) {
  if (m && s) launch_fwd<KIND, true, true, false>(ctx, wgs, p);
  else if (m) launch_fwd<KIND, true, false, false>(ctx, wgs, p);
  else if (s) launch_fwd<KIND, false, true, false>(ctx, wgs, p);
  else launch_fwd<KIND, false, false, false>(ctx, wgs, p);
}
template <int KIND>
void launch_bwd_ms(e2_ctx* ctx, unsigned wgs, const LossP& p, bool m, bool s, bool acc) {
  if (m && s) launch_bwd<KIND, true, true, false>(ctx, wgs, p, acc);
  else if (m) launch_bwd<KIND, true, false, false>(ctx, wgs, p, acc);
  else if (s) launch_bwd<KIND, false, true, false>(ctx, wgs, p, acc);
  else launch_bwd<KIND, false, false, false>(ctx, wgs, p, acc);
}

}  // namespace

extern "C" size_t e2_loss_partials(e2_ctx*, const e2_tensor5* pred) {
  if (!pred || pred->n <= 0 || pred->c <= 0 || pred->d <= 0 || pred->h <= 0 || pred->w <= 0)
    return 0;
  return (size_t)loss_wgs(n_elem(pred), E2_LOSS_FWD_CAP);
}

extern "C" int e2_loss_fwd(e2_ctx* ctx, const e2_loss_term* term, const e2_tensor5* pred,
                           const e2_tensor5* sig, const e2_tensor5* target, float* partials) {
  E2_REQUIRE(ctx && term && pred && target && partials && pred->ptr && target->ptr,
             "e2_loss_fwd: null argument");
  E2_REQUIRE(kind_ok(term->kind), "e2_loss_fwd: unknown loss kind %d", term->kind);
  E2_REQUIRE((((uintptr_t)partials) & 15) == 0, "e2_loss_fwd: partials must be 16-byte aligned");
  const bool gauss = term->kind == E2_LOSS_GAUSS_NLL;
  E2_REQUIRE(!gauss || (sig && sig->ptr), "e2_loss_fwd: GAUSS_NLL needs sig");
  E2_REQUIRE(same_size(pred, target) && (!gauss || same_size(pred, sig)),
             "e2_loss_fwd: size mismatch");
  LossP p = LossP{};
  const e2_tensor5* v[3] = {pred, target, sig};
  LView* lv[3] = {&p.vp, &p.vt, &p.vs};
  if (int rc = loss_geometry(v, gauss ? 3 : 2, p, lv, "e2_loss_fwd")) return rc;
  p.pred = pred->ptr; p.tgt = target->ptr; p.sig = gauss ? sig->ptr : nullptr;
  p.margin = term->margin; p.sc = term->scale_correction; p.partials = partials;
  const unsigned wgs = loss_wgs(n_elem(pred), E2_LOSS_FWD_CAP);
  const bool m = has_margin(term), s = has_sc(term);
  switch (term->kind) {
    case E2_LOSS_SQUARED: launch_fwd_ms<E2_LOSS_SQUARED>(ctx, wgs, p, m, s); break;
    case E2_LOSS_ABS: launch_fwd_ms<E2_LOSS_ABS>(ctx, wgs, p, m, s); break;
    case E2_LOSS_BINARY_NLL:
      if (term->subtract_label_entropy) launch_fwd<E2_LOSS_BINARY_NLL, false, false, true>(ctx, wgs, p);
      else launch_fwd<E2_LOSS_BINARY_NLL, false, false, false>(ctx, wgs, p);
      break;
    default:
      if (term->sig_is_log) launch_fwd<E2_LOSS_GAUSS_NLL, false, false, true>(ctx, wgs, p);
      else launch_fwd<E2_LOSS_GAUSS_NLL, false, false, false>(ctx, wgs, p);
      break;
  }
  E2_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" int e2_loss_mix(e2_ctx* ctx, int k, const e2_loss_term* terms,
                           float* const* partials, const size_t* rows, const int64_t* n_tot,
                           const float* mix, float* coef, float* term_loss, float* count,
                           float* loss_out) {
  E2_REQUIRE(ctx && terms && partials && rows && n_tot && mix && coef && term_loss && count &&
                 loss_out, "e2_loss_mix: null argument");
  E2_REQUIRE(k >= 1 && k <= E2_MAX_LOSS_TERMS, "e2_loss_mix: %d terms, 1..%d are supported", k,
             E2_MAX_LOSS_TERMS);
  MixP p = MixP{};
  p.k = k;
  for (int j = 0; j < k; ++j) {
    E2_REQUIRE(kind_ok(terms[j].kind), "e2_loss_mix: unknown loss kind %d", terms[j].kind);
    E2_REQUIRE(partials[j] && (((uintptr_t)partials[j]) & 15) == 0,
               "e2_loss_mix: partials[%d] null or not 16-byte aligned", j);
    E2_REQUIRE(rows[j] >= 1 && rows[j] <= E2_LOSS_FWD_CAP && n_tot[j] >= 1,
               "e2_loss_mix: term %d has %zu rows / %lld elements", j, rows[j], (long long)n_tot[j]);
    p.t[j].partials = partials[j];
    p.t[j].margin = has_margin(&terms[j]) ? terms[j].margin : nullptr;
    p.t[j].rows = (unsigned)rows[j];
    p.t[j].kind = terms[j].kind;
    p.t[j].n_tot = (double)n_tot[j];
  }
  p.mix = mix; p.coef = coef; p.term_loss = term_loss; p.count = count; p.loss_out = loss_out;
  hipLaunchKernelGGL(e2loss_mix_kernel, dim3(1), dim3(256), 0, ctx->stream, p);
  E2_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" int e2_loss_bwd(e2_ctx* ctx, const e2_loss_term* term, const e2_tensor5* pred,
                           const e2_tensor5* sig, const e2_tensor5* target, const float* coef,
                           const e2_tensor5* dpred, const e2_tensor5* dsig, int accumulate) {
  E2_REQUIRE(ctx && term && pred && target && coef && pred->ptr && target->ptr,
             "e2_loss_bwd: null argument");
  E2_REQUIRE(kind_ok(term->kind), "e2_loss_bwd: unknown loss kind %d", term->kind);
  const bool gauss = term->kind == E2_LOSS_GAUSS_NLL;
  E2_REQUIRE(!gauss || (sig && sig->ptr), "e2_loss_bwd: GAUSS_NLL needs sig");
  const bool wp = dpred && dpred->ptr, ws = gauss && dsig && dsig->ptr;
  E2_REQUIRE(wp || ws, "e2_loss_bwd: no gradient view given");
  E2_REQUIRE(gauss || !(dsig && dsig->ptr), "e2_loss_bwd: dsig is for GAUSS_NLL alone");
  E2_REQUIRE(same_size(pred, target) && (!gauss || same_size(pred, sig)) &&
                 (!wp || same_size(pred, dpred)) && (!ws || same_size(pred, dsig)),
             "e2_loss_bwd: size mismatch");
  LossP p = LossP{};
  const e2_tensor5* v[5];
  LView* lv[5];
  int nv = 0;
  v[nv] = pred; lv[nv++] = &p.vp;
  v[nv] = target; lv[nv++] = &p.vt;
  if (gauss) { v[nv] = sig; lv[nv++] = &p.vs; }
  if (wp) { v[nv] = dpred; lv[nv++] = &p.vdp; }
  if (ws) { v[nv] = dsig; lv[nv++] = &p.vds; }
  if (int rc = loss_geometry(v, nv, p, lv, "e2_loss_bwd")) return rc;
  p.pred = pred->ptr; p.tgt = target->ptr; p.sig = gauss ? sig->ptr : nullptr;
  p.dpred = wp ? dpred->ptr : nullptr; p.dsig = ws ? dsig->ptr : nullptr;
  p.margin = term->margin; p.sc = term->scale_correction; p.coef = coef;
  const unsigned wgs = loss_wgs(n_elem(pred), E2_LOSS_BWD_CAP);
  const bool m = has_margin(term), s = has_sc(term), acc = accumulate != 0;
  switch (term->kind) {
    case E2_LOSS_SQUARED: launch_bwd_ms<E2_LOSS_SQUARED>(ctx, wgs, p, m, s, acc); break;
    case E2_LOSS_ABS: launch_bwd_ms<E2_LOSS_ABS>(ctx, wgs, p, m, s, acc); break;
    case E2_LOSS_BINARY_NLL:       // (the label entropy does not depend on the prediction)
      launch_bwd<E2_LOSS_BINARY_NLL, false, false, false>(ctx, wgs, p, acc);
      break;
    default:
      if (term->sig_is_log) launch_bwd<E2_LOSS_GAUSS_NLL, false, false, true>(ctx, wgs, p, acc);
      else launch_bwd<E2_LOSS_GAUSS_NLL, false, false, false>(ctx, wgs, p, acc);
      break;
  }
  E2_CHECK_HIP(hipGetLastError());
  return 0;
}

// ---- BetaNLL (loss.py:890-950): entry points of its own; the slab rows are e2_loss_fwd's and the
// term is a GAUSS_NLL-kind row of e2_loss_mix (a plain mean over n_tot, no mask)
extern "C" int e2_beta_nll_fwd(e2_ctx* ctx, const e2_tensor5* mode, const e2_tensor5* conc,
                               const e2_tensor5* target, float* partials) {
  E2_REQUIRE(ctx && mode && conc && target && partials && mode->ptr && conc->ptr && target->ptr,
             "e2_beta_nll_fwd: null argument");
  E2_REQUIRE((((uintptr_t)partials) & 15) == 0, "e2_beta_nll_fwd: partials must be 16-byte aligned");
  E2_REQUIRE(same_size(mode, target) && same_size(mode, conc), "e2_beta_nll_fwd: size mismatch");
  LossP p = LossP{};
  const e2_tensor5* v[3] = {mode, target, conc};
  LView* lv[3] = {&p.vp, &p.vt, &p.vs};
  if (int rc = loss_geometry(v, 3, p, lv, "e2_beta_nll_fwd")) return rc;
  p.pred = mode->ptr; p.tgt = target->ptr; p.sig = conc->ptr; p.partials = partials;
  launch_fwd<E2I_LOSS_BETA_NLL, false, false, false>(ctx, loss_wgs(n_elem(mode), E2_LOSS_FWD_CAP), p);
  E2_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" int e2_beta_nll_bwd(e2_ctx* ctx, const e2_tensor5* mode, const e2_tensor5* conc,
                               const e2_tensor5* target, const float* coef,
                               const e2_tensor5* dmode, const e2_tensor5* dconc, int accumulate) {
  E2_REQUIRE(ctx && mode && conc && target && coef && mode->ptr && conc->ptr && target->ptr,
             "e2_beta_nll_bwd: null argument");
  const bool wp = dmode && dmode->ptr, ws = dconc && dconc->ptr;
  E2_REQUIRE(wp || ws, "e2_beta_nll_bwd: no gradient view given");
  E2_REQUIRE(same_size(mode, target) && same_size(mode, conc) && (!wp || same_size(mode, dmode)) &&
                 (!ws || same_size(mode, dconc)), "e2_beta_nll_bwd: size mismatch");
  LossP p = LossP{};
  const e2_tensor5* v[5];
  LView* lv[5];
  int nv = 0;
  v[nv] = mode; lv[nv++] = &p.vp;
  v[nv] = target; lv[nv++] = &p.vt;
  v[nv] = conc; lv[nv++] = &p.vs;
  if (wp) { v[nv] = dmode; lv[nv++] = &p.vdp; }
  if (ws) { v[nv] = dconc; lv[nv++] = &p.vds; }
  if (int rc = loss_geometry(v, nv, p, lv, "e2_beta_nll_bwd")) return rc;
  p.pred = mode->ptr; p.tgt = target->ptr; p.sig = conc->ptr;
  p.dpred = wp ? dmode->ptr : nullptr; p.dsig = ws ? dconc->ptr : nullptr; p.coef = coef;
  launch_bwd<E2I_LOSS_BETA_NLL, false, false, false>(ctx, loss_wgs(n_elem(mode), E2_LOSS_BWD_CAP), p,
                                                     accumulate != 0);
  E2_CHECK_HIP(hipGetLastError());
  return 0;
}
