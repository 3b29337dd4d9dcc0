// gauss_rv.hip -- the two nodes that make a conv net a variational autoencoder (various.py:32-151):
// GaussianRV, the re-parameterised sample z = mu + exp(log_sig) * eps with eps ~ N(0, 1), and its
// AEVB prior, the KL term 0.5 (mu^2 + sig^2 - 1 - 2 log_sig) (e2_gaussrv_fwd / _bwd,
// e2_aevb_prior_fwd / _bwd; the noise contract is written out in include/e2hip.h).
//
// eps of an element is a pure function of (seed, counter, stream, j), j its row-major index in the
// LOGICAL shape: one Philox4x32-10 block gives two pairs of uniforms, each pair one Box-Muller
// pair of normals -- the four normals of the quad j = 4q .. 4q + 3.  So one thread makes one block
// and moves its quad: as ONE 16-byte access per view where the quad lies in one aligned piece of a
// row in every view, element by element (same j, same normals) at row ends, odd pitches and
// misaligned views.  The backward pass makes the same block again: eps is never stored, the
// forward writes z alone and the backward reads dz and log_sig alone -- 12 bytes per element each
// way instead of 16 + 16 with a stored eps, and the 14 ALU instructions per round of Philox hide
// behind the HBM stream (dropout.hip is the same trade).
// The host collapses neighbouring axes that are dense in ALL views of a launch (a contiguous
// tensor becomes one long row; the channel halves of one (n, 2F, ...) buffer become n rows of
// F d h w), which changes no j.  No LDS and no atomics in the three streaming kernels; the
// prior's forward is a grid-stride sum that leaves one slab row per work-group (loss_elem.hip).
#include "stream_common.hpp"
#include "philox.hpp"

namespace {

#define GR_MAXV 4

typedef float gr_f4 __attribute__((ext_vector_type(4)));

struct GaussP {
  float* v[GR_MAXV];            // the views of the launch (unused / unwanted: null, strides 0)
  long s[GR_MAXV][5];           // element strides on the collapsed axes
  unsigned dim[5];              // collapsed logical extents, row-major (unused leading axes: 1)
  FastDiv div[5];
  unsigned long long total;     // number of elements = prod(dim)
  unsigned long long quads;     // ceil(total / 4)
  int unit;                     // innermost stride is 1 in every view (16-byte path possible)
  int acc0, acc1;               // bwd: add to what the first / second gradient view holds
  const unsigned* state;        // seed lo, seed hi, counter, -
  unsigned stream;
  const float* coef;            // prior bwd: the device scalar of e2_loss_mix
  float* partials;              // prior fwd: [gridDim.x][4]
};

// element j -> offsets in the NV views and its coordinate on the innermost axis
template <bool BIG, int NV>
__device__ __forceinline__ void decode(const GaussP& p, unsigned long long j, long (&off)[NV],
                                       unsigned& x) {
#pragma unroll
  for (int v = 0; v < NV; ++v) off[v] = 0;
  if (BIG) {
    unsigned long long r = j;
#pragma unroll
    for (int k = 4; k >= 1; --k) {
      const unsigned long long q = r / p.dim[k];
      const unsigned i = (unsigned)(r - q * p.dim[k]);
#pragma unroll
      for (int v = 0; v < NV; ++v) off[v] += (long)i * p.s[v][k];
      if (k == 4) x = i;
      r = q;
    }
#pragma unroll
    for (int v = 0; v < NV; ++v) off[v] += (long)r * p.s[v][0];
  } else {
    unsigned r = (unsigned)j;
#pragma unroll
    for (int k = 4; k >= 1; --k) {
      const unsigned q = fdiv(r, p.div[k]);
      const unsigned i = r - q * p.dim[k];
#pragma unroll
      for (int v = 0; v < NV; ++v) off[v] += (long)i * p.s[v][k];
      if (k == 4) x = i;
      r = q;
    }
#pragma unroll
    for (int v = 0; v < NV; ++v) off[v] += (long)r * p.s[v][0];
  }
}

// Box-Muller on two words: ua in (0, 1] and ub in [0, 1) are exact in f32 (24 bits each);
// cos(2 pi ub) as cospi(2 ub): the argument 2 ub is exact, no rounding of 2 pi ub enters
__device__ __forceinline__ void normal_pair(unsigned wa, unsigned wb, float& e0, float& e1) {
  const float ua = (float)((wa >> 8) + 1u) * 0x1p-24f;
  const float ub = (float)(wb >> 8) * 0x1p-24f;
  const float r = sqrtf(-2.0f * logf(ua));
  float sn, cs;
  sincospif(2.0f * ub, &sn, &cs);
  e0 = r * cs;
  e1 = r * sn;
}
// the four normals of quad q (elements 4q .. 4q + 3)
__device__ __forceinline__ gr_f4 quad_normals(const GaussP& p, unsigned long long q) {
  const unsigned k0 = p.state[0], k1 = p.state[1], cnt = p.state[2];
  const U4 r = philox4x32_10((unsigned)q, (unsigned)(q >> 32), p.stream, cnt, k0, k1);
  float e0, e1, e2, e3;
  normal_pair(r.x, r.y, e0, e1);
  normal_pair(r.z, r.w, e2, e3);
  gr_f4 e;
  e[0] = e0; e[1] = e1; e[2] = e2; e[3] = e3;
  return e;
}

// the quad lies inside one row and is 16-byte aligned in every view (a null view aligns)
template <int NV>
__device__ __forceinline__ bool quad_ok(const GaussP& p, unsigned x0, float* const (&a)[NV]) {
  uintptr_t al = 0;
#pragma unroll
  for (int v = 0; v < NV; ++v) al |= (uintptr_t)a[v];
  return p.unit && x0 + 4u <= p.dim[4] && (al & 15) == 0;
}

// out = mu + exp(log_sig) * eps.  Views: 0 mu, 1 log_sig, 2 out
template <bool BIG>
__global__ __launch_bounds__(256) void e2gauss_rv_fwd_kernel(GaussP p) {
  const unsigned long long q = (unsigned long long)blockIdx.x * 256ull + threadIdx.x;
  const unsigned long long j0 = q << 2;
  if (j0 >= p.total) return;
  const gr_f4 eps = quad_normals(p, q);
  long off[3];
  unsigned x0;
  decode<BIG, 3>(p, j0, off, x0);
  float* const a[3] = {p.v[0] + off[0], p.v[1] + off[1], p.v[2] + off[2]};
  if (quad_ok<3>(p, x0, a)) {
    const gr_f4 m = *reinterpret_cast<const gr_f4*>(a[0]);
    const gr_f4 ls = *reinterpret_cast<const gr_f4*>(a[1]);
    gr_f4 o;
    o[0] = m[0] + expf(ls[0]) * eps[0];
    o[1] = m[1] + expf(ls[1]) * eps[1];
    o[2] = m[2] + expf(ls[2]) * eps[2];
    o[3] = m[3] + expf(ls[3]) * eps[3];
    *reinterpret_cast<gr_f4*>(a[2]) = o;
    return;
  }
#pragma unroll
  for (unsigned e = 0; e < 4; ++e) {
    const unsigned long long j = j0 + e;
    if (j >= p.total) break;
    unsigned x;
    decode<BIG, 3>(p, j, off, x);
    const float ev = e == 0 ? eps[0] : (e == 1 ? eps[1] : (e == 2 ? eps[2] : eps[3]));
    p.v[2][off[2]] = p.v[0][off[0]] + expf(p.v[1][off[1]]) * ev;
  }
}

// dmu (=|+=) dout;  dlog_sig (=|+=) dout * eps * exp(log_sig), eps made again from the state the
// forward read.  Views: 0 dout, 1 log_sig, 2 dmu, 3 dlog_sig (either of the last two may be null)
template <bool BIG>
__global__ __launch_bounds__(256) void e2gauss_rv_bwd_kernel(GaussP p) {
  const unsigned long long q = (unsigned long long)blockIdx.x * 256ull + threadIdx.x;
  const unsigned long long j0 = q << 2;
  if (j0 >= p.total) return;
  const bool wm = p.v[2] != nullptr, ws = p.v[3] != nullptr;
  const bool am = p.acc0 != 0, as = p.acc1 != 0;
  gr_f4 eps = gr_f4{0.f, 0.f, 0.f, 0.f};
  if (ws) eps = quad_normals(p, q);        // (uniform: dmu alone needs no noise)
  long off[4];
  unsigned x0;
  decode<BIG, 4>(p, j0, off, x0);
  float* const a[4] = {p.v[0] + off[0], p.v[1] + off[1], wm ? p.v[2] + off[2] : nullptr,
                       ws ? p.v[3] + off[3] : nullptr};
  if (quad_ok<4>(p, x0, a)) {
    const gr_f4 g = *reinterpret_cast<const gr_f4*>(a[0]);
    if (wm) {
      gr_f4 o = g;
      if (am) o += *reinterpret_cast<const gr_f4*>(a[2]);
      *reinterpret_cast<gr_f4*>(a[2]) = o;
    }
    if (ws) {
      const gr_f4 ls = *reinterpret_cast<const gr_f4*>(a[1]);
      gr_f4 o;
      o[0] = g[0] * eps[0] * expf(ls[0]);
      o[1] = g[1] * eps[1] * expf(ls[1]);
      o[2] = g[2] * eps[2] * expf(ls[2]);
      o[3] = g[3] * eps[3] * expf(ls[3]);
      if (as) o += *reinterpret_cast<const gr_f4*>(a[3]);
      *reinterpret_cast<gr_f4*>(a[3]) = o;
    }
    return;
  }
#pragma unroll
  for (unsigned e = 0; e < 4; ++e) {
    const unsigned long long j = j0 + e;
    if (j >= p.total) break;
    unsigned x;
    decode<BIG, 4>(p, j, off, x);
    const float ev = e == 0 ? eps[0] : (e == 1 ? eps[1] : (e == 2 ? eps[2] : eps[3]));
    const float g = p.v[0][off[0]];
    if (wm) p.v[2][off[2]] = am ? p.v[2][off[2]] + g : g;
    if (ws) {
      const float d = g * ev * expf(p.v[1][off[1]]);
      p.v[3][off[3]] = as ? p.v[3][off[3]] + d : d;
    }
  }
}

// 0.5 (mu^2 + exp(2 log_sig) - 1 - 2 log_sig)
__device__ __forceinline__ float prior_elem(float m, float ls) {
  return 0.5f * (m * m + expf(2.0f * ls) - 1.0f - 2.0f * ls);
}

// one slab row (S1, elements, 0, 0) per work-group; quads q = wg * 256 + tid, then grid-stride.
// Views: 0 mu, 1 log_sig
template <bool BIG>
__global__ __launch_bounds__(256) void e2gauss_prior_fwd_kernel(GaussP p) {
  __shared__ float red[4];
  float s1 = 0.f, cnt = 0.f;
  const unsigned long long step = (unsigned long long)gridDim.x * 256ull;
  for (unsigned long long q = (unsigned long long)blockIdx.x * 256ull + threadIdx.x; q < p.quads;
       q += step) {
    const unsigned long long j0 = q << 2;
    long off[2];
    unsigned x0;
    decode<BIG, 2>(p, j0, off, x0);
    float* const a[2] = {p.v[0] + off[0], p.v[1] + off[1]};
    if (quad_ok<2>(p, x0, a)) {
      const gr_f4 m = *reinterpret_cast<const gr_f4*>(a[0]);
      const gr_f4 ls = *reinterpret_cast<const gr_f4*>(a[1]);
      s1 += prior_elem(m[0], ls[0]);
      s1 += prior_elem(m[1], ls[1]);
      s1 += prior_elem(m[2], ls[2]);
      s1 += prior_elem(m[3], ls[3]);
      cnt += 4.f;
    } else {
      for (unsigned e = 0; e < 4; ++e) {
        const unsigned long long j = j0 + e;
        if (j >= p.total) break;
        unsigned x;
        decode<BIG, 2>(p, j, off, x);
        s1 += prior_elem(p.v[0][off[0]], p.v[1][off[1]]);
        cnt += 1.f;
      }
    }
  }
  s1 = block_sum256(s1, red);
  cnt = block_sum256(cnt, red);
  if (threadIdx.x == 0) {
    gr_f4 r;
    r[0] = s1; r[1] = cnt; r[2] = 0.f; r[3] = 0.f;
    *reinterpret_cast<gr_f4*>(p.partials + 4l * blockIdx.x) = r;
  }
}

// dmu (=|+=) coef mu;  dlog_sig (=|+=) coef (exp(2 log_sig) - 1).
// Views: 0 mu, 1 log_sig, 2 dmu, 3 dlog_sig (either of the last two may be null)
template <bool BIG>
__global__ __launch_bounds__(256) void e2gauss_prior_bwd_kernel(GaussP p) {
  const unsigned long long q = (unsigned long long)blockIdx.x * 256ull + threadIdx.x;
  const unsigned long long j0 = q << 2;
  if (j0 >= p.total) return;
  const float co = e2_uniform_ld(p.coef, 0);
  const bool wm = p.v[2] != nullptr, ws = p.v[3] != nullptr;
  const bool am = p.acc0 != 0, as = p.acc1 != 0;
  long off[4];
  unsigned x0;
  decode<BIG, 4>(p, j0, off, x0);
  float* const a[4] = {p.v[0] + off[0], p.v[1] + off[1], wm ? p.v[2] + off[2] : nullptr,
                       ws ? p.v[3] + off[3] : nullptr};
  if (quad_ok<4>(p, x0, a)) {
    if (wm) {
      gr_f4 o = co * *reinterpret_cast<const gr_f4*>(a[0]);
      if (am) o += *reinterpret_cast<const gr_f4*>(a[2]);
      *reinterpret_cast<gr_f4*>(a[2]) = o;
    }
    if (ws) {
      const gr_f4 ls = *reinterpret_cast<const gr_f4*>(a[1]);
      gr_f4 o;
      o[0] = co * (expf(2.0f * ls[0]) - 1.0f);
      o[1] = co * (expf(2.0f * ls[1]) - 1.0f);
      o[2] = co * (expf(2.0f * ls[2]) - 1.0f);
      o[3] = co * (expf(2.0f * ls[3]) - 1.0f);
      if (as) o += *reinterpret_cast<const gr_f4*>(a[3]);
      *reinterpret_cast<gr_f4*>(a[3]) = o;
    }
    return;
  }
#pragma unroll
  for (unsigned e = 0; e < 4; ++e) {
    const unsigned long long j = j0 + e;
    if (j >= p.total) break;
    unsigned x;
    decode<BIG, 4>(p, j, off, x);
    if (wm) {
      const float d = co * p.v[0][off[0]];
      p.v[2][off[2]] = am ? p.v[2][off[2]] + d : d;
    }
    if (ws) {
      const float d = co * (expf(2.0f * p.v[1][off[1]]) - 1.0f);
      p.v[3][off[3]] = as ? p.v[3][off[3]] + d : d;
    }
  }
}

// Checks the views (t[k] may be null: not wanted) against t[0] and collapses: walking from the
// innermost axis outwards, an axis joins the current one when the two are dense in EVERY view (or
// one of them has extent 1) and the joint extent stays < 2^31
int gauss_geometry(const e2_tensor5* const* t, int nv, GaussP& p, const char* who) {
  const e2_tensor5* a = t[0];
  E2_REQUIRE(a->n > 0 && a->c > 0 && a->d > 0 && a->h > 0 && a->w > 0,
             "%s: empty tensor (%d,%d,%d,%d,%d)", who, a->n, a->c, a->d, a->h, a->w);
  E2_REQUIRE((unsigned long long)a->d * a->h * a->w < (1ull << 31),
             "%s: a channel of %llu elements, 2^31 or more are not supported", who,
             (unsigned long long)a->d * a->h * a->w);
  const unsigned dim[5] = {(unsigned)a->n, (unsigned)a->c, (unsigned)a->d, (unsigned)a->h,
                           (unsigned)a->w};
  long st[GR_MAXV][5];
  for (int v = 0; v < GR_MAXV; ++v) {
    const e2_tensor5* b = v < nv ? t[v] : nullptr;
    if (b) E2_REQUIRE(same_size(a, b), "%s: views of different sizes", who);
    p.v[v] = b ? b->ptr : nullptr;
    st[v][0] = b ? (long)b->sn : 0; st[v][1] = b ? (long)b->sc : 0; st[v][2] = b ? (long)b->sd : 0;
    st[v][3] = b ? (long)b->sh : 0; st[v][4] = b ? 1 : 0;
  }
  p.total = 1;
  for (int k = 0; k < 5; ++k) p.total *= dim[k];
  unsigned cd[5];
  long cs[GR_MAXV][5];
  int nc = 0;
  for (int k = 4; k >= 0; --k) {
    const int top = nc - 1;
    if (nc > 0 && dim[k] == 1) continue;
    bool take = nc == 0 || cd[top] == 1, join = nc > 0 && !take;
    if (join) {
      for (int v = 0; v < GR_MAXV; ++v)
        join = join && (p.v[v] == nullptr || st[v][k] == (long)cd[top] * cs[v][top]);
      join = join && (unsigned long long)cd[top] * dim[k] < (1ull << 31);
    }
    if (join) { cd[top] *= dim[k]; continue; }
    const int dst = take && nc > 0 ? top : nc++;
    cd[dst] = dim[k];
    for (int v = 0; v < GR_MAXV; ++v) cs[v][dst] = st[v][k];
  }
  p.unit = 1;
  for (int k = 0; k < 5; ++k) {            // cd[0] is the innermost axis -> p.dim[4]
    const int src = 4 - k;
    p.dim[k] = src < nc ? cd[src] : 1u;
    p.div[k] = mk_div(p.dim[k]);
    for (int v = 0; v < GR_MAXV; ++v) p.s[v][k] = src < nc ? cs[v][src] : 0;
  }
  for (int v = 0; v < GR_MAXV; ++v)
    if (p.v[v] != nullptr && p.s[v][4] != 1) p.unit = 0;
  p.quads = (p.total + 3) / 4;
  E2_REQUIRE((p.quads + 255) / 256 < (1ull << 31), "%s: tensor too large", who);
  return 0;
}

bool given(const e2_tensor5* t) { return t != nullptr && t->ptr != nullptr; }

#define GR_LAUNCH(KERNEL, BLOCKS, P)                                                            \
  do {                                                                                          \
    if ((P).total < (1ull << 31))                                                               \
      hipLaunchKernelGGL(KERNEL<false>, dim3((unsigned)(BLOCKS)), dim3(256), 0, ctx->stream, P); \
    else                                                                                        \
      hipLaunchKernelGGL(KERNEL<true>, dim3((unsigned)(BLOCKS)), dim3(256), 0, ctx->stream, P);  \
    E2_CHECK_HIP(hipGetLastError());                                                            \
  } while (0)

}  // namespace

// various.py:61-83 (n_samples = 0): z = mu + exp(log_sig) * rng.normal(mu.shape)
extern "C" int e2_gaussrv_fwd(e2_ctx* ctx, const e2_tensor5* mu, const e2_tensor5* log_sig,
                              const e2_tensor5* out, const void* state, uint32_t stream) {
  E2_REQUIRE(ctx && given(mu) && given(log_sig) && given(out), "e2_gaussrv_fwd: null argument");
  E2_REQUIRE(state != nullptr, "e2_gaussrv_fwd: null state");
  E2_REQUIRE(((uintptr_t)state & 15) == 0, "e2_gaussrv_fwd: state must be 16-byte aligned");
  E2_REQUIRE(out->ptr != mu->ptr && out->ptr != log_sig->ptr,
             "e2_gaussrv_fwd: out may alias neither input");
  GaussP p = GaussP{};
  const e2_tensor5* t[3] = {mu, log_sig, out};
  if (int rc = gauss_geometry(t, 3, p, "e2_gaussrv_fwd")) return rc;
  p.state = (const unsigned*)state; p.stream = stream;
  GR_LAUNCH(e2gauss_rv_fwd_kernel, (p.quads + 255) / 256, p);
  return 0;
}

// T.grad of various.py:61-83: dz/dmu = 1, dz/dlog_sig = exp(log_sig) * eps
extern "C" int e2_gaussrv_bwd(e2_ctx* ctx, const e2_tensor5* dout, const e2_tensor5* log_sig,
                              const e2_tensor5* dmu, const e2_tensor5* dlog_sig, int acc_mu,
                              int acc_sig, const void* state, uint32_t stream) {
  E2_REQUIRE(ctx && given(dout) && given(log_sig), "e2_gaussrv_bwd: null argument");
  E2_REQUIRE(state != nullptr, "e2_gaussrv_bwd: null state");
  E2_REQUIRE(((uintptr_t)state & 15) == 0, "e2_gaussrv_bwd: state must be 16-byte aligned");
  E2_REQUIRE(given(dmu) || given(dlog_sig), "e2_gaussrv_bwd: no gradient view given");
  GaussP p = GaussP{};
  const e2_tensor5* t[4] = {dout, log_sig, given(dmu) ? dmu : nullptr,
                            given(dlog_sig) ? dlog_sig : nullptr};
  if (int rc = gauss_geometry(t, 4, p, "e2_gaussrv_bwd")) return rc;
  p.state = (const unsigned*)state; p.stream = stream;
  p.acc0 = acc_mu != 0; p.acc1 = acc_sig != 0;
  GR_LAUNCH(e2gauss_rv_bwd_kernel, (p.quads + 255) / 256, p);
  return 0;
}

// various.py:134-151 (n_samples = 0): prior = 0.5 (mu^2 + sig^2 - 1 - 2 log_sig); its mean is the
// term of AggregateLoss (loss.py:1357-1363)
extern "C" int e2_aevb_prior_fwd(e2_ctx* ctx, const e2_tensor5* mu, const e2_tensor5* log_sig,
                                 float* partials) {
  E2_REQUIRE(ctx && given(mu) && given(log_sig) && partials, "e2_aevb_prior_fwd: null argument");
  E2_REQUIRE((((uintptr_t)partials) & 15) == 0,
             "e2_aevb_prior_fwd: partials must be 16-byte aligned");
  GaussP p = GaussP{};
  const e2_tensor5* t[2] = {mu, log_sig};
  if (int rc = gauss_geometry(t, 2, p, "e2_aevb_prior_fwd")) return rc;
  p.partials = partials;
  const size_t rows = e2_loss_partials(ctx, mu);       // (one row per work-group, every row written)
  GR_LAUNCH(e2gauss_prior_fwd_kernel, rows, p);
  return 0;
}

// T.grad of various.py:134-151 times the coefficient of the mix: d/dmu = mu, d/dlog_sig =
// exp(2 log_sig) - 1
extern "C" int e2_aevb_prior_bwd(e2_ctx* ctx, const e2_tensor5* mu, const e2_tensor5* log_sig,
                                 const float* coef, const e2_tensor5* dmu,
                                 const e2_tensor5* dlog_sig, int acc_mu, int acc_sig) {
  E2_REQUIRE(ctx && given(mu) && given(log_sig) && coef, "e2_aevb_prior_bwd: null argument");
  E2_REQUIRE(given(dmu) || given(dlog_sig), "e2_aevb_prior_bwd: no gradient view given");
  GaussP p = GaussP{};
  const e2_tensor5* t[4] = {mu, log_sig, given(dmu) ? dmu : nullptr,
                            given(dlog_sig) ? dlog_sig : nullptr};
  if (int rc = gauss_geometry(t, 4, p, "e2_aevb_prior_bwd")) return rc;
  p.coef = coef;
  p.acc0 = acc_mu != 0; p.acc1 = acc_sig != 0;
  GR_LAUNCH(e2gauss_prior_bwd_kernel, (p.quads + 255) / 256, p);
  return 0;
}
