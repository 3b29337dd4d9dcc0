// dropout.hip -- Bernoulli(1 - rate) gates made on the device and applied to a strided 5-D view
// (e2_dropout_fwd / _bwd / _tick; the contract is written out in include/e2hip.h).
//
// The gate of an element is a pure function of (seed, counter, stream, j): one Philox4x32-10
// block yields the words of four consecutive gate indices j, so one thread makes one block and
// moves its four elements -- as ONE 16-byte access where they lie in one aligned piece of a row,
// element by element (same j, same words) at row ends, odd pitches and misaligned views.
// j is the row-major index in the LOGICAL shape; the host collapses neighbouring axes that are
// dense in both views (a contiguous tensor becomes one long row), which changes no j.
// A pure stream: no LDS, no atomics, no cross-work-group traffic; the counter is advanced by a
// launch of its own (dropout_tick_kernel) in front of the step's dropout launches.
#include "stream_common.hpp"

namespace {

struct DropP {
  const float* src;
  float* dst;
  unsigned dim[5];              // collapsed logical extents, row-major (unused leading axes: 1)
  long ss[5], ds[5];            // element strides of the two views
  FastDiv div[5];
  unsigned long long total;     // number of elements = prod(dim)
  const float* rate;
  const unsigned* state;        // seed lo, seed hi, counter, -
  unsigned stream;
  int feature;                  // 1: gate index = coordinate on axis 1 (axes are NOT collapsed)
  int unit;                     // innermost stride is 1 in both views (16-byte path possible)
};

struct U4 {
  unsigned x, y, z, w;
};

__device__ __forceinline__ U4 philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3,
                                            unsigned k0, unsigned k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const unsigned hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const unsigned hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    const unsigned n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
    c0 = n0; c1 = lo1; c2 = n2; c3 = lo0;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  return U4{c0, c1, c2, c3};
}
// (a select chain: indexing a register array with a run-time index would go through scratch)
__device__ __forceinline__ unsigned pick(const U4& r, unsigned i) {
  return i == 0 ? r.x : (i == 1 ? r.y : (i == 2 ? r.z : r.w));
}

// element j -> offsets in the two views, its coordinate on the innermost axis and on axis 1
template <bool BIG>
__device__ __forceinline__ void decode(const DropP& p, unsigned long long j, long& so, long& dof,
                                       unsigned& x, unsigned& c) {
  so = 0; dof = 0; c = 0;
  if (BIG) {
    unsigned long long r = j;
#pragma unroll
    for (int k = 4; k >= 1; --k) {
      const unsigned long long q = r / p.dim[k];
      const unsigned i = (unsigned)(r - q * p.dim[k]);
      so += (long)i * p.ss[k]; dof += (long)i * p.ds[k];
      if (k == 4) x = i;
      if (k == 1) c = i;
      r = q;
    }
    so += (long)r * p.ss[0]; dof += (long)r * p.ds[0];
  } else {
    unsigned r = (unsigned)j;
#pragma unroll
    for (int k = 4; k >= 1; --k) {
      const unsigned q = fdiv(r, p.div[k]);
      const unsigned i = r - q * p.dim[k];
      so += (long)i * p.ss[k]; dof += (long)i * p.ds[k];
      if (k == 4) x = i;
      if (k == 1) c = i;
      r = q;
    }
    so += (long)r * p.ss[0]; dof += (long)r * p.ds[0];
  }
}

template <bool BIG>
__global__ __launch_bounds__(256) void dropout_kernel(DropP p) {
  const unsigned long long q = (unsigned long long)blockIdx.x * 256ull + threadIdx.x;
  const unsigned long long j0 = q << 2;
  if (j0 >= p.total) return;
  const float rate = *p.rate;
  const unsigned T = rate >= 1.0f ? 0xffffffffu : (unsigned)(rate * 4294967296.0f);
  const float scale = 1.0f / (1.0f - rate);
  const unsigned k0 = p.state[0], k1 = p.state[1], cnt = p.state[2];
  long so, dof;
  unsigned x0, c0;
  decode<BIG>(p, j0, so, dof, x0, c0);
  U4 r = U4{0, 0, 0, 0};
  if (!p.feature) r = philox4x32_10((unsigned)q, (unsigned)(q >> 32), p.stream, cnt, k0, k1);
  const float* s = p.src + so;
  float* d = p.dst + dof;
  // four elements of one row (never past the end: the row ends inside the tensor), both 16-byte aligned
  if (p.unit && x0 + 4u <= p.dim[4] && ((((uintptr_t)s) | ((uintptr_t)d)) & 15) == 0) {
    if (p.feature) {          // one feature, one gate for all four
      const unsigned w = pick(philox4x32_10(c0 >> 2, 0u, p.stream, cnt, k0, k1), c0 & 3u);
      r = U4{w, w, w, w};
    }
    const float4 v = *reinterpret_cast<const float4*>(s);
    float4 o;
    o.x = r.x >= T ? v.x * scale : 0.0f;
    o.y = r.y >= T ? v.y * scale : 0.0f;
    o.z = r.z >= T ? v.z * scale : 0.0f;
    o.w = r.w >= T ? v.w * scale : 0.0f;
    *reinterpret_cast<float4*>(d) = o;
    return;
  }
#pragma unroll
  for (unsigned e = 0; e < 4; ++e) {
    const unsigned long long j = j0 + e;
    if (j >= p.total) break;
    unsigned x, c;
    decode<BIG>(p, j, so, dof, x, c);
    unsigned w = e == 0 ? r.x : (e == 1 ? r.y : (e == 2 ? r.z : r.w));
    if (p.feature) w = pick(philox4x32_10(c >> 2, 0u, p.stream, cnt, k0, k1), c & 3u);
    const float v = p.src[so];
    p.dst[dof] = w >= T ? v * scale : 0.0f;
  }
}

__global__ void dropout_tick_kernel(unsigned* state) {
  if (blockIdx.x == 0 && threadIdx.x == 0) state[2] = state[2] + 1u;
}

int dropout_launch(e2_ctx* ctx, const e2_tensor5* a, const e2_tensor5* b, int feature,
                   const float* rate, const void* state, uint32_t stream, const char* who) {
  E2_REQUIRE(ctx && a && b && a->ptr && b->ptr && rate && state, "%s: null argument", who);
  E2_REQUIRE(((uintptr_t)state & 15) == 0, "%s: state must be 16-byte aligned", who);
  E2_REQUIRE(a->n > 0 && a->c > 0 && a->d > 0 && a->h > 0 && a->w > 0,
             "%s: empty tensor (%d,%d,%d,%d,%d)", who, a->n, a->c, a->d, a->h, a->w);
  E2_REQUIRE(same_size(a, b), "%s: size mismatch", who);
  const unsigned dim[5] = {(unsigned)a->n, (unsigned)a->c, (unsigned)a->d, (unsigned)a->h,
                           (unsigned)a->w};
  const long ss[5] = {(long)a->sn, (long)a->sc, (long)a->sd, (long)a->sh, 1};
  const long ds[5] = {(long)b->sn, (long)b->sc, (long)b->sd, (long)b->sh, 1};
  DropP p;
  p.src = a->ptr; p.dst = b->ptr; p.rate = rate; p.state = (const unsigned*)state;
  p.stream = stream; p.feature = feature ? 1 : 0;
  p.total = 1;
  for (int k = 0; k < 5; ++k) p.total *= dim[k];
  // collapse: walk from the innermost axis outwards; an axis joins the current one when the two
  // are dense in BOTH views (or when one of them has extent 1) and the joint extent stays < 2^31
  unsigned cd[5]; long cs[5], cq[5];
  int nc = 0;
  if (p.feature) {
    for (int k = 4; k >= 0; --k) { cd[nc] = dim[k]; cs[nc] = ss[k]; cq[nc] = ds[k]; ++nc; }
  } else {
    for (int k = 4; k >= 0; --k) {
      if (nc == 0) { cd[0] = dim[k]; cs[0] = ss[k]; cq[0] = ds[k]; nc = 1; continue; }
      if (dim[k] == 1) continue;
      int t = nc - 1;
      if (cd[t] == 1) { cd[t] = dim[k]; cs[t] = ss[k]; cq[t] = ds[k]; continue; }
      if (ss[k] == (long)cd[t] * cs[t] && ds[k] == (long)cd[t] * cq[t] &&
          (unsigned long long)cd[t] * dim[k] < (1ull << 31)) {
        cd[t] *= dim[k];
        continue;
      }
      cd[nc] = dim[k]; cs[nc] = ss[k]; cq[nc] = ds[k]; ++nc;
    }
  }
  for (int k = 0; k < 5; ++k) {            // cd[0] is the innermost axis -> p.dim[4]
    const int src = 4 - k;
    p.dim[k] = src < nc ? cd[src] : 1u;
    p.ss[k] = src < nc ? cs[src] : 0;
    p.ds[k] = src < nc ? cq[src] : 0;
    p.div[k] = mk_div(p.dim[k]);
  }
  p.unit = (p.ss[4] == 1 && p.ds[4] == 1) ? 1 : 0;
  const unsigned long long nq = (p.total + 3) / 4, blocks = (nq + 255) / 256;
  E2_REQUIRE(blocks < (1ull << 31), "%s: tensor too large", who);
  if (p.total < (1ull << 31))
    hipLaunchKernelGGL(dropout_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, ctx->stream, p);
  else
    hipLaunchKernelGGL(dropout_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, ctx->stream, p);
  E2_CHECK_HIP(hipGetLastError());
  return 0;
}

}  // namespace

extern "C" int e2_dropout_fwd(e2_ctx* ctx, const e2_tensor5* x, const e2_tensor5* out,
                              int feature_mode, const float* rate, const void* state,
                              uint32_t stream) {
  return dropout_launch(ctx, x, out, feature_mode, rate, state, stream, "e2_dropout_fwd");
}

// dx = keep ? dout * scale : 0 -- the product's derivative is the same gate (neural.py:714-720
// under T.grad), so the backward pass is the forward kernel on the gradient
extern "C" int e2_dropout_bwd(e2_ctx* ctx, const e2_tensor5* dout, const e2_tensor5* dx,
                              int feature_mode, const float* rate, const void* state,
                              uint32_t stream) {
  return dropout_launch(ctx, dout, dx, feature_mode, rate, state, stream, "e2_dropout_bwd");
}

extern "C" int e2_dropout_tick(e2_ctx* ctx, void* state) {
  E2_REQUIRE(ctx && state && ((uintptr_t)state & 15) == 0,
             "e2_dropout_tick: null / misaligned state");
  hipLaunchKernelGGL(dropout_tick_kernel, dim3(1), dim3(64), 0, ctx->stream, (unsigned*)state);
  E2_CHECK_HIP(hipGetLastError());
  return 0;
}
