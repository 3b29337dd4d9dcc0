// act.hip -- bias + activation as an op of its own on strided 5-D views (e2_act_fwd / e2_act_bwd;
// computations.py:57-134 apply_activation): tanh, sigmoid, abs, elu, selu, soft+ next to relu / lin.
//
//   fwd:  out  = f(pre + bias[c])
//   bwd:  dpre = dout * f'(pre + bias[c]);   dbias[c] += sum over n, z, y, x of dpre
//
// Nodes with relu / lin never come here (their bias + activation lives in the pooling kernels and
// the GEMM epilogues); a node with one of the other functions runs its 'lin' launches, which leave
// v = pre + bias's operand in a buffer, and then this pair.
//
// The activation is a template parameter: the host switches over eight instantiations, no kernel
// branches per element.  A work-group stays inside one (n, c): the bias is one scalar load and the
// bias gradient one block reduction + one atomic.  A thread owns FOUR consecutive x of one row and
// moves them as one 16-byte access where that row piece is 16-byte aligned in every view, element
// by element at row ends and on misaligned views (odd pitches, Crop offsets); nothing outside a
// view is read or written.  Neighbouring spatial axes that are dense in all views are collapsed
// on the host (a contiguous (d, h, w) block becomes one long row).  Pure streams: no LDS beyond
// the reduction scratch, no workspace.
//
// Slopes at the kinks follow the reading of Theano the relu rule rests on (T.nnet.relu =
// 0.5 (v + |v|) and grad |v| = sgn v with sgn 0 = 0, hence relu'(0) = 0.5): abs'(0) = 0, and
// elu / selu are switch(v > 0, v, alpha * expm1(v)), whose gradient at v = 0 (either sign of
// zero) is the SECOND branch's: alpha * e^0.  Theano cannot be imported where this is developed:
// abs'(0) and elu'(0) / selu'(0) are pinned by that reading alone, not by a recorded run.
//
// All arithmetic is f32 in forms that stay finite over the whole f32 range of v (no e^{+|v|}):
// sigmoid through e^-|v|, soft+ as max(v, 0) + log1p(e^-|v|), elu / selu through expm1f, tanh'
// from the tanh just computed.
#include "stream_common.hpp"

namespace {

#define E2_SELU_ALPHA 1.6732632423543772848170429916717f
#define E2_SELU_SCALE 1.0507009873554804934193349852946f

// f(v)
template <int ACT>
__device__ __forceinline__ float act_f(float v) {
  if (ACT == E2_ACT_RELU) return fmaxf(v, 0.f);
  if (ACT == E2_ACT_TANH) return tanhf(v);
  if (ACT == E2_ACT_SIGMOID) {
    const float e = expf(-fabsf(v));                        // e in [0, 1]
    return (v >= 0.f ? 1.f : e) / (1.f + e);
  }
  if (ACT == E2_ACT_ABS) return fabsf(v);
  if (ACT == E2_ACT_ELU) return v > 0.f ? v : expm1f(v);
  if (ACT == E2_ACT_SELU) return E2_SELU_SCALE * (v > 0.f ? v : E2_SELU_ALPHA * expm1f(v));
  if (ACT == E2_ACT_SOFTPLUS) return fmaxf(v, 0.f) + log1pf(expf(-fabsf(v)));
  return v;
}

// f'(v)
template <int ACT>
__device__ __forceinline__ float act_df(float v) {
  if (ACT == E2_ACT_RELU) return v > 0.f ? 1.f : (v == 0.f ? 0.5f : 0.f);
  if (ACT == E2_ACT_TANH) {
    const float t = tanhf(v);
    return 1.f - t * t;
  }
  if (ACT == E2_ACT_SIGMOID) {      // f (1 - f) = e / (1 + e)^2 with e = e^-|v|: no cancellation
    const float e = expf(-fabsf(v));
    const float q = 1.f + e;
    return e / (q * q);
  }
  if (ACT == E2_ACT_ABS) return v > 0.f ? 1.f : (v < 0.f ? -1.f : 0.f);
  if (ACT == E2_ACT_ELU) return v > 0.f ? 1.f : expf(v);
  if (ACT == E2_ACT_SELU) return v > 0.f ? E2_SELU_SCALE : E2_SELU_SCALE * (E2_SELU_ALPHA * expf(v));
  if (ACT == E2_ACT_SOFTPLUS) {     // sigmoid v
    const float e = expf(-fabsf(v));
    return (v >= 0.f ? 1.f : e) / (1.f + e);
  }
  return 1.f;
}

// the (d, h, w) block of one (n, c) after the host's collapse: `rows` rows of `w` elements
struct ActP {
  const float* a;               // fwd: pre      bwd: dout
  const float* b;               // fwd: unused   bwd: pre
  float* o;                     // fwd: out      bwd: dpre
  long an, ac, ar1, ar0;        // strides: batch, feature, outer row axis, inner row axis
  long bn, bc, br1, br0;
  long on, oc, or1, or0;
  unsigned w, r0;               // row length; extent of the inner row axis (rows = r1 * r0)
  unsigned quads;               // ceil(w / 4)
  unsigned items;               // rows * quads  (< 2^31)
  unsigned chunk;               // items per work-group, a multiple of 256
  FastDiv dq, dr0;
  const float* bias;
  float* dbias;
};

typedef float act_f4 __attribute__((ext_vector_type(4)));

template <int ACT, bool HAS_BIAS>
__global__ __launch_bounds__(256) void e2act_fwd_kernel(ActP p) {
  const unsigned s0 = blockIdx.x * p.chunk;
  const unsigned s1 = min(s0 + p.chunk, p.items);
  const unsigned c = blockIdx.y, n = blockIdx.z;
  const float bv = HAS_BIAS ? p.bias[c] : 0.f;
  const float* abase = p.a + (long)n * p.an + (long)c * p.ac;
  float* obase = p.o + (long)n * p.on + (long)c * p.oc;
  for (unsigned s = s0 + threadIdx.x; s < s1; s += 256) {
    const unsigned row = fdiv(s, p.dq);
    const unsigned x0 = (s - row * p.quads) << 2;
    const unsigned i1 = fdiv(row, p.dr0);
    const unsigned i0 = row - i1 * p.r0;
    const float* src = abase + (long)i1 * p.ar1 + (long)i0 * p.ar0 + x0;
    float* dst = obase + (long)i1 * p.or1 + (long)i0 * p.or0 + x0;
    if (x0 + 4u <= p.w && ((((uintptr_t)src) | ((uintptr_t)dst)) & 15) == 0) {
      const act_f4 v = *reinterpret_cast<const act_f4*>(src);
      act_f4 r;
      r[0] = act_f<ACT>(v[0] + bv);
      r[1] = act_f<ACT>(v[1] + bv);
      r[2] = act_f<ACT>(v[2] + bv);
      r[3] = act_f<ACT>(v[3] + bv);
      *reinterpret_cast<act_f4*>(dst) = r;
    } else {
      const unsigned nv = min(4u, p.w - x0);
      for (unsigned e = 0; e < nv; ++e) dst[e] = act_f<ACT>(src[e] + bv);
    }
  }
}

template <int ACT, bool HAS_BIAS>
__global__ __launch_bounds__(256) void e2act_bwd_kernel(ActP p) {
  __shared__ float red[4];
  const unsigned s0 = blockIdx.x * p.chunk;
  const unsigned s1 = min(s0 + p.chunk, p.items);
  const unsigned c = blockIdx.y, n = blockIdx.z;
  const float bv = HAS_BIAS ? p.bias[c] : 0.f;
  const float* gbase = p.a + (long)n * p.an + (long)c * p.ac;
  const float* vbase = p.b + (long)n * p.bn + (long)c * p.bc;
  float* obase = p.o + (long)n * p.on + (long)c * p.oc;
  float gsum = 0.f;
  for (unsigned s = s0 + threadIdx.x; s < s1; s += 256) {
    const unsigned row = fdiv(s, p.dq);
    const unsigned x0 = (s - row * p.quads) << 2;
    const unsigned i1 = fdiv(row, p.dr0);
    const unsigned i0 = row - i1 * p.r0;
    const float* g = gbase + (long)i1 * p.ar1 + (long)i0 * p.ar0 + x0;
    const float* pre = vbase + (long)i1 * p.br1 + (long)i0 * p.br0 + x0;
    float* dst = obase + (long)i1 * p.or1 + (long)i0 * p.or0 + x0;
    if (x0 + 4u <= p.w &&
        ((((uintptr_t)g) | ((uintptr_t)pre) | ((uintptr_t)dst)) & 15) == 0) {
      const act_f4 gv = *reinterpret_cast<const act_f4*>(g);
      const act_f4 v = *reinterpret_cast<const act_f4*>(pre);
      act_f4 r;
      r[0] = gv[0] * act_df<ACT>(v[0] + bv);
      r[1] = gv[1] * act_df<ACT>(v[1] + bv);
      r[2] = gv[2] * act_df<ACT>(v[2] + bv);
      r[3] = gv[3] * act_df<ACT>(v[3] + bv);
      *reinterpret_cast<act_f4*>(dst) = r;
      gsum += (r[0] + r[1]) + (r[2] + r[3]);
    } else {
      const unsigned nv = min(4u, p.w - x0);
      for (unsigned e = 0; e < nv; ++e) {
        const float r = g[e] * act_df<ACT>(pre[e] + bv);
        dst[e] = r;
        gsum += r;
      }
    }
  }
  if (p.dbias != nullptr) {          // (uniform over the grid)
    gsum = wave_sum(gsum);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) red[wave] = gsum;
    __syncthreads();
    if (threadIdx.x == 0) {
      const float tot = (red[0] + red[1]) + (red[2] + red[3]);
      if (tot != 0.f) unsafeAtomicAdd(p.dbias + c, tot);
    }
  }
}

// geometry shared by the two launches: collapse (d, h, w) over the views in `v` (nv of them)
// want_per_cu / per_max: work-groups wanted per CU before the chunks shrink, and the largest chunk
// in items per thread
int act_geometry(e2_ctx* ctx, const e2_tensor5* const* v, int nv, ActP& p, dim3& grid,
                 const char* who, unsigned want_per_cu, unsigned per_max) {
  const e2_tensor5* t = v[0];
  E2_REQUIRE(t->n > 0 && t->c > 0 && t->d > 0 && t->h > 0 && t->w > 0,
             "%s: empty tensor (%d,%d,%d,%d,%d)", who, t->n, t->c, t->d, t->h, t->w);
  E2_REQUIRE(t->c <= 65535 && t->n <= 65535, "%s: more than 65535 features / batch entries", who);
  unsigned long long w = (unsigned long long)t->w, r0 = (unsigned long long)t->h,
                     r1 = (unsigned long long)t->d;
  long s0[3], s1[3];                 // strides of the inner / outer row axis, per view
  for (int k = 0; k < nv; ++k) { s0[k] = (long)v[k]->sh; s1[k] = (long)v[k]->sd; }
  // h joins w where every view's rows follow each other without a gap (or there is one row)
  bool join = true;
  for (int k = 0; k < nv; ++k) join = join && (r0 == 1 || s0[k] == (long)w);
  if (join && w * r0 < (1ull << 31)) {
    w *= r0; r0 = r1; r1 = 1;
    for (int k = 0; k < nv; ++k) { s0[k] = s1[k]; s1[k] = 0; }
    join = true;
    for (int k = 0; k < nv; ++k) join = join && (r0 == 1 || s0[k] == (long)w);
    if (join && w * r0 < (1ull << 31)) {
      w *= r0; r0 = 1;
      for (int k = 0; k < nv; ++k) s0[k] = 0;
    }
  }
  const unsigned long long quads = (w + 3) / 4, items = r1 * r0 * quads;
  E2_REQUIRE(w < (1ull << 31) && items < (1ull << 31), "%s: feature map too large", who);
  p.w = (unsigned)w; p.r0 = (unsigned)r0; p.quads = (unsigned)quads; p.items = (unsigned)items;
  p.dq = mk_div(p.quads); p.dr0 = mk_div(p.r0);
  p.an = (long)v[0]->sn; p.ac = (long)v[0]->sc; p.ar0 = s0[0]; p.ar1 = s1[0];
  const int kb = nv == 3 ? 1 : 0, ko = nv - 1;
  p.bn = (long)v[kb]->sn; p.bc = (long)v[kb]->sc; p.br0 = s0[kb]; p.br1 = s1[kb];
  p.on = (long)v[ko]->sn; p.oc = (long)v[ko]->sc; p.or0 = s0[ko]; p.or1 = s1[ko];
  p.chunk = stream_chunk(ctx, (unsigned long long)t->n * t->c, items, per_max, want_per_cu);
  grid = dim3((unsigned)((items + p.chunk - 1) / p.chunk), (unsigned)t->c, (unsigned)t->n);
  return 0;
}

template <int ACT>
void launch_fwd(e2_ctx* ctx, dim3 grid, const ActP& p) {
  if (p.bias)
    hipLaunchKernelGGL((e2act_fwd_kernel<ACT, true>), grid, dim3(256), 0, ctx->stream, p);
  else
    hipLaunchKernelGGL((e2act_fwd_kernel<ACT, false>), grid, dim3(256), 0, ctx->stream, p);
}
template <int ACT>
void launch_bwd(e2_ctx* ctx, dim3 grid, const ActP& p) {
  if (p.bias)
    hipLaunchKernelGGL((e2act_bwd_kernel<ACT, true>), grid, dim3(256), 0, ctx->stream, p);
  else
    hipLaunchKernelGGL((e2act_bwd_kernel<ACT, false>), grid, dim3(256), 0, ctx->stream, p);
}

}  // namespace

extern "C" int e2_act_fwd(e2_ctx* ctx, const e2_tensor5* pre, const float* bias, int act,
                          const e2_tensor5* out) {
  E2_REQUIRE(ctx && pre && out && pre->ptr && out->ptr, "e2_act_fwd: null argument");
  E2_REQUIRE(same_size(pre, out), "e2_act_fwd: size mismatch");
  E2_REQUIRE(act >= E2_ACT_LIN && act <= E2_ACT_SOFTPLUS, "e2_act_fwd: unknown activation %d", act);
  ActP p = ActP{};
  dim3 grid;
  const e2_tensor5* v[2] = {pre, out};
  if (int rc = act_geometry(ctx, v, 2, p, grid, "e2_act_fwd", 8, 8)) return rc;
  p.a = pre->ptr; p.b = nullptr; p.o = out->ptr; p.bias = bias; p.dbias = nullptr;
  switch (act) {
    case E2_ACT_LIN: launch_fwd<E2_ACT_LIN>(ctx, grid, p); break;
    case E2_ACT_RELU: launch_fwd<E2_ACT_RELU>(ctx, grid, p); break;
    case E2_ACT_TANH: launch_fwd<E2_ACT_TANH>(ctx, grid, p); break;
    case E2_ACT_SIGMOID: launch_fwd<E2_ACT_SIGMOID>(ctx, grid, p); break;
    case E2_ACT_ABS: launch_fwd<E2_ACT_ABS>(ctx, grid, p); break;
    case E2_ACT_ELU: launch_fwd<E2_ACT_ELU>(ctx, grid, p); break;
    case E2_ACT_SELU: launch_fwd<E2_ACT_SELU>(ctx, grid, p); break;
    default: launch_fwd<E2_ACT_SOFTPLUS>(ctx, grid, p); break;
  }
  E2_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" int e2_act_bwd(e2_ctx* ctx, const e2_tensor5* dout, const e2_tensor5* pre,
                          const float* bias, int act, const e2_tensor5* dpre, float* dbias) {
  E2_REQUIRE(ctx && dout && pre && dpre && dout->ptr && pre->ptr && dpre->ptr,
             "e2_act_bwd: null argument");
  E2_REQUIRE(same_size(dout, pre) && same_size(dout, dpre), "e2_act_bwd: size mismatch");
  E2_REQUIRE(act >= E2_ACT_LIN && act <= E2_ACT_SOFTPLUS, "e2_act_bwd: unknown activation %d", act);
  ActP p = ActP{};
  dim3 grid;
  const e2_tensor5* v[3] = {dout, pre, dpre};
  // (Known lever: with a bias gradient the atomics of one channel hit ONE address and serialise,
  // about 0.2 us each as measured on (1, 20, 23, 90, 90); longer chunks would trade them for
  // fewer work-groups.  Not taken here without a measurement of its own.)
  if (int rc = act_geometry(ctx, v, 3, p, grid, "e2_act_bwd", 8, 8)) return rc;
  p.a = dout->ptr; p.b = pre->ptr; p.o = dpre->ptr; p.bias = bias; p.dbias = dbias;
  switch (act) {
    case E2_ACT_LIN: launch_bwd<E2_ACT_LIN>(ctx, grid, p); break;
    case E2_ACT_RELU: launch_bwd<E2_ACT_RELU>(ctx, grid, p); break;
    case E2_ACT_TANH: launch_bwd<E2_ACT_TANH>(ctx, grid, p); break;
    case E2_ACT_SIGMOID: launch_bwd<E2_ACT_SIGMOID>(ctx, grid, p); break;
    case E2_ACT_ABS: launch_bwd<E2_ACT_ABS>(ctx, grid, p); break;
    case E2_ACT_ELU: launch_bwd<E2_ACT_ELU>(ctx, grid, p); break;
    case E2_ACT_SELU: launch_bwd<E2_ACT_SELU>(ctx, grid, p); break;
    default: launch_bwd<E2_ACT_SOFTPLUS>(ctx, grid, p); break;
  }
  E2_CHECK_HIP(hipGetLastError());
  return 0;
}
