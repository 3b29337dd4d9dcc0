// arena_ops.hip -- grid-stride sweeps over flat arenas: the flat fills (one region, many regions
// in one launch) and the four optimiser updates (one sweep, arena_sweep, over the rules of
// opt_rules.hpp).  Bound by HBM, one launch each.  The fills and the updates share this
// translation unit.
#include "common.hpp"
#include "opt_rules.hpp"
#include <algorithm>
#include <initializer_list>

__global__ void fill_flat_kernel(float* p, size_t n, float v) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n;
       i += (size_t)gridDim.x * blockDim.x)
    p[i] = v;
}

// many flat fills in one launch (blockIdx.y = region)
__global__ void fill_multi_kernel(float* const* __restrict__ ptrs,
                                  const unsigned long long* __restrict__ counts, float v) {
  float* p = ptrs[blockIdx.y];
  const size_t n = (size_t)counts[blockIdx.y];
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n;
       i += (size_t)gridDim.x * blockDim.x)
    p[i] = v;
}

// ---------------------------------------------------------------------------
// optimisers on a flat arena (hyper = {lr, mom, beta2, wd, t, factor, -, arrivals})
// ---------------------------------------------------------------------------
// Every tensor of the arena starts on a 16-byte boundary and is padded to a multiple of
// four elements (model.py ensure_arena), so a float4 never straddles two tensors: one
// weight-decay multiplier per float4, found by a binary search over the segment table in
// LDS.  The step counter t of Adam and AdaGrad lives on the device (hipGraph replay cannot
// pass a new value): every work-group reads t_old, uses it, and the LAST work-group to
// finish -- an arrival counter, at most 256 arrivals -- publishes t for the next step.
// No work-group can still need t_old then.  (A separate one-thread "tick" kernel took 5 us
// per step; one arrival per work-group of a 4096-group grid serialised for 46 us.)
constexpr int kOptMaxSeg = 1024;
__device__ __forceinline__ float seg_mult_lds(const long* so, const float* sr, int n_seg, size_t i) {
  int lo = 0, hi = n_seg - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if ((size_t)so[mid] <= i) lo = mid; else hi = mid - 1;
  }
  return sr[lo];
}

__device__ __forceinline__ float& comp(float4& v, int c) { return c == 0 ? v.x : c == 1 ? v.y : c == 2 ? v.z : v.w; }

// The sweep of all four optimisers; Rule (opt_rules.hpp) is what happens to one element, st the
// rule's state arenas.
// gdiv / gmul: the gradient that enters the update is g * gmul / (gdiv ? gdiv[0] + 1e-5 : 1) --
// the data-parallel step sums UNNORMALISED gradients over the ranks and divides by the summed
// labelled-voxel count here (one device scalar behind the arena) instead of in elementwise
// launches of its own.  zero_g: the arena is left ZERO for the next backward pass, which then
// needs no fill launch (e2_adam_step_ex).  All loads of an element come before its first store:
// g is read AND cleared here, and a load behind a store to the same array waits for it.
template <class Rule, class Hyper>
__device__ __forceinline__ void arena_sweep(float* __restrict__ p, float* __restrict__ g,
                                            float* const (&st)[Rule::NS], size_t n,
                                            const int64_t* __restrict__ seg_off,
                                            const float* __restrict__ seg_reg, int n_seg, Hyper hyper,
                                            const float* __restrict__ gdiv, float gmul, int zero_g) {
  constexpr int NS = Rule::NS;
  __shared__ long so[kOptMaxSeg];
  __shared__ float sr[kOptMaxSeg];
  for (int i = threadIdx.x; i < n_seg; i += blockDim.x) { so[i] = seg_off[i]; sr[i] = seg_reg[i]; }
  const Rule rule(hyper);
  const float gs = gdiv ? gmul / (gdiv[0] + 1e-5f) : gmul;
  __syncthreads();
  const size_t n4 = n >> 2;
  float4* p4 = reinterpret_cast<float4*>(p);
  float4* g4 = reinterpret_cast<float4*>(g);
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n4;
       i += (size_t)gridDim.x * blockDim.x) {
    float4 gv = g4[i];
    float4 sv[NS];
#pragma unroll
    for (int k = 0; k < NS; ++k) sv[k] = reinterpret_cast<float4*>(st[k])[i];
    float4 pv = p4[i];
    if (gs != 1.f) { gv.x *= gs; gv.y *= gs; gv.z *= gs; gv.w *= gs; }
    if (zero_g) g4[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    const float mult = rule.mult(seg_mult_lds(so, sr, n_seg, 4 * i));
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      float e[NS];
#pragma unroll
      for (int k = 0; k < NS; ++k) e[k] = comp(sv[k], c);
      rule.apply(comp(pv, c), comp(gv, c), e, mult);
#pragma unroll
      for (int k = 0; k < NS; ++k) comp(sv[k], c) = e[k];
    }
#pragma unroll
    for (int k = 0; k < NS; ++k) reinterpret_cast<float4*>(st[k])[i] = sv[k];
    p4[i] = pv;
  }
  if (blockIdx.x == 0)                                 // (n is a multiple of 4 in the plan's arena)
    for (size_t i = 4 * n4 + threadIdx.x; i < n; i += blockDim.x) {
      const float gi = g[i] * gs;
      float e[NS];
#pragma unroll
      for (int k = 0; k < NS; ++k) e[k] = st[k][i];
      float pi = p[i];
      if (zero_g) g[i] = 0.f;
      rule.apply(pi, gi, e, rule.mult(seg_mult_lds(so, sr, n_seg, i)));
#pragma unroll
      for (int k = 0; k < NS; ++k) st[k][i] = e[k];
      p[i] = pi;
    }
  if constexpr (Rule::kCounter) {
    // publish t once every work-group has read the old value
    __syncthreads();
    if (threadIdx.x == 0) {
      unsigned* arrivals = reinterpret_cast<unsigned*>(hyper + 7);
      const unsigned prev = __hip_atomic_fetch_add(arrivals, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (prev == gridDim.x - 1) {
        __hip_atomic_store(arrivals, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        rule.publish(hyper);
      }
    }
  }
}

// (The kernels keep their names: the profiles and the tools that compare kernel times find them by name.)
__global__ __launch_bounds__(256) void adam_kernel(float* __restrict__ p, float* __restrict__ g,
                                                   float* __restrict__ m, float* __restrict__ s, size_t n,
                                                   const int64_t* __restrict__ seg_off,
                                                   const float* __restrict__ seg_reg, int n_seg,
                                                   float* __restrict__ hyper,
                                                   const float* __restrict__ gdiv, float gmul, int zero_g) {
  arena_sweep<AdamRule>(p, g, {m, s}, n, seg_off, seg_reg, n_seg, hyper, gdiv, gmul, zero_g);
}

__global__ __launch_bounds__(256) void sgd_kernel(float* __restrict__ p, float* __restrict__ g,
                                                  float* __restrict__ d, size_t n,
                                                  const int64_t* __restrict__ seg_off,
                                                  const float* __restrict__ seg_reg, int n_seg,
                                                  const float* __restrict__ hyper,
                                                  const float* __restrict__ gdiv, float gmul, int zero_g) {
  arena_sweep<SgdRule>(p, g, {d}, n, seg_off, seg_reg, n_seg, hyper, gdiv, gmul, zero_g);
}

__global__ __launch_bounds__(256) void adagrad_kernel(float* __restrict__ p, float* __restrict__ g,
                                                      float* __restrict__ h, size_t n,
                                                      const int64_t* __restrict__ seg_off,
                                                      const float* __restrict__ seg_reg, int n_seg,
                                                      float* __restrict__ hyper,
                                                      const float* __restrict__ gdiv, float gmul, int zero_g) {
  arena_sweep<AdaGradRule>(p, g, {h}, n, seg_off, seg_reg, n_seg, hyper, gdiv, gmul, zero_g);
}

__global__ __launch_bounds__(256) void adadelta_kernel(float* __restrict__ p, float* __restrict__ g,
                                                       float* __restrict__ s, float* __restrict__ d, size_t n,
                                                       const int64_t* __restrict__ seg_off,
                                                       const float* __restrict__ seg_reg, int n_seg,
                                                       const float* __restrict__ hyper,
                                                       const float* __restrict__ gdiv, float gmul, int zero_g) {
  arena_sweep<AdaDeltaRule>(p, g, {s, d}, n, seg_off, seg_reg, n_seg, hyper, gdiv, gmul, zero_g);
}


// Flat fill as a KERNEL, also for zeros: hipMemsetAsync nodes inside a captured
// hipGraph were observed to be re-ordered against the kernel that follows them on
// replay (unet3d_lite: the split-K accumulation of a conv started from stale data in
// ~1 of 3 processes); kernel nodes keep their order.
int e2i_fill_flat(e2_ctx* ctx, float* ptr, size_t n, float value) {
  if (n == 0) return 0;
  int grid = (int)std::min<size_t>((n + 255) / 256, 8192);
  hipLaunchKernelGGL(fill_flat_kernel, dim3(grid), dim3(256), 0, ctx->stream, ptr, n, value);
  E2_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" int e2_fill_multi(e2_ctx* ctx, const void* ptrs_dev, const void* counts_dev,
                             int nregions, float value) {
  E2_REQUIRE(ctx && ptrs_dev && counts_dev && nregions > 0 && nregions < 65536,
             "e2_fill_multi: bad argument");
  hipLaunchKernelGGL(fill_multi_kernel, dim3(512, nregions), dim3(256), 0, ctx->stream,
                     (float* const*)ptrs_dev, (const unsigned long long*)counts_dev, value);
  E2_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" int e2_fill(e2_ctx* ctx, float* ptr, size_t n, float value) {
  E2_REQUIRE(ctx && ptr, "e2_fill: null argument");
  return e2i_fill_flat(ctx, ptr, n, value);
}

// The checks of the four e2_*_step_ex entry points and the grid of their launch.  arenas: p, g and
// the rule's state; counter: the rule publishes t through the arrival counter, which takes at most
// 256 arrivals -- one work-group per CU, where the other two rules run two.  launch(grid) enqueues
// the kernel.
template <class Launch>
static int opt_step(e2_ctx* ctx, const char* name, bool counter, std::initializer_list<const float*> arenas,
                    size_t n, const int64_t* seg_off, const float* seg_reg, int n_seg, const float* hyper,
                    Launch launch) {
  bool all = true;
  uintptr_t bits = 0;
  for (const float* a : arenas) { all = all && a; bits |= (uintptr_t)a; }
  E2_REQUIRE(ctx && all && seg_off && seg_reg && hyper && n_seg > 0, "%s: null argument", name);
  E2_REQUIRE(n_seg <= kOptMaxSeg, "%s: %d parameter tensors (at most %d)", name, n_seg, kOptMaxSeg);
  E2_REQUIRE((bits & 15) == 0, "%s: arenas must be 16-byte aligned", name);
  const size_t cap = (counter ? 1 : 2) * (size_t)ctx->num_cu;
  launch(dim3((unsigned)std::min<size_t>(std::max<size_t>((n / 4 + 255) / 256, 1), cap)));
  E2_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" int e2_adam_step(e2_ctx* ctx, float* p, const float* g, float* m, float* s,
                            size_t n, const int64_t* seg_off, const float* seg_reg,
                            int n_seg, const float* hyper) {
  return e2_adam_step_ex(ctx, p, const_cast<float*>(g), m, s, n, seg_off, seg_reg, n_seg, hyper,
                         nullptr, 1.f, 0);
}

extern "C" int e2_adam_step_ex(e2_ctx* ctx, float* p, float* g, float* m, float* s,
                               size_t n, const int64_t* seg_off, const float* seg_reg,
                               int n_seg, const float* hyper, const float* gdiv, float gmul,
                               int zero_g) {
  return opt_step(ctx, "adam_step", AdamRule::kCounter, {p, g, m, s}, n, seg_off, seg_reg, n_seg, hyper, [&](dim3 grid) {
    hipLaunchKernelGGL(adam_kernel, grid, dim3(256), 0, ctx->stream, p, g, m, s, n, seg_off, seg_reg,
                       n_seg, const_cast<float*>(hyper), gdiv, gmul, zero_g ? 1 : 0);
  });
}

extern "C" int e2_sgd_step(e2_ctx* ctx, float* p, const float* g, float* d, size_t n,
                           const int64_t* seg_off, const float* seg_reg, int n_seg,
                           const float* hyper) {
  return e2_sgd_step_ex(ctx, p, const_cast<float*>(g), d, n, seg_off, seg_reg, n_seg, hyper,
                        nullptr, 1.f, 0);
}

extern "C" int e2_sgd_step_ex(e2_ctx* ctx, float* p, float* g, float* d, size_t n,
                              const int64_t* seg_off, const float* seg_reg, int n_seg,
                              const float* hyper, const float* gdiv, float gmul, int zero_g) {
  return opt_step(ctx, "sgd_step", SgdRule::kCounter, {p, g, d}, n, seg_off, seg_reg, n_seg, hyper, [&](dim3 grid) {
    hipLaunchKernelGGL(sgd_kernel, grid, dim3(256), 0, ctx->stream, p, g, d, n, seg_off, seg_reg,
                       n_seg, hyper, gdiv, gmul, zero_g ? 1 : 0);
  });
}

extern "C" int e2_adagrad_step_ex(e2_ctx* ctx, float* p, float* g, float* h, size_t n,
                                  const int64_t* seg_off, const float* seg_reg, int n_seg,
                                  const float* hyper, const float* gdiv, float gmul, int zero_g) {
  return opt_step(ctx, "adagrad_step", AdaGradRule::kCounter, {p, g, h}, n, seg_off, seg_reg, n_seg, hyper, [&](dim3 grid) {
    hipLaunchKernelGGL(adagrad_kernel, grid, dim3(256), 0, ctx->stream, p, g, h, n, seg_off, seg_reg,
                       n_seg, const_cast<float*>(hyper), gdiv, gmul, zero_g ? 1 : 0);
  });
}

extern "C" int e2_adadelta_step_ex(e2_ctx* ctx, float* p, float* g, float* s, float* d, size_t n,
                                   const int64_t* seg_off, const float* seg_reg, int n_seg,
                                   const float* hyper, const float* gdiv, float gmul, int zero_g) {
  return opt_step(ctx, "adadelta_step", AdaDeltaRule::kCounter, {p, g, s, d}, n, seg_off, seg_reg, n_seg, hyper, [&](dim3 grid) {
    hipLaunchKernelGGL(adadelta_kernel, grid, dim3(256), 0, ctx->stream, p, g, s, d, n, seg_off, seg_reg,
                       n_seg, hyper, gdiv, gmul, zero_g ? 1 : 0);
  });
}
