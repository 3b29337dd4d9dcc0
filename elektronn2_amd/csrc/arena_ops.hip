// arena_ops.hip -- grid-stride sweeps over flat arenas: the flat fills (one region, many regions
// in one launch) and the reference's Adam / SGD updates.  Bound by HBM, one launch each.
// (The fills and the updates share this translation unit on purpose: compiled without the fill
// kernels next to them, adam_kernel and sgd_kernel come out of hipcc with four instructions
// changed -- a logical for an arithmetic shift in seg_mult_lds.)
#include "common.hpp"
#include <algorithm>

#define E2_EPS_ADAM 1e-5f

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
// LDS.  Adam's step counter t lives on the device (hipGraph replay cannot pass a new
// value): every work-group reads t_old, uses t = t_old + 1, and the LAST work-group to
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

// gdiv / gmul: the gradient that enters the update is g * gmul / (gdiv ? gdiv[0] + 1e-5 : 1) --
// the data-parallel step sums UNNORMALISED gradients over the ranks and divides by the summed
// labelled-voxel count here (one device scalar behind the arena) instead of in elementwise
// launches of its own.  zero_g: the arena is left ZERO for the next backward pass, which then
// needs no fill launch (e2_adam_step_ex).
__global__ __launch_bounds__(256) void adam_kernel(float* __restrict__ p, float* __restrict__ g,
                                                   float* __restrict__ m, float* __restrict__ s, size_t n,
                                                   const int64_t* __restrict__ seg_off,
                                                   const float* __restrict__ seg_reg, int n_seg,
                                                   float* __restrict__ hyper,
                                                   const float* __restrict__ gdiv, float gmul, int zero_g) {
  __shared__ long so[kOptMaxSeg];
  __shared__ float sr[kOptMaxSeg];
  for (int i = threadIdx.x; i < n_seg; i += blockDim.x) { so[i] = seg_off[i]; sr[i] = seg_reg[i]; }
  const float lr = hyper[0], mom = hyper[1], b2 = hyper[2], wd = hyper[3];
  const float t = hyper[4] + 1.f;
  const float fac = sqrtf(1.f - powf(b2, t)) / (1.f - powf(mom, t));
  const float gs = gdiv ? gmul / (gdiv[0] + 1e-5f) : gmul;
  __syncthreads();
  const size_t n4 = n >> 2;
  float4* p4 = reinterpret_cast<float4*>(p);
  float4* g4 = reinterpret_cast<float4*>(g);
  float4* m4 = reinterpret_cast<float4*>(m);
  float4* s4 = reinterpret_cast<float4*>(s);
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n4;
       i += (size_t)gridDim.x * blockDim.x) {
    float4 gv = g4[i];
    const float4 mv = m4[i], sv = s4[i];
    float4 pv = p4[i];
    if (gs != 1.f) { gv.x *= gs; gv.y *= gs; gv.z *= gs; gv.w *= gs; }
    if (zero_g) g4[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    const float mult = seg_mult_lds(so, sr, n_seg, 4 * i) * wd;
    float4 nm, ns;
#define E2_ADAM1(c)                                                      \
    nm.c = mom * mv.c + (1.f - mom) * gv.c;                              \
    ns.c = b2 * sv.c + (1.f - b2) * gv.c * gv.c;                         \
    {                                                                    \
      float dir = fac * nm.c / sqrtf(ns.c + E2_EPS_ADAM);                \
      if (mult != 0.f) dir += mult * pv.c;                               \
      pv.c = pv.c - lr * dir;                                            \
    }
    E2_ADAM1(x) E2_ADAM1(y) E2_ADAM1(z) E2_ADAM1(w)
#undef E2_ADAM1
    m4[i] = nm; s4[i] = ns; p4[i] = pv;
  }
  if (blockIdx.x == 0)                                 // (n is a multiple of 4 in the plan's arena)
    for (size_t i = 4 * n4 + threadIdx.x; i < n; i += blockDim.x) {
      const float gi = g[i] * gs;
      if (zero_g) g[i] = 0.f;
      const float nm = mom * m[i] + (1.f - mom) * gi;
      const float ns = b2 * s[i] + (1.f - b2) * gi * gi;
      float dir = fac * nm / sqrtf(ns + E2_EPS_ADAM);
      const float mult = seg_mult_lds(so, sr, n_seg, i) * wd;
      const float pi = p[i];
      if (mult != 0.f) dir += mult * pi;
      m[i] = nm; s[i] = ns; p[i] = pi - lr * dir;
    }
  // publish t once every work-group has read the old value
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned* arrivals = reinterpret_cast<unsigned*>(hyper + 7);
    const unsigned prev = __hip_atomic_fetch_add(arrivals, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (prev == gridDim.x - 1) {
      __hip_atomic_store(arrivals, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      hyper[4] = t;
      hyper[5] = fac;
    }
  }
}

__global__ __launch_bounds__(256) void sgd_kernel(float* __restrict__ p, float* __restrict__ g,
                                                  float* __restrict__ d, size_t n,
                                                  const int64_t* __restrict__ seg_off,
                                                  const float* __restrict__ seg_reg, int n_seg,
                                                  const float* __restrict__ hyper,
                                                  const float* __restrict__ gdiv, float gmul, int zero_g) {
  __shared__ long so[kOptMaxSeg];
  __shared__ float sr[kOptMaxSeg];
  for (int i = threadIdx.x; i < n_seg; i += blockDim.x) { so[i] = seg_off[i]; sr[i] = seg_reg[i]; }
  const float lr = hyper[0], mom = hyper[1], wd = hyper[3];
  const float gs = gdiv ? gmul / (gdiv[0] + 1e-5f) : gmul;
  __syncthreads();
  const size_t n4 = n >> 2;
  float4* p4 = reinterpret_cast<float4*>(p);
  float4* g4 = reinterpret_cast<float4*>(g);
  float4* d4 = reinterpret_cast<float4*>(d);
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n4;
       i += (size_t)gridDim.x * blockDim.x) {
    float4 gv = g4[i];
    const float4 dv = d4[i];
    float4 pv = p4[i];
    if (gs != 1.f) { gv.x *= gs; gv.y *= gs; gv.z *= gs; gv.w *= gs; }
    if (zero_g) g4[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    const float mult = seg_mult_lds(so, sr, n_seg, 4 * i) * wd;
    float4 nd;
#define E2_SGD1(c)                                                       \
    nd.c = gv.c + mom * dv.c;                                            \
    pv.c = pv.c - lr * (mult != 0.f ? nd.c + mult * pv.c : nd.c);
    E2_SGD1(x) E2_SGD1(y) E2_SGD1(z) E2_SGD1(w)
#undef E2_SGD1
    d4[i] = nd; p4[i] = pv;
  }
  if (blockIdx.x == 0)
    for (size_t i = 4 * n4 + threadIdx.x; i < n; i += blockDim.x) {
      const float nd = g[i] * gs + mom * d[i];
      if (zero_g) g[i] = 0.f;
      const float mult = seg_mult_lds(so, sr, n_seg, i) * wd;
      const float pi = p[i];
      d[i] = nd;
      p[i] = pi - lr * (mult != 0.f ? nd + mult * pi : nd);
    }
}

// AdaGrad (optimiser.py:168-214 of the reference): h' = h + c g^2, p' = p - lr / sqrt(h') (g + wd r p).
// c = 2 at the first step (t_old == 0): the reference's init_func adds g^2 of the same batch once
// before its first step adds it again (optimiser.py:200-214), one launch here in place of a second
// forward / backward pass.  r = 1 where the segment has a multiplier at all: the reference has no
// apply_reg > 1 branch for AdaGrad (optimiser.py:187-189).  Where h' == 0 -- a gradient that has
// been exactly zero since the start -- the element is left as it is (the reference divides by
// sqrt(0)).  t lives in hyper[4] and is published by the last work-group to arrive, as in
// adam_kernel.
__global__ __launch_bounds__(256) void adagrad_kernel(float* __restrict__ p, float* __restrict__ g,
                                                      float* __restrict__ h, size_t n,
                                                      const int64_t* __restrict__ seg_off,
                                                      const float* __restrict__ seg_reg, int n_seg,
                                                      float* __restrict__ hyper,
                                                      const float* __restrict__ gdiv, float gmul, int zero_g) {
  __shared__ long so[kOptMaxSeg];
  __shared__ float sr[kOptMaxSeg];
  for (int i = threadIdx.x; i < n_seg; i += blockDim.x) { so[i] = seg_off[i]; sr[i] = seg_reg[i]; }
  const float lr = hyper[0], wd = hyper[3];
  const float t_old = hyper[4];
  const float c = t_old == 0.f ? 2.f : 1.f;
  const float gs = gdiv ? gmul / (gdiv[0] + 1e-5f) : gmul;
  __syncthreads();
  const size_t n4 = n >> 2;
  float4* p4 = reinterpret_cast<float4*>(p);
  float4* g4 = reinterpret_cast<float4*>(g);
  float4* h4 = reinterpret_cast<float4*>(h);
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n4;
       i += (size_t)gridDim.x * blockDim.x) {
    float4 gv = g4[i];
    const float4 hv = h4[i];
    float4 pv = p4[i];
    if (gs != 1.f) { gv.x *= gs; gv.y *= gs; gv.z *= gs; gv.w *= gs; }
    if (zero_g) g4[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    const float rw = seg_mult_lds(so, sr, n_seg, 4 * i) != 0.f ? wd : 0.f;
    float4 nh;
#define E2_ADAGRAD1(k)                                                   \
    nh.k = hv.k + c * (gv.k * gv.k);                                     \
    if (nh.k != 0.f)                                                     \
      pv.k = pv.k - lr / sqrtf(nh.k) * (rw != 0.f ? gv.k + rw * pv.k : gv.k);
    E2_ADAGRAD1(x) E2_ADAGRAD1(y) E2_ADAGRAD1(z) E2_ADAGRAD1(w)
#undef E2_ADAGRAD1
    h4[i] = nh; p4[i] = pv;
  }
  if (blockIdx.x == 0)
    for (size_t i = 4 * n4 + threadIdx.x; i < n; i += blockDim.x) {
      const float gi = g[i] * gs;
      if (zero_g) g[i] = 0.f;
      const float nh = h[i] + c * (gi * gi);
      const float rw = seg_mult_lds(so, sr, n_seg, i) != 0.f ? wd : 0.f;
      const float pi = p[i];
      h[i] = nh;
      if (nh != 0.f) p[i] = pi - lr / sqrtf(nh) * (rw != 0.f ? gi + rw * pi : gi);
    }
  // publish t once every work-group has read the old value
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned* arrivals = reinterpret_cast<unsigned*>(hyper + 7);
    const unsigned prev = __hip_atomic_fetch_add(arrivals, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (prev == gridDim.x - 1) {
      __hip_atomic_store(arrivals, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      hyper[4] = t_old + 1.f;
    }
  }
}

// AdaDelta (optimiser.py:222-264), eps = 1e-5 inside both roots; the direction takes the OLD s and
// the OLD d, as the reference has it; the multiplier as in sgd_kernel.  No step counter.
__global__ __launch_bounds__(256) void adadelta_kernel(float* __restrict__ p, float* __restrict__ g,
                                                       float* __restrict__ s, float* __restrict__ d, size_t n,
                                                       const int64_t* __restrict__ seg_off,
                                                       const float* __restrict__ seg_reg, int n_seg,
                                                       const float* __restrict__ hyper,
                                                       const float* __restrict__ gdiv, float gmul, int zero_g) {
  __shared__ long so[kOptMaxSeg];
  __shared__ float sr[kOptMaxSeg];
  for (int i = threadIdx.x; i < n_seg; i += blockDim.x) { so[i] = seg_off[i]; sr[i] = seg_reg[i]; }
  const float lr = hyper[0], mom = hyper[1], wd = hyper[3];
  const float gs = gdiv ? gmul / (gdiv[0] + 1e-5f) : gmul;
  __syncthreads();
  const size_t n4 = n >> 2;
  float4* p4 = reinterpret_cast<float4*>(p);
  float4* g4 = reinterpret_cast<float4*>(g);
  float4* s4 = reinterpret_cast<float4*>(s);
  float4* d4 = reinterpret_cast<float4*>(d);
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n4;
       i += (size_t)gridDim.x * blockDim.x) {
    float4 gv = g4[i];
    const float4 sv = s4[i], dv = d4[i];
    float4 pv = p4[i];
    if (gs != 1.f) { gv.x *= gs; gv.y *= gs; gv.z *= gs; gv.w *= gs; }
    if (zero_g) g4[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    const float mult = seg_mult_lds(so, sr, n_seg, 4 * i) * wd;
    float4 ns, nd;
#define E2_ADADELTA1(k)                                                  \
    ns.k = mom * sv.k + (1.f - mom) * gv.k * gv.k;                       \
    {                                                                    \
      const float dir = gv.k * sqrtf(dv.k + E2_EPS_ADAM) / sqrtf(sv.k + E2_EPS_ADAM); \
      nd.k = mom * dv.k + (1.f - mom) * dir * dir;                       \
      pv.k = pv.k - lr * (mult != 0.f ? dir + mult * pv.k : dir);        \
    }
    E2_ADADELTA1(x) E2_ADADELTA1(y) E2_ADADELTA1(z) E2_ADADELTA1(w)
#undef E2_ADADELTA1
    s4[i] = ns; d4[i] = nd; p4[i] = pv;
  }
  if (blockIdx.x == 0)
    for (size_t i = 4 * n4 + threadIdx.x; i < n; i += blockDim.x) {
      const float gi = g[i] * gs;
      if (zero_g) g[i] = 0.f;
      const float si = s[i], di = d[i], pi = p[i];
      const float dir = gi * sqrtf(di + E2_EPS_ADAM) / sqrtf(si + E2_EPS_ADAM);
      const float mult = seg_mult_lds(so, sr, n_seg, i) * wd;
      s[i] = mom * si + (1.f - mom) * gi * gi;
      d[i] = mom * di + (1.f - mom) * dir * dir;
      p[i] = pi - lr * (mult != 0.f ? dir + mult * pi : dir);
    }
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
  E2_REQUIRE(ctx && p && g && m && s && seg_off && seg_reg && hyper && n_seg > 0,
             "adam_step: null argument");
  E2_REQUIRE(n_seg <= kOptMaxSeg, "adam_step: %d parameter tensors (at most %d)", n_seg, kOptMaxSeg);
  E2_REQUIRE((((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)s) & 15) == 0,
             "adam_step: arenas must be 16-byte aligned");
  const int grid = (int)std::min<size_t>(std::max<size_t>((n / 4 + 255) / 256, 1), ctx->num_cu);
  hipLaunchKernelGGL(adam_kernel, dim3(grid), dim3(256), 0, ctx->stream, p, g, m, s, n,
                     seg_off, seg_reg, n_seg, const_cast<float*>(hyper), gdiv, gmul, zero_g ? 1 : 0);
  E2_CHECK_HIP(hipGetLastError());
  return 0;
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
  E2_REQUIRE(ctx && p && g && d && seg_off && seg_reg && hyper && n_seg > 0,
             "sgd_step: null argument");
  E2_REQUIRE(n_seg <= kOptMaxSeg, "sgd_step: %d parameter tensors (at most %d)", n_seg, kOptMaxSeg);
  E2_REQUIRE((((uintptr_t)p | (uintptr_t)g | (uintptr_t)d) & 15) == 0, "sgd_step: arenas must be 16-byte aligned");
  const int grid = (int)std::min<size_t>(std::max<size_t>((n / 4 + 255) / 256, 1), 2 * (size_t)ctx->num_cu);
  hipLaunchKernelGGL(sgd_kernel, dim3(grid), dim3(256), 0, ctx->stream, p, g, d, n, seg_off,
                     seg_reg, n_seg, hyper, gdiv, gmul, zero_g ? 1 : 0);
  E2_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" int e2_adagrad_step_ex(e2_ctx* ctx, float* p, float* g, float* h, size_t n,
                                  const int64_t* seg_off, const float* seg_reg, int n_seg,
                                  const float* hyper, const float* gdiv, float gmul, int zero_g) {
  E2_REQUIRE(ctx && p && g && h && seg_off && seg_reg && hyper && n_seg > 0,
             "adagrad_step: null argument");
  E2_REQUIRE(n_seg <= kOptMaxSeg, "adagrad_step: %d parameter tensors (at most %d)", n_seg, kOptMaxSeg);
  E2_REQUIRE((((uintptr_t)p | (uintptr_t)g | (uintptr_t)h) & 15) == 0,
             "adagrad_step: arenas must be 16-byte aligned");
  // (at most one work-group per CU: the arrival counter, as e2_adam_step_ex)
  const int grid = (int)std::min<size_t>(std::max<size_t>((n / 4 + 255) / 256, 1), ctx->num_cu);
  hipLaunchKernelGGL(adagrad_kernel, dim3(grid), dim3(256), 0, ctx->stream, p, g, h, n, seg_off,
                     seg_reg, n_seg, const_cast<float*>(hyper), gdiv, gmul, zero_g ? 1 : 0);
  E2_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" int e2_adadelta_step_ex(e2_ctx* ctx, float* p, float* g, float* s, float* d, size_t n,
                                   const int64_t* seg_off, const float* seg_reg, int n_seg,
                                   const float* hyper, const float* gdiv, float gmul, int zero_g) {
  E2_REQUIRE(ctx && p && g && s && d && seg_off && seg_reg && hyper && n_seg > 0,
             "adadelta_step: null argument");
  E2_REQUIRE(n_seg <= kOptMaxSeg, "adadelta_step: %d parameter tensors (at most %d)", n_seg, kOptMaxSeg);
  E2_REQUIRE((((uintptr_t)p | (uintptr_t)g | (uintptr_t)s | (uintptr_t)d) & 15) == 0,
             "adadelta_step: arenas must be 16-byte aligned");
  const int grid = (int)std::min<size_t>(std::max<size_t>((n / 4 + 255) / 256, 1), 2 * (size_t)ctx->num_cu);
  hipLaunchKernelGGL(adadelta_kernel, dim3(grid), dim3(256), 0, ctx->stream, p, g, s, d, n, seg_off,
                     seg_reg, n_seg, hyper, gdiv, gmul, zero_g ? 1 : 0);
  E2_CHECK_HIP(hipGetLastError());
  return 0;
}
