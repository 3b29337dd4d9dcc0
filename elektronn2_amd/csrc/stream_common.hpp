// Helpers shared by the streaming (HBM-bound) kernels and their launchers: the strided 5-D view,
// the magic-number divider, the wave / work-group sums, the argument checks and the chunk sizing.
// One definition each, at global scope: View5 and FastDiv are kernel parameters, so their names are
// part of mangled kernel names.  A new op file includes this header; it does not copy from it.
// The device parts need hipcc; the host parts also compile with a plain C++ compiler
// (tests/test_stream_common_host.py).
#pragma once
#include "common.hpp"

struct View5 {
  float* p;
  int n, c, d, h, w;
  long sn, sc, sd, sh;
};
static inline View5 mk(const e2_tensor5* t) {
  return View5{t->ptr, t->n, t->c, t->d, t->h, t->w, (long)t->sn, (long)t->sc,
               (long)t->sd, (long)t->sh};
}

// exact unsigned division of n < 2^31 by a runtime constant (host-made magic):
// l = ceil(log2 d), m = ceil(2^(31+l) / d);  n / d == umulhi(n, m) >> (l - 1)
struct FastDiv {
  unsigned d, m, sh;
};
static inline FastDiv mk_div(unsigned d) {
  FastDiv f;
  f.d = d;
  if (d <= 1) { f.m = 0; f.sh = 0; return f; }
  unsigned l = 0;
  while ((1ull << l) < d) ++l;
  const unsigned long long num = 1ull << (31 + l);
  f.m = (unsigned)((num + d - 1) / d);
  f.sh = l - 1;
  return f;
}
// (one text for the device function and for the host function the test of the divider calls)
#ifdef __HIPCC__
#define E2_STREAM_DEVICE __device__ __forceinline__
#define E2_UMULHI(a, b) __umulhi(a, b)
#else
#define E2_STREAM_DEVICE static inline
#define E2_UMULHI(a, b) ((unsigned)(((uint64_t)(a) * (b)) >> 32))
#endif
E2_STREAM_DEVICE unsigned fdiv(unsigned n, const FastDiv& f) {
  return f.d <= 1 ? n : (E2_UMULHI(n, f.m) >> f.sh);
}

#ifdef __HIPCC__
__device__ __forceinline__ long vidx(const View5& v, int n, int c, int z, int y, int x) {
  return (long)n * v.sn + (long)c * v.sc + (long)z * v.sd + (long)y * v.sh + x;
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;
}
// sum over a 256-thread block; result valid in thread 0
__device__ __forceinline__ float block_sum256(float v, float* red) {
  v = wave_sum(v);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) red[wave] = v;
  __syncthreads();
  float r = 0.f;
  if (threadIdx.x == 0) r = red[0] + red[1] + red[2] + red[3];
  __syncthreads();
  return r;
}
#endif

static inline int check_view(const e2_tensor5* t, const char* name) {
  E2_REQUIRE(t && t->ptr, "%s: null tensor", name);
  E2_REQUIRE(t->n > 0 && t->c > 0 && t->d > 0 && t->h > 0 && t->w > 0,
             "%s: empty tensor (%d,%d,%d,%d,%d)", name, t->n, t->c, t->d, t->h, t->w);
  E2_REQUIRE(t->c < 65536 && t->n < 65536, "%s: n/c too large for grid", name);
  return 0;
}
// the same n, c, d, h, w
static inline bool same_size(const e2_tensor5* a, const e2_tensor5* b) {
  return a->n == b->n && a->c == b->c && a->d == b->d && a->h == b->h && a->w == b->w;
}
// the same n, d, h, w (any feature counts)
static inline bool same_extents(const e2_tensor5* a, const e2_tensor5* b) {
  return a->n == b->n && a->d == b->d && a->h == b->h && a->w == b->w;
}

// items per work-group of a grid (chunks of `items`, planes): 256 threads with up to per_max items
// each, fewer while the grid would not reach want_per_cu work-groups per CU
static inline unsigned stream_chunk(const e2_ctx* ctx, unsigned long long planes,
                                    unsigned long long items, unsigned per_max,
                                    unsigned want_per_cu) {
  const unsigned long long want =
      (unsigned long long)want_per_cu * (unsigned long long)(ctx->num_cu > 0 ? ctx->num_cu : 256);
  unsigned per = per_max;
  while (per > 1 && planes * ((items + 256ull * per - 1) / (256ull * per)) < want) per >>= 1;
  return 256u * per;
}
