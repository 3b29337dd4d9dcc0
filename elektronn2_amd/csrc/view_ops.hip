// view_ops.hip -- fills and copies of strided 5-D views, the NCDHW<->NDHWC transposes through LDS,
// and the prologue of a captured step (batch ring, loss history).  One-element-per-lane,
// W-contiguous (coalesced) streaming kernels.
#include "stream_common.hpp"
#include <algorithm>

// ---------------------------------------------------------------------------
// fill / copy
// ---------------------------------------------------------------------------
// (32-bit index math with magic-number division: 64-bit % and / made these ALU-bound)
__global__ void fill_view_kernel(View5 v, float val, FastDiv dw, FastDiv dh) {
  // grid: (ceil(d*h*w/256), c, n)
  const unsigned S = (unsigned)v.d * v.h * v.w;
  const unsigned s = blockIdx.x * 256u + threadIdx.x;
  if (s >= S) return;
  const unsigned t = fdiv(s, dw);
  const unsigned x = s - t * v.w;
  const unsigned z = fdiv(t, dh);
  const unsigned y = t - z * v.h;
  v.p[vidx(v, blockIdx.z, blockIdx.y, (int)z, (int)y, (int)x)] = val;
}

__global__ void copy_view_kernel(View5 src, View5 dst, int accumulate, FastDiv dw, FastDiv dh) {
  const unsigned S = (unsigned)src.d * src.h * src.w;
  const unsigned s = blockIdx.x * 256u + threadIdx.x;
  if (s >= S) return;
  const unsigned t = fdiv(s, dw);
  const unsigned x = s - t * src.w;
  const unsigned z = fdiv(t, dh);
  const unsigned y = t - z * src.h;
  const float v = src.p[vidx(src, blockIdx.z, blockIdx.y, (int)z, (int)y, (int)x)];
  float* d = dst.p + vidx(dst, blockIdx.z, blockIdx.y, (int)z, (int)y, (int)x);
  *d = accumulate ? (*d + v) : v;
}

// ---------------------------------------------------------------------------
// transposes through a 32x33 LDS tile:  [C][S] <-> [S][C]
// ---------------------------------------------------------------------------
__global__ void ncdhw_to_ndhwc_kernel(View5 src, float* __restrict__ dst) {
  __shared__ float tile[32][33];
  const long S = (long)src.d * src.h * src.w;
  const int n = blockIdx.z;
  const long s0 = blockIdx.x * 32L;
  const int c0 = blockIdx.y * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;   // 32 x 8
  for (int i = ty; i < 32; i += 8) {
    const int c = c0 + i;
    const long s = s0 + tx;
    float v = 0.f;
    if (c < src.c && s < S) {
      const int x = (int)(s % src.w);
      const long t = s / src.w;
      v = src.p[vidx(src, n, c, (int)(t / src.h), (int)(t % src.h), x)];
    }
    tile[i][tx] = v;
  }
  __syncthreads();
  for (int i = ty; i < 32; i += 8) {
    const long s = s0 + i;
    const int c = c0 + tx;
    if (c < src.c && s < S) dst[((long)n * S + s) * src.c + c] = tile[tx][i];
  }
}

__global__ void ndhwc_to_ncdhw_kernel(const float* __restrict__ src, View5 dst) {
  __shared__ float tile[32][33];
  const long S = (long)dst.d * dst.h * dst.w;
  const int n = blockIdx.z;
  const long s0 = blockIdx.x * 32L;
  const int c0 = blockIdx.y * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  for (int i = ty; i < 32; i += 8) {
    const long s = s0 + i;
    const int c = c0 + tx;
    float v = 0.f;
    if (c < dst.c && s < S) v = src[((long)n * S + s) * dst.c + c];
    tile[i][tx] = v;
  }
  __syncthreads();
  for (int i = ty; i < 32; i += 8) {
    const int c = c0 + i;
    const long s = s0 + tx;
    if (c < dst.c && s < S) {
      const int x = (int)(s % dst.w);
      const long t = s / dst.w;
      dst.p[vidx(dst, n, c, (int)(t / dst.h), (int)(t % dst.h), x)] = tile[tx][i];
    }
  }
}

static dim3 grid_for(const View5& v) {
  const long S = (long)v.d * v.h * v.w;
  return dim3((unsigned)((S + 255) / 256), (unsigned)v.c, (unsigned)v.n);
}

int e2i_fill_view(e2_ctx* ctx, const e2_tensor5* t, float value) {
  if (int rc = check_view(t, "fill_view")) return rc;
  View5 v = mk(t);
  E2_REQUIRE((long)v.d * v.h * v.w < (1L << 31), "fill_view: channel too large");
  hipLaunchKernelGGL(fill_view_kernel, grid_for(v), dim3(256), 0, ctx->stream, v, value,
                     mk_div(v.w), mk_div(v.h));
  E2_CHECK_HIP(hipGetLastError());
  return 0;
}

// ---- several steps in one graph: the batches come out of a ring in HBM, the losses go into one ----
// A captured step is the same launches every time; what changes from step to step are the batch
// and the loss.  Both become position-independent through a launch COUNT kept in device memory:
// launch number L of the prologue reads slot L % n of the batch ring and stores the loss the
// PREVIOUS step left behind in slot (L - 1) % n of the history.  The count is read with plain
// loads (it was written by the previous launch) and advanced by the work-group that arrives last
// at the end of the launch -- no load of the copy waits for an atomic.  So the SAME captured step
// can stand k times in one graph (DESIGN finding 55).
struct PrologueP {
  const float* ring; int nSlots; long slotFloats; float* dst;
  const float* src; int nVals; float* hist; int histSlots;
  unsigned long long* state;           // [0] launches so far, [1] arrivals of the running launch
};
__global__ __launch_bounds__(256) void step_prologue_kernel(PrologueP p) {
  const unsigned long long L = *(volatile unsigned long long*)p.state;
  if (p.hist && L > 0 && blockIdx.x == 0) {
    float* d = p.hist + (long)((L - 1) % (unsigned long long)p.histSlots) * p.nVals;
    for (int i = threadIdx.x; i < p.nVals; i += 256) d[i] = p.src[i];
  }
  if (p.ring) {
    const float* src = p.ring + (long)(L % (unsigned long long)p.nSlots) * p.slotFloats;
    const long n4 = p.slotFloats >> 2;
    const float4* s4 = reinterpret_cast<const float4*>(src);
    float4* d4 = reinterpret_cast<float4*>(p.dst);
    const long stride = gridDim.x * 256L;
    long i = blockIdx.x * 256L + threadIdx.x;
    for (; i + 3 * stride < n4; i += 4 * stride) {       // four 16-byte loads in flight per lane
      const float4 a = s4[i], b = s4[i + stride], c = s4[i + 2 * stride], d = s4[i + 3 * stride];
      d4[i] = a; d4[i + stride] = b; d4[i + 2 * stride] = c; d4[i + 3 * stride] = d;
    }
    for (; i < n4; i += stride) d4[i] = s4[i];
    if (blockIdx.x == 0 && threadIdx.x < (p.slotFloats & 3)) p.dst[4 * n4 + threadIdx.x] = src[4 * n4 + threadIdx.x];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    if (atomicAdd(p.state + 1, 1ull) == (unsigned long long)gridDim.x - 1) {
      p.state[1] = 0;                  // (every work-group of this launch has read state[0] by now)
      p.state[0] = L + 1;
    }
  }
}

/* The first launch of a captured step that may stand several times in one graph:
 *   dst[0 .. slot_floats) = ring[L % n_slots]              (ring != NULL)
 *   hist[(L - 1) % hist_slots][0 .. n_vals) = src[..]       (hist != NULL and L > 0: what the step
 *                                                            BEFORE this one left in src, its loss)
 * with L = the number of prologue launches on `state` so far; state: two zeroed 64-bit words in
 * device memory owned by the caller ([0] = L, readable by the host after a synchronisation).
 * ring, dst 16-byte aligned, slot_floats a multiple of 4.  Launches on one `state` must be
 * ordered (one stream). */
extern "C" int e2_step_prologue(e2_ctx* ctx, const float* ring, int n_slots, size_t slot_floats,
                                float* dst, const float* src, int n_vals, float* hist,
                                int hist_slots, void* state) {
  E2_REQUIRE(ctx && state && ((uintptr_t)state & 7) == 0, "e2_step_prologue: null / misaligned state");
  E2_REQUIRE(!ring || (dst && n_slots > 0 && slot_floats > 0 &&
                       (((uintptr_t)ring | (uintptr_t)dst) & 15) == 0 && ((slot_floats * 4) & 15) == 0),
             "e2_step_prologue: ring / dst must be 16-byte aligned and slots a multiple of 16 bytes");
  E2_REQUIRE(!hist || (src && n_vals > 0 && hist_slots > 0), "e2_step_prologue: bad history arguments");
  PrologueP p;
  p.ring = ring; p.nSlots = n_slots; p.slotFloats = (long)slot_floats; p.dst = dst;
  p.src = src; p.nVals = n_vals; p.hist = hist; p.histSlots = hist_slots;
  p.state = (unsigned long long*)state;
  const int grid = ring ? (int)std::min<size_t>(std::max<size_t>((slot_floats / 4 + 1023) / 1024, 1),
                                                (size_t)ctx->num_cu) : 1;
  hipLaunchKernelGGL(step_prologue_kernel, dim3(grid), dim3(256), 0, ctx->stream, p);
  E2_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" int e2_set_skip_zero_fill(e2_ctx* ctx, int on) {
  E2_REQUIRE(ctx, "e2_set_skip_zero_fill: null context");
  ctx->skip_zero_fill = on ? 1 : 0;
  return 0;
}

extern "C" int e2_conv_last_zero_fill(const e2_ctx* ctx, void** ptr, size_t* n) {
  E2_REQUIRE(ctx && ptr && n, "e2_conv_last_zero_fill: null argument");
  *ptr = ctx->last_fill_ptr;
  *n = ctx->last_fill_n;
  return 0;
}

extern "C" int e2_copy5(e2_ctx* ctx, const e2_tensor5* src, const e2_tensor5* dst,
                        int accumulate) {
  E2_REQUIRE(ctx, "e2_copy5: null ctx");
  if (int rc = check_view(src, "copy5 src")) return rc;
  if (int rc = check_view(dst, "copy5 dst")) return rc;
  E2_REQUIRE(same_size(src, dst), "e2_copy5: size mismatch");
  View5 s = mk(src), d = mk(dst);
  E2_REQUIRE((long)s.d * s.h * s.w < (1L << 31), "e2_copy5: channel too large");
  hipLaunchKernelGGL(copy_view_kernel, grid_for(s), dim3(256), 0, ctx->stream, s, d,
                     accumulate, mk_div(s.w), mk_div(s.h));
  E2_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" int e2_transpose_ncdhw_to_ndhwc(e2_ctx* ctx, const e2_tensor5* src, float* dst) {
  E2_REQUIRE(ctx && dst, "transpose: null argument");
  if (int rc = check_view(src, "transpose src")) return rc;
  View5 v = mk(src);
  const long S = (long)v.d * v.h * v.w;
  dim3 grid((unsigned)((S + 31) / 32), (unsigned)((v.c + 31) / 32), (unsigned)v.n);
  hipLaunchKernelGGL(ncdhw_to_ndhwc_kernel, grid, dim3(256), 0, ctx->stream, v, dst);
  E2_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" int e2_transpose_ndhwc_to_ncdhw(e2_ctx* ctx, const float* src,
                                           const e2_tensor5* dst) {
  E2_REQUIRE(ctx && src, "transpose: null argument");
  if (int rc = check_view(dst, "transpose dst")) return rc;
  View5 v = mk(dst);
  const long S = (long)v.d * v.h * v.w;
  dim3 grid((unsigned)((S + 31) / 32), (unsigned)((v.c + 31) / 32), (unsigned)v.n);
  hipLaunchKernelGGL(ndhwc_to_ncdhw_kernel, grid, dim3(256), 0, ctx->stream, src, v);
  E2_CHECK_HIP(hipGetLastError());
  return 0;
}
