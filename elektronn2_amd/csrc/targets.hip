// targets.hip -- the target forms of the batch creator, made on the device from the target patch
// that already lies in HBM (data/cnndata.py:319-396, data/image.py:80-102 and :138-220):
//
//   e2_target_stride    dst = t[..., ::sz, ::sx, ::sy], NaN -> -666
//   e2_target_nhood     make_nhood_targets on the full-resolution patch, then the stride, NaN -> -666
//   e2_target_affinity  seg_to_affgraph of rint(strided channel 0): 0 / 1 per edge
//   e2_count_negative   count[0] += #{t < 0}
//   e2_ids2barriers     ids2barriers(smoothen=False) of one ID volume, as a gather
//
// All are latency-bound streams over 1e5..1e6 voxels; what they replace is a device-to-host copy
// and a device sync per batch, not bandwidth.  The quad geometry is that of act.hip / pool.hip: a
// thread owns FOUR consecutive output x of one row and stores them as one 16-byte access where the
// destination row piece is 16-byte aligned, element by element at row ends and on misaligned
// views.  A source quad is one 16-byte load where the y stride is 1 and the piece lies inside its
// row and is aligned, single loads otherwise (a strided or shifted read has no neighbours to
// share a line with).  Nothing outside a view is read or written.  In the nhood and affinity
// kernels a thread loads its centre quad once and loops over the E edges, whose displacements sit
// in the kernel parameters (wave-uniform reads).
#include "stream_common.hpp"

namespace {

constexpr int kMaxEdges = 64;
typedef float tg_f4 __attribute__((ext_vector_type(4)));

// output geometry and the full-resolution source, shared by the three target kernels
struct TgtG {
  const float* t;
  float* o;
  long tn, tc, td, th;          // source strides (w stride 1)
  long on, oc, od, oh;          // destination strides
  int C, D, H, W;               // source extents
  int d, h, w;                  // destination extents = ceil(source / stride)
  int sz, sx, sy;               // the stride on (d, h, w)
  unsigned quads, items, chunk; // ceil(w / 4); d * h * quads (< 2^31); items per work-group
  FastDiv dq, dh;
};
struct TgtE {
  TgtG g;
  int E;
  int off[kMaxEdges * 3];
};

__device__ __forceinline__ float nan666(float v) { return v != v ? -666.f : v; }

// four source values at x = x0, x0 + step, ... of one row of W elements; `fill` where x is outside
__device__ __forceinline__ tg_f4 ld_quad(const float* row, int x0, int step, int W, float fill) {
  if (step == 1 && x0 >= 0 && x0 + 4 <= W && (((uintptr_t)(row + x0)) & 15) == 0)
    return *reinterpret_cast<const tg_f4*>(row + x0);
  tg_f4 v;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int x = x0 + k * step;
    v[k] = (x >= 0 && x < W) ? row[x] : fill;
  }
  return v;
}
// the first nv (1..4) of them to dst
__device__ __forceinline__ void st_quad(float* dst, tg_f4 v, unsigned nv) {
  if (nv == 4u && (((uintptr_t)dst) & 15) == 0) {
    *reinterpret_cast<tg_f4*>(dst) = v;
  } else {
    for (unsigned k = 0; k < nv; ++k) dst[k] = v[k];
  }
}
__device__ __forceinline__ tg_f4 nan666(tg_f4 v) {
  tg_f4 r;
  r[0] = nan666(v[0]); r[1] = nan666(v[1]); r[2] = nan666(v[2]); r[3] = nan666(v[3]);
  return r;
}

// item s of a plane -> output row (z, y) and first x of the quad
__device__ __forceinline__ void item_pos(const TgtG& p, unsigned s, int& z, int& y, int& x0) {
  const unsigned row = fdiv(s, p.dq);
  x0 = (int)((s - row * p.quads) << 2);
  z = (int)fdiv(row, p.dh);
  y = (int)(row - (unsigned)z * (unsigned)p.h);
}

// grid (chunks, C, n)
__global__ __launch_bounds__(256) void e2tgt_stride_kernel(TgtG p) {
  const unsigned s0 = blockIdx.x * p.chunk, s1 = min(s0 + p.chunk, p.items);
  const float* tb = p.t + (long)blockIdx.z * p.tn + (long)blockIdx.y * p.tc;
  float* ob = p.o + (long)blockIdx.z * p.on + (long)blockIdx.y * p.oc;
  for (unsigned s = s0 + threadIdx.x; s < s1; s += 256) {
    int z, y, x0;
    item_pos(p, s, z, y, x0);
    const float* row = tb + (long)z * p.sz * p.td + (long)y * p.sx * p.th;
    const tg_f4 v = nan666(ld_quad(row, x0 * p.sy, p.sy, p.W, 0.f));
    st_quad(ob + (long)z * p.od + (long)y * p.oh + x0, v, min(4u, (unsigned)(p.w - x0)));
  }
}

// grid (chunks, 1, n): channel e < E = channel 0 read at p * s - off_e (-1 outside), channels E.. =
// the strided channels 1..
__global__ __launch_bounds__(256) void e2tgt_nhood_kernel(TgtE a) {
  const TgtG& p = a.g;
  const unsigned s0 = blockIdx.x * p.chunk, s1 = min(s0 + p.chunk, p.items);
  const float* tb = p.t + (long)blockIdx.z * p.tn;
  float* ob = p.o + (long)blockIdx.z * p.on;
  for (unsigned s = s0 + threadIdx.x; s < s1; s += 256) {
    int z, y, x0;
    item_pos(p, s, z, y, x0);
    const int cz = z * p.sz, cy = y * p.sx, cx = x0 * p.sy;
    const unsigned nv = min(4u, (unsigned)(p.w - x0));
    float* dst = ob + (long)z * p.od + (long)y * p.oh + x0;
    const tg_f4 ctr = nan666(ld_quad(tb + (long)cz * p.td + (long)cy * p.th, cx, p.sy, p.W, -1.f));
    for (int e = 0; e < a.E; ++e) {
      const int oz = a.off[3 * e], oy = a.off[3 * e + 1], ox = a.off[3 * e + 2];
      tg_f4 v = ctr;
      if ((oz | oy | ox) != 0) {
        const int qz = cz - oz, qy = cy - oy;
        if (qz < 0 || qz >= p.D || qy < 0 || qy >= p.H) {
          v[0] = -1.f; v[1] = -1.f; v[2] = -1.f; v[3] = -1.f;
        } else {
          v = nan666(ld_quad(tb + (long)qz * p.td + (long)qy * p.th, cx - ox, p.sy, p.W, -1.f));
        }
      }
      st_quad(dst + (long)e * p.oc, v, nv);
    }
    for (int c = 1; c < p.C; ++c) {
      const float* row = tb + (long)c * p.tc + (long)cz * p.td + (long)cy * p.th;
      st_quad(dst + (long)(a.E + c - 1) * p.oc, nan666(ld_quad(row, cx, p.sy, p.W, 0.f)), nv);
    }
  }
}

__device__ __forceinline__ float same_id(float a, float b) {
  return (a == b && a > 0.f && b > 0.f) ? 1.f : 0.f;      // (NaN compares false)
}

// grid (chunks, 1, n): the edge p -> p + off_e of the STRIDED channel 0
__global__ __launch_bounds__(256) void e2tgt_affinity_kernel(TgtE a) {
  const TgtG& p = a.g;
  const unsigned s0 = blockIdx.x * p.chunk, s1 = min(s0 + p.chunk, p.items);
  const float* tb = p.t + (long)blockIdx.z * p.tn;
  float* ob = p.o + (long)blockIdx.z * p.on;
  for (unsigned s = s0 + threadIdx.x; s < s1; s += 256) {
    int z, y, x0;
    item_pos(p, s, z, y, x0);
    const unsigned nv = min(4u, (unsigned)(p.w - x0));
    float* dst = ob + (long)z * p.od + (long)y * p.oh + x0;
    tg_f4 c = ld_quad(tb + (long)z * p.sz * p.td + (long)y * p.sx * p.th, x0 * p.sy, p.sy, p.W, 0.f);
    c[0] = rintf(c[0]); c[1] = rintf(c[1]); c[2] = rintf(c[2]); c[3] = rintf(c[3]);
    for (int e = 0; e < a.E; ++e) {
      const int pz = z + a.off[3 * e], py = y + a.off[3 * e + 1], px = x0 + a.off[3 * e + 2];
      tg_f4 r;
      r[0] = 0.f; r[1] = 0.f; r[2] = 0.f; r[3] = 0.f;
      if (pz >= 0 && pz < p.d && py >= 0 && py < p.h) {
        // (x * sy < W  <=>  x < w = ceil(W / sy): the row's own bound is the strided one; the id 0
        // outside connects to nothing)
        const tg_f4 b = ld_quad(tb + (long)pz * p.sz * p.td + (long)py * p.sx * p.th, px * p.sy,
                                p.sy, p.W, 0.f);
        r[0] = same_id(c[0], rintf(b[0]));
        r[1] = same_id(c[1], rintf(b[1]));
        r[2] = same_id(c[2], rintf(b[2]));
        r[3] = same_id(c[3], rintf(b[3]));
      }
      st_quad(dst + (long)e * p.oc, r, nv);
    }
  }
}

__device__ __forceinline__ unsigned wave_sum_u(unsigned v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += (unsigned)__shfl_down((int)v, o, 64);
  return v;
}

// grid (chunks, C, n); TgtG with stride 1 and o unused: one integer atomic per work-group
__global__ __launch_bounds__(256) void e2tgt_count_negative_kernel(TgtG p, unsigned* count) {
  __shared__ unsigned red[4];
  const unsigned s0 = blockIdx.x * p.chunk, s1 = min(s0 + p.chunk, p.items);
  const float* tb = p.t + (long)blockIdx.z * p.tn + (long)blockIdx.y * p.tc;
  unsigned cnt = 0;
  for (unsigned s = s0 + threadIdx.x; s < s1; s += 256) {
    int z, y, x0;
    item_pos(p, s, z, y, x0);
    const tg_f4 v = ld_quad(tb + (long)z * p.td + (long)y * p.th, x0, 1, p.W, 0.f);
    cnt += (v[0] < 0.f) + (v[1] < 0.f) + (v[2] < 0.f) + (v[3] < 0.f);
  }
  cnt = wave_sum_u(cnt);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned tot = (red[0] + red[1]) + (red[2] + red[3]);
    if (tot != 0u) atomicAdd(count, tot);
  }
}

// ids2barriers as a gather.  The reference's forward pass visits the cells whose three coordinates
// are all below n - 1 and, per connected axis a, marks both ends of a differing edge (c, c + e_a)
// and, diluted, c - e_a and c + 2 e_a where they exist; the pass on the fully reversed volume is the
// same over the cells whose coordinates are all above 0, looking down.  Both mark the same four
// voxels around an edge, so: voxel v is a barrier through axis a iff one of the edges
// (v-2,v-1), (v-1,v), (v,v+1), (v+1,v+2) along a exists and differs (the outer two only when
// diluted) AND v's other two coordinates are all <= n - 2 (forward) or all >= 1 (reversed).
struct BarrP {
  TgtG g;                       // source = ids, C = 1, stride 1
  int conn[3], dil[3];
  int ecs;
};

__device__ __forceinline__ bool barr_axis(const float* at, long st, int v, int n, bool dilute) {
  // at = &ids[v] along an axis of stride st and extent n
  const int k0 = dilute ? -2 : -1, k1 = dilute ? 1 : 0;
  bool m = false;
  for (int k = k0; k <= k1; ++k) {
    const int lo = v + k;                                   // edge (lo, lo + 1)
    if (lo >= 0 && lo + 1 < n) m = m || (at[(long)k * st] != at[(long)(k + 1) * st]);
  }
  return m;
}

__global__ __launch_bounds__(256) void e2tgt_barriers_kernel(BarrP a) {
  const TgtG& p = a.g;
  const unsigned s0 = blockIdx.x * p.chunk, s1 = min(s0 + p.chunk, p.items);
  for (unsigned s = s0 + threadIdx.x; s < s1; s += 256) {
    int z, y, x0;
    item_pos(p, s, z, y, x0);
    const unsigned nv = min(4u, (unsigned)(p.w - x0));
    const float* row = p.t + (long)z * p.td + (long)y * p.th;
    const bool zf = z <= p.D - 2, zr = z >= 1, yf = y <= p.H - 2, yr = y >= 1;
    tg_f4 r;
    r[0] = 0.f; r[1] = 0.f; r[2] = 0.f; r[3] = 0.f;
    for (unsigned k = 0; k < nv; ++k) {
      const int x = x0 + (int)k;
      const float* at = row + x;
      const bool xf = x <= p.W - 2, xr = x >= 1;
      bool m = false;
      if (a.conn[0] && ((yf && xf) || (yr && xr))) m = m || barr_axis(at, p.td, z, p.D, a.dil[0] != 0);
      if (a.conn[1] && ((zf && xf) || (zr && xr))) m = m || barr_axis(at, p.th, y, p.H, a.dil[1] != 0);
      if (a.conn[2] && ((zf && yf) || (zr && yr))) m = m || barr_axis(at, 1, x, p.W, a.dil[2] != 0);
      float b = m ? 1.f : 0.f;
      if (a.ecs != 0 && !m && *at == 0.f) b = a.ecs == 1 ? 1.f : 2.f;
      r[k] = b;
    }
    st_quad(p.o + (long)z * p.od + (long)y * p.oh + x0, r, nv);
  }
}

int tgt_stride_arg(const int* stride, const char* who, int s[3]) {
  E2_REQUIRE(stride, "%s: null stride", who);
  for (int k = 0; k < 3; ++k) {
    E2_REQUIRE(stride[k] >= 1, "%s: stride %d on axis %d (>= 1)", who, stride[k], k);
    s[k] = stride[k];
  }
  return 0;
}

// t (any C) strided by s must give dst's extents; fills the geometry and the grid's x
int tgt_geometry(e2_ctx* ctx, const e2_tensor5* t, const int s[3], const e2_tensor5* dst,
                 unsigned long long planes, TgtG& p, unsigned& gx, const char* who) {
  if (int rc = check_view(t, who)) return rc;
  if (dst) {
    if (int rc = check_view(dst, who)) return rc;
    E2_REQUIRE(dst->n == t->n && dst->d == e2_cdiv(t->d, s[0]) && dst->h == e2_cdiv(t->h, s[1]) &&
                   dst->w == e2_cdiv(t->w, s[2]),
               "%s: dst (%d,.,%d,%d,%d) is not t (%d,.,%d,%d,%d) strided by (%d,%d,%d)", who, dst->n,
               dst->d, dst->h, dst->w, t->n, t->d, t->h, t->w, s[0], s[1], s[2]);
  }
  p = TgtG{};
  p.t = t->ptr; p.tn = (long)t->sn; p.tc = (long)t->sc; p.td = (long)t->sd; p.th = (long)t->sh;
  p.C = t->c; p.D = t->d; p.H = t->h; p.W = t->w;
  p.d = e2_cdiv(t->d, s[0]); p.h = e2_cdiv(t->h, s[1]); p.w = e2_cdiv(t->w, s[2]);
  p.sz = s[0]; p.sx = s[1]; p.sy = s[2];
  if (dst) {
    p.o = dst->ptr; p.on = (long)dst->sn; p.oc = (long)dst->sc; p.od = (long)dst->sd;
    p.oh = (long)dst->sh;
  }
  const unsigned long long quads = ((unsigned long long)p.w + 3) / 4;
  const unsigned long long items = (unsigned long long)p.d * p.h * quads;
  E2_REQUIRE(items < (1ull << 31), "%s: target too large", who);
  p.quads = (unsigned)quads; p.items = (unsigned)items;
  p.dq = mk_div(p.quads); p.dh = mk_div((unsigned)p.h);
  p.chunk = stream_chunk(ctx, planes, items, 4, 8);
  gx = (unsigned)((items + p.chunk - 1) / p.chunk);
  return 0;
}

int tgt_edges(const int* nhood, int E, const char* who, TgtE& a) {
  E2_REQUIRE(nhood, "%s: null nhood", who);
  E2_REQUIRE(E >= 1 && E <= kMaxEdges, "%s: %d edges (1..%d)", who, E, kMaxEdges);
  a = TgtE{};
  a.E = E;
  for (int k = 0; k < 3 * E; ++k) a.off[k] = nhood[k];
  return 0;
}

}  // namespace

extern "C" int e2_target_stride(e2_ctx* ctx, const e2_tensor5* t, const int* stride,
                                const e2_tensor5* dst) {
  E2_REQUIRE(ctx && t && dst, "e2_target_stride: null argument");
  int s[3];
  if (int rc = tgt_stride_arg(stride, "e2_target_stride", s)) return rc;
  TgtG p;
  unsigned gx;
  if (int rc = tgt_geometry(ctx, t, s, dst, (unsigned long long)t->n * t->c, p, gx,
                            "e2_target_stride"))
    return rc;
  E2_REQUIRE(dst->c == t->c, "e2_target_stride: %d features into %d", t->c, dst->c);
  hipLaunchKernelGGL(e2tgt_stride_kernel, dim3(gx, (unsigned)t->c, (unsigned)t->n), dim3(256), 0,
                     ctx->stream, p);
  E2_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" int e2_target_nhood(e2_ctx* ctx, const e2_tensor5* t, const int* nhood, int E,
                               const int* stride, const e2_tensor5* dst) {
  E2_REQUIRE(ctx && t && dst, "e2_target_nhood: null argument");
  int s[3];
  if (int rc = tgt_stride_arg(stride, "e2_target_nhood", s)) return rc;
  TgtE a;
  if (int rc = tgt_edges(nhood, E, "e2_target_nhood", a)) return rc;
  unsigned gx;
  if (int rc = tgt_geometry(ctx, t, s, dst, (unsigned long long)t->n, a.g, gx, "e2_target_nhood"))
    return rc;
  E2_REQUIRE(dst->c == E + t->c - 1, "e2_target_nhood: dst has %d features, E + C - 1 = %d", dst->c,
             E + t->c - 1);
  const int ext[3] = {t->d, t->h, t->w};
  for (int e = 0; e < E; ++e)
    for (int k = 0; k < 3; ++k)
      E2_REQUIRE(abs(nhood[3 * e + k]) < ext[k],
                 "e2_target_nhood: edge %d moves %d along axis %d of extent %d", e, nhood[3 * e + k],
                 k, ext[k]);
  hipLaunchKernelGGL(e2tgt_nhood_kernel, dim3(gx, 1, (unsigned)t->n), dim3(256), 0, ctx->stream, a);
  E2_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" int e2_target_affinity(e2_ctx* ctx, const e2_tensor5* t, const int* nhood, int E,
                                  const int* stride, const e2_tensor5* dst) {
  E2_REQUIRE(ctx && t && dst, "e2_target_affinity: null argument");
  int s[3];
  if (int rc = tgt_stride_arg(stride, "e2_target_affinity", s)) return rc;
  TgtE a;
  if (int rc = tgt_edges(nhood, E, "e2_target_affinity", a)) return rc;
  unsigned gx;
  if (int rc = tgt_geometry(ctx, t, s, dst, (unsigned long long)t->n, a.g, gx, "e2_target_affinity"))
    return rc;
  E2_REQUIRE(dst->c == E, "e2_target_affinity: dst has %d features for %d edges", dst->c, E);
  for (int k = 0; k < 3 * E; ++k)       // (p + off in int, times the stride in int)
    E2_REQUIRE(abs(nhood[k]) < (1 << 20), "e2_target_affinity: displacement %d", nhood[k]);
  hipLaunchKernelGGL(e2tgt_affinity_kernel, dim3(gx, 1, (unsigned)t->n), dim3(256), 0, ctx->stream,
                     a);
  E2_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" int e2_count_negative(e2_ctx* ctx, const e2_tensor5* t, unsigned* count) {
  E2_REQUIRE(ctx && t && count, "e2_count_negative: null argument");
  const int s[3] = {1, 1, 1};
  TgtG p;
  unsigned gx;
  if (int rc = tgt_geometry(ctx, t, s, nullptr, (unsigned long long)t->n * t->c, p, gx,
                            "e2_count_negative"))
    return rc;
  E2_REQUIRE((unsigned long long)t->n * t->c * t->d * t->h * t->w < (1ull << 32),
             "e2_count_negative: more than 2^32 elements");
  hipLaunchKernelGGL(e2tgt_count_negative_kernel, dim3(gx, (unsigned)t->c, (unsigned)t->n),
                     dim3(256), 0, ctx->stream, p, count);
  E2_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" int e2_ids2barriers(e2_ctx* ctx, const e2_tensor5* ids, const int* dilute,
                               const int* connectivity, int ecs_mode, const e2_tensor5* dst) {
  E2_REQUIRE(ctx && ids && dst && dilute && connectivity, "e2_ids2barriers: null argument");
  E2_REQUIRE(ecs_mode >= 0 && ecs_mode <= 2, "e2_ids2barriers: ecs_mode %d (0, 1, 2)", ecs_mode);
  const int s[3] = {1, 1, 1};
  BarrP a;
  unsigned gx;
  if (int rc = tgt_geometry(ctx, ids, s, dst, 1, a.g, gx, "e2_ids2barriers")) return rc;
  E2_REQUIRE(ids->n == 1 && ids->c == 1 && dst->c == 1, "e2_ids2barriers: ids and dst are (1,1,D,H,W)");
  for (int k = 0; k < 3; ++k) { a.conn[k] = connectivity[k] != 0; a.dil[k] = dilute[k] != 0; }
  a.ecs = ecs_mode;
  hipLaunchKernelGGL(e2tgt_barriers_kernel, dim3(gx, 1, 1), dim3(256), 0, ctx->stream, a);
  E2_CHECK_HIP(hipGetLastError());
  return 0;
}
