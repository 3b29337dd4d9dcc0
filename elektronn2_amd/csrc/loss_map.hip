// loss_map.hip -- losses that make a one-feature MAP out of the feature axis, and the mean of such
// a map as a term of the element-wise mix (loss.py:1104-1151 EuclideanDistance, 1154-1212 RampLoss,
// 1346-1363 AggregateLoss).
//
//   e2_fdist_fwd   out[n,0,z,y,x] = sqrt(sum_f (target - pred)^2); a NaN result is stored as 0
//   e2_fdist_bwd   dpred[n,f,..] (=|+=) -(target - pred) / out * dout,  dtarget the negative
//   e2_ramp_fwd    out[n,0,..] = (1/F) sum_f r,  r = d_low - d_big + margin, r < 0 -> 0, NaN -> 0
//   e2_ramp_bwd    dd_low[n,f,..] (=|+=) dout / F where r >= 0 (a NaN r is not), else 0; dd_big the
//                  negative.  The reference masks r < 0 only: the slope AT r == 0 is 1.
//   e2_mean_fwd    slab rows (sum x, elements summed, 0, 0) of the row's work-group
//   e2_mean_bwd    dx (=|+=) coef[0] in every element
//   e2_onehot      out[n,k,..] = target[n,0,..] == k ? 1 : 0  (loss.py:96-138 OneHot, exact equality)
//
// Two stated departures from the reference's gradient in e2_fdist_bwd: where out == 0 (pred ==
// target over all features) T.grad of the norm is 0/0 = NaN; here every feature gets an exact 0.
// Where the forward replaced a NaN by 0, the same: an exact 0 in every feature.
//
// The mean of a map is one more term of e2_loss_mix, which does not change: the slab rows have the
// layout of e2_loss_fwd's -- (S1, n, S2, 0) per work-group, a plain 16-byte store, no atomics, as
// many rows as e2_loss_partials names for the map -- and the term is normalised by n_tot (a plain
// mean, no -666 mask), which is the GAUSS_NLL row of the mix: L = S1 / n_tot, coef = mix / (K n_tot).
// The caller hands e2_loss_mix a GAUSS_NLL-kind descriptor for such a term.
//
// Geometry as in act.hip / loss_elem.hip: a thread owns FOUR consecutive x of one row and moves
// them as one 16-byte access where that piece is 16-byte aligned in every view and every feature
// (the feature strides are part of the test), element by element at row ends and on misaligned
// views; the y and z axes are collapsed into the row on the host where they are dense in all
// views.  The feature axis is a loop INSIDE the thread: consecutive threads stay consecutive in x
// for every feature, so every load is coalesced.  All operands are strided e2_tensor5 views;
// nothing outside a view is read or written.  margin and coef are device scalars read when the
// kernel runs.  All arithmetic is f32.
#include "stream_common.hpp"

namespace {

typedef float map_f4 __attribute__((ext_vector_type(4)));

// strides of the (up to) three axes that stay outside the collapsed row, innermost first, and of
// the feature axis
struct MView {
  long s[3];
  long sc;
};

struct MapP {
  const float* a;               // pred / d_low / x
  const float* b;               // target / d_big
  const float* o;               // bwd: the forward's map (fdist)
  const float* g;               // bwd: the map's gradient
  float* out;                   // fwd: the map
  float* da;                    // bwd outputs; either may be null
  float* db;
  MView va, vb, vo, vg, vout, vda, vdb;
  unsigned w;                   // row length after the collapse
  unsigned quads;               // ceil(w / 4)
  unsigned items;               // rows * quads  (< 2^31)
  unsigned e0, e1;              // extents of the two inner outside axes
  unsigned F;                   // features of the F-feature operands
  unsigned fbits;               // OR of their feature strides in bytes (alignment test)
  FastDiv dq, d0, d1;
  const float* scalar;          // margin / coef: device scalar, read when the kernel runs
  float* partials;              // mean fwd: [gridDim.x][4]
};

struct MPos {
  unsigned i0, i1, i2, x0;
};
__device__ __forceinline__ MPos locate(const MapP& p, unsigned s) {
  MPos q;
  const unsigned row = fdiv(s, p.dq);
  q.x0 = (s - row * p.quads) << 2;
  const unsigned r1 = fdiv(row, p.d0);
  q.i0 = row - r1 * p.e0;
  q.i2 = fdiv(r1, p.d1);
  q.i1 = r1 - q.i2 * p.e1;
  return q;
}
__device__ __forceinline__ long voff(const MView& v, const MPos& q) {
  return (long)q.i0 * v.s[0] + (long)q.i1 * v.s[1] + (long)q.i2 * v.s[2] + (long)q.x0;
}
__device__ __forceinline__ map_f4 ld4(const float* p) {
  return *reinterpret_cast<const map_f4*>(p);
}
__device__ __forceinline__ void st4(float* p, map_f4 v, bool acc) {
  if (acc) v += *reinterpret_cast<const map_f4*>(p);
  *reinterpret_cast<map_f4*>(p) = v;
}
__device__ __forceinline__ bool whole(const MapP& p, const MPos& q, uintptr_t al) {
  return q.x0 + 4u <= p.w && ((al | (uintptr_t)p.fbits) & 15) == 0;
}

// ---- EuclideanDistance ---------------------------------------------------------------------
__device__ __forceinline__ float dist_of(float ss) {
  const float r = sqrtf(ss);
  return r != r ? 0.f : r;
}

__global__ __launch_bounds__(256) void e2map_fdist_fwd_kernel(MapP p) {
  const unsigned step = gridDim.x * 256u;
  for (unsigned s = blockIdx.x * 256u + threadIdx.x; s < p.items; s += step) {
    const MPos q = locate(p, s);
    const float* pa = p.a + voff(p.va, q);
    const float* pb = p.b + voff(p.vb, q);
    float* po = p.out + voff(p.vout, q);
    if (whole(p, q, ((uintptr_t)pa) | ((uintptr_t)pb) | ((uintptr_t)po))) {
      map_f4 ss = {0.f, 0.f, 0.f, 0.f};
      for (unsigned f = 0; f < p.F; ++f) {
        const map_f4 d = ld4(pb + (long)f * p.vb.sc) - ld4(pa + (long)f * p.va.sc);
        ss += d * d;
      }
      map_f4 r;
      r[0] = dist_of(ss[0]); r[1] = dist_of(ss[1]); r[2] = dist_of(ss[2]); r[3] = dist_of(ss[3]);
      *reinterpret_cast<map_f4*>(po) = r;
    } else {
      const unsigned nv = min(4u, p.w - q.x0);
      for (unsigned e = 0; e < nv; ++e) {
        float ss = 0.f;
        for (unsigned f = 0; f < p.F; ++f) {
          const float d = pb[(long)f * p.vb.sc + e] - pa[(long)f * p.va.sc + e];
          ss += d * d;
        }
        po[e] = dist_of(ss);
      }
    }
  }
}

// -(target - pred) / out * dout, an exact 0 where the map is 0 (or not a number)
__device__ __forceinline__ float dist_grad(float d, float o, float g) {
  return o > 0.f ? (-d / o) * g : 0.f;
}

template <bool ACCA, bool ACCB>
__global__ __launch_bounds__(256) void e2map_fdist_bwd_kernel(MapP p) {
  const bool wa = p.da != nullptr, wb = p.db != nullptr;
  const unsigned step = gridDim.x * 256u;
  for (unsigned s = blockIdx.x * 256u + threadIdx.x; s < p.items; s += step) {
    const MPos q = locate(p, s);
    const float* pa = p.a + voff(p.va, q);
    const float* pb = p.b + voff(p.vb, q);
    const float* po = p.o + voff(p.vo, q);
    const float* pg = p.g + voff(p.vg, q);
    float* da = wa ? p.da + voff(p.vda, q) : nullptr;
    float* db = wb ? p.db + voff(p.vdb, q) : nullptr;
    const uintptr_t al = ((uintptr_t)pa) | ((uintptr_t)pb) | ((uintptr_t)po) | ((uintptr_t)pg) |
                         ((uintptr_t)da) | ((uintptr_t)db);
    if (whole(p, q, al)) {
      const map_f4 o = ld4(po), g = ld4(pg);
      for (unsigned f = 0; f < p.F; ++f) {
        const map_f4 d = ld4(pb + (long)f * p.vb.sc) - ld4(pa + (long)f * p.va.sc);
        map_f4 r;
        r[0] = dist_grad(d[0], o[0], g[0]); r[1] = dist_grad(d[1], o[1], g[1]);
        r[2] = dist_grad(d[2], o[2], g[2]); r[3] = dist_grad(d[3], o[3], g[3]);
        if (wa) st4(da + (long)f * p.vda.sc, r, ACCA);
        if (wb) st4(db + (long)f * p.vdb.sc, -r, ACCB);
      }
    } else {
      const unsigned nv = min(4u, p.w - q.x0);
      for (unsigned e = 0; e < nv; ++e) {
        const float o = po[e], g = pg[e];
        for (unsigned f = 0; f < p.F; ++f) {
          const float d = pb[(long)f * p.vb.sc + e] - pa[(long)f * p.va.sc + e];
          const float r = dist_grad(d, o, g);
          if (wa) {
            float* t = da + (long)f * p.vda.sc + e;
            *t = ACCA ? *t + r : r;
          }
          if (wb) {
            float* t = db + (long)f * p.vdb.sc + e;
            *t = ACCB ? *t - r : -r;
          }
        }
      }
    }
  }
}

// ---- RampLoss ------------------------------------------------------------------------------
// r = d_low - d_big + margin with r < 0 -> 0, then NaN -> 0
__device__ __forceinline__ float ramp_of(float lo, float big, float m) {
  const float r = (lo - big) + m;
  return r >= 0.f ? r : 0.f;
}
// the slope of ramp_of wrt d_low: 1 where r >= 0 (r == 0 included, a NaN r not)
__device__ __forceinline__ float ramp_slope(float lo, float big, float m, float g) {
  const float r = (lo - big) + m;
  return r >= 0.f ? g : 0.f;
}

__global__ __launch_bounds__(256) void e2map_ramp_fwd_kernel(MapP p) {
  const float m = e2_uniform_ld(p.scalar, 0);
  const float nf = (float)p.F;
  const unsigned step = gridDim.x * 256u;
  for (unsigned s = blockIdx.x * 256u + threadIdx.x; s < p.items; s += step) {
    const MPos q = locate(p, s);
    const float* pa = p.a + voff(p.va, q);
    const float* pb = p.b + voff(p.vb, q);
    float* po = p.out + voff(p.vout, q);
    if (whole(p, q, ((uintptr_t)pa) | ((uintptr_t)pb) | ((uintptr_t)po))) {
      map_f4 acc = {0.f, 0.f, 0.f, 0.f};
      for (unsigned f = 0; f < p.F; ++f) {
        const map_f4 lo = ld4(pa + (long)f * p.va.sc), big = ld4(pb + (long)f * p.vb.sc);
        acc[0] += ramp_of(lo[0], big[0], m); acc[1] += ramp_of(lo[1], big[1], m);
        acc[2] += ramp_of(lo[2], big[2], m); acc[3] += ramp_of(lo[3], big[3], m);
      }
      *reinterpret_cast<map_f4*>(po) = acc / nf;
    } else {
      const unsigned nv = min(4u, p.w - q.x0);
      for (unsigned e = 0; e < nv; ++e) {
        float acc = 0.f;
        for (unsigned f = 0; f < p.F; ++f)
          acc += ramp_of(pa[(long)f * p.va.sc + e], pb[(long)f * p.vb.sc + e], m);
        po[e] = acc / nf;
      }
    }
  }
}

template <bool ACCA, bool ACCB>
__global__ __launch_bounds__(256) void e2map_ramp_bwd_kernel(MapP p) {
  const float m = e2_uniform_ld(p.scalar, 0);
  const float nf = (float)p.F;
  const bool wa = p.da != nullptr, wb = p.db != nullptr;
  const unsigned step = gridDim.x * 256u;
  for (unsigned s = blockIdx.x * 256u + threadIdx.x; s < p.items; s += step) {
    const MPos q = locate(p, s);
    const float* pa = p.a + voff(p.va, q);
    const float* pb = p.b + voff(p.vb, q);
    const float* pg = p.g + voff(p.vg, q);
    float* da = wa ? p.da + voff(p.vda, q) : nullptr;
    float* db = wb ? p.db + voff(p.vdb, q) : nullptr;
    const uintptr_t al = ((uintptr_t)pa) | ((uintptr_t)pb) | ((uintptr_t)pg) | ((uintptr_t)da) |
                         ((uintptr_t)db);
    if (whole(p, q, al)) {
      const map_f4 g = ld4(pg) / nf;
      for (unsigned f = 0; f < p.F; ++f) {
        const map_f4 lo = ld4(pa + (long)f * p.va.sc), big = ld4(pb + (long)f * p.vb.sc);
        map_f4 r;
        r[0] = ramp_slope(lo[0], big[0], m, g[0]); r[1] = ramp_slope(lo[1], big[1], m, g[1]);
        r[2] = ramp_slope(lo[2], big[2], m, g[2]); r[3] = ramp_slope(lo[3], big[3], m, g[3]);
        if (wa) st4(da + (long)f * p.vda.sc, r, ACCA);
        if (wb) st4(db + (long)f * p.vdb.sc, -r, ACCB);
      }
    } else {
      const unsigned nv = min(4u, p.w - q.x0);
      for (unsigned e = 0; e < nv; ++e) {
        const float g = pg[e] / nf;
        for (unsigned f = 0; f < p.F; ++f) {
          const float r = ramp_slope(pa[(long)f * p.va.sc + e], pb[(long)f * p.vb.sc + e], m, g);
          if (wa) {
            float* t = da + (long)f * p.vda.sc + e;
            *t = ACCA ? *t + r : r;
          }
          if (wb) {
            float* t = db + (long)f * p.vdb.sc + e;
            *t = ACCB ? *t - r : -r;
          }
        }
      }
    }
  }
}

// ---- the mean of a map as a term of the mix ----------------------------------------------------
__global__ __launch_bounds__(256) void e2map_mean_fwd_kernel(MapP p) {
  __shared__ float red[4][2];
  float s1 = 0.f, cnt = 0.f;
  const unsigned step = gridDim.x * 256u;
  for (unsigned s = blockIdx.x * 256u + threadIdx.x; s < p.items; s += step) {
    const MPos q = locate(p, s);
    const float* pa = p.a + voff(p.va, q);
    if (whole(p, q, (uintptr_t)pa)) {
      for (unsigned f = 0; f < p.F; ++f) {
        const map_f4 v = ld4(pa + (long)f * p.va.sc);
        s1 += (v[0] + v[1]) + (v[2] + v[3]);
        cnt += 4.f;
      }
    } else {
      const unsigned nv = min(4u, p.w - q.x0);
      for (unsigned f = 0; f < p.F; ++f)
        for (unsigned e = 0; e < nv; ++e) {
          s1 += pa[(long)f * p.va.sc + e];
          cnt += 1.f;
        }
    }
  }
  s1 = wave_sum(s1);
  cnt = wave_sum(cnt);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) { red[wave][0] = s1; red[wave][1] = cnt; }
  __syncthreads();
  if (threadIdx.x == 0) {
    map_f4 r;
    r[0] = (red[0][0] + red[1][0]) + (red[2][0] + red[3][0]);
    r[1] = (red[0][1] + red[1][1]) + (red[2][1] + red[3][1]);
    r[2] = 0.f;
    r[3] = 0.f;
    *reinterpret_cast<map_f4*>(p.partials + 4l * blockIdx.x) = r;
  }
}

template <bool ACC>
__global__ __launch_bounds__(256) void e2map_mean_bwd_kernel(MapP p) {
  const float co = e2_uniform_ld(p.scalar, 0);
  const map_f4 c4 = {co, co, co, co};
  const unsigned step = gridDim.x * 256u;
  for (unsigned s = blockIdx.x * 256u + threadIdx.x; s < p.items; s += step) {
    const MPos q = locate(p, s);
    float* da = p.da + voff(p.vda, q);
    if (whole(p, q, (uintptr_t)da)) {
      for (unsigned f = 0; f < p.F; ++f) st4(da + (long)f * p.vda.sc, c4, ACC);
    } else {
      const unsigned nv = min(4u, p.w - q.x0);
      for (unsigned f = 0; f < p.F; ++f)
        for (unsigned e = 0; e < nv; ++e) {
          float* t = da + (long)f * p.vda.sc + e;
          *t = ACC ? *t + co : co;
        }
    }
  }
}

// ---- OneHot --------------------------------------------------------------------------------
// out[n,k,..] = (id == k) ? 1 : 0, equality exact: a negative, fractional or NaN id, or one >=
// n_class, gives a column of zeros.  One read of a quad of ids, n_class quad stores.
__global__ __launch_bounds__(256) void e2map_onehot_kernel(MapP p) {
  const unsigned step = gridDim.x * 256u;
  for (unsigned s = blockIdx.x * 256u + threadIdx.x; s < p.items; s += step) {
    const MPos q = locate(p, s);
    const float* pa = p.a + voff(p.va, q);
    float* po = p.out + voff(p.vout, q);
    if (whole(p, q, ((uintptr_t)pa) | ((uintptr_t)po))) {
      const map_f4 id = ld4(pa);
      for (unsigned f = 0; f < p.F; ++f) {
        const float k = (float)f;
        map_f4 r;
        r[0] = id[0] == k ? 1.f : 0.f; r[1] = id[1] == k ? 1.f : 0.f;
        r[2] = id[2] == k ? 1.f : 0.f; r[3] = id[3] == k ? 1.f : 0.f;
        *reinterpret_cast<map_f4*>(po + (long)f * p.vout.sc) = r;
      }
    } else {
      const unsigned nv = min(4u, p.w - q.x0);
      for (unsigned e = 0; e < nv; ++e) {
        const float id = pa[e];
        for (unsigned f = 0; f < p.F; ++f) po[(long)f * p.vout.sc + e] = id == (float)f ? 1.f : 0.f;
      }
    }
  }
}

// ---- host ----------------------------------------------------------------------------------
#define E2_MAP_CAP 4096u        /* work-groups of a map launch; the kernels grid-stride beyond */

// One view of a launch: its tensor, where its strides go, and whether it carries the F features
// (else exactly one).
struct MArg {
  const e2_tensor5* t;
  MView* v;
  bool wide;
};

// collapse over the views: the row absorbs y, then z, where that axis is dense in ALL views; the
// axes left over and the batch axis keep their strides.  Sizes: every view has the extents of
// a[0]; a wide view has F features, the others one.
int map_geometry(const MArg* a, int nv, int F, MapP& p, const char* who) {
  const e2_tensor5* t = a[0].t;
  E2_REQUIRE(F > 0, "%s: no features", who);
  for (int k = 0; k < nv; ++k) {
    const e2_tensor5* u = a[k].t;
    E2_REQUIRE(u->n > 0 && u->c > 0 && u->d > 0 && u->h > 0 && u->w > 0,
               "%s: empty tensor (%d,%d,%d,%d,%d)", who, u->n, u->c, u->d, u->h, u->w);
    E2_REQUIRE(same_extents(t, u) && u->c == (a[k].wide ? F : 1), "%s: size mismatch", who);
  }
  const unsigned long long ext[3] = {(unsigned long long)t->h, (unsigned long long)t->d,
                                     (unsigned long long)t->n};
  long st[8][3];
  for (int k = 0; k < nv; ++k) {
    st[k][0] = (long)a[k].t->sh; st[k][1] = (long)a[k].t->sd; st[k][2] = (long)a[k].t->sn;
  }
  unsigned long long w = (unsigned long long)t->w;
  int first = 0;                     // first axis that stays outside the row (the batch axis always does)
  while (first < 2) {
    bool join = true;
    for (int k = 0; k < nv; ++k) join = join && (ext[first] == 1 || st[k][first] == (long)w);
    if (!join || w * ext[first] >= (1ull << 31)) break;
    w *= ext[first];
    ++first;
  }
  unsigned long long e[3] = {1, 1, 1}, rows = 1;
  for (int x = first; x < 3; ++x) { e[x - first] = ext[x]; rows *= ext[x]; }
  const unsigned long long quads = (w + 3) / 4, items = rows * quads;
  E2_REQUIRE(w < (1ull << 31) && items < (1ull << 31), "%s: tensor too large", who);
  unsigned fbits = 0;
  for (int k = 0; k < nv; ++k) {
    for (int x = 0; x < 3; ++x) a[k].v->s[x] = x + first < 3 ? st[k][x + first] : 0;
    a[k].v->sc = (long)a[k].t->sc;
    if (a[k].wide && F > 1) fbits |= (unsigned)(((unsigned long long)a[k].t->sc << 2) & 15ull);
  }
  p.w = (unsigned)w; p.quads = (unsigned)quads; p.items = (unsigned)items;
  p.e0 = (unsigned)e[0]; p.e1 = (unsigned)e[1];
  p.F = (unsigned)F; p.fbits = fbits;
  p.dq = mk_div(p.quads); p.d0 = mk_div(p.e0); p.d1 = mk_div(p.e1);
  return 0;
}

unsigned map_wgs(const MapP& p) {
  const unsigned g = (p.items + 255u) / 256u;
  return g < 1u ? 1u : (g > E2_MAP_CAP ? E2_MAP_CAP : g);
}

bool given(const e2_tensor5* t) { return t && t->ptr; }

// the four (accumulate a, accumulate b) instances of a backward kernel
#define E2_MAP_LAUNCH_BWD(kernel, ctx, p, acca, accb)                                              \
  do {                                                                                             \
    const dim3 g_(map_wgs(p)), b_(256);                                                            \
    if ((acca) && (accb)) hipLaunchKernelGGL((kernel<true, true>), g_, b_, 0, (ctx)->stream, p);   \
    else if (acca) hipLaunchKernelGGL((kernel<true, false>), g_, b_, 0, (ctx)->stream, p);         \
    else if (accb) hipLaunchKernelGGL((kernel<false, true>), g_, b_, 0, (ctx)->stream, p);         \
    else hipLaunchKernelGGL((kernel<false, false>), g_, b_, 0, (ctx)->stream, p);                  \
  } while (0)

}  // namespace

extern "C" int e2_fdist_fwd(e2_ctx* ctx, const e2_tensor5* pred, const e2_tensor5* target,
                            const e2_tensor5* out) {
  E2_REQUIRE(ctx && given(pred) && given(target) && given(out), "e2_fdist_fwd: null argument");
  MapP p = MapP{};
  const MArg a[3] = {{pred, &p.va, true}, {target, &p.vb, true}, {out, &p.vout, false}};
  if (int rc = map_geometry(a, 3, pred->c, p, "e2_fdist_fwd")) return rc;
  p.a = pred->ptr; p.b = target->ptr; p.out = out->ptr;
  hipLaunchKernelGGL(e2map_fdist_fwd_kernel, dim3(map_wgs(p)), dim3(256), 0, ctx->stream, p);
  E2_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" int e2_fdist_bwd(e2_ctx* ctx, const e2_tensor5* pred, const e2_tensor5* target,
                            const e2_tensor5* out, const e2_tensor5* dout, const e2_tensor5* dpred,
                            const e2_tensor5* dtarget, int acc_pred, int acc_target) {
  E2_REQUIRE(ctx && given(pred) && given(target) && given(out) && given(dout),
             "e2_fdist_bwd: null argument");
  const bool wa = given(dpred), wb = given(dtarget);
  E2_REQUIRE(wa || wb, "e2_fdist_bwd: no gradient view given");
  MapP p = MapP{};
  MArg a[6] = {{pred, &p.va, true}, {target, &p.vb, true}, {out, &p.vo, false},
               {dout, &p.vg, false}};
  int nv = 4;
  if (wa) a[nv++] = MArg{dpred, &p.vda, true};
  if (wb) a[nv++] = MArg{dtarget, &p.vdb, true};
  if (int rc = map_geometry(a, nv, pred->c, p, "e2_fdist_bwd")) return rc;
  p.a = pred->ptr; p.b = target->ptr; p.o = out->ptr; p.g = dout->ptr;
  p.da = wa ? dpred->ptr : nullptr; p.db = wb ? dtarget->ptr : nullptr;
  E2_MAP_LAUNCH_BWD(e2map_fdist_bwd_kernel, ctx, p, acc_pred != 0, acc_target != 0);
  E2_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" int e2_ramp_fwd(e2_ctx* ctx, const e2_tensor5* d_low, const e2_tensor5* d_big,
                           const float* margin, const e2_tensor5* out) {
  E2_REQUIRE(ctx && given(d_low) && given(d_big) && margin && given(out),
             "e2_ramp_fwd: null argument");
  MapP p = MapP{};
  const MArg a[3] = {{d_low, &p.va, true}, {d_big, &p.vb, true}, {out, &p.vout, false}};
  if (int rc = map_geometry(a, 3, d_low->c, p, "e2_ramp_fwd")) return rc;
  p.a = d_low->ptr; p.b = d_big->ptr; p.out = out->ptr; p.scalar = margin;
  hipLaunchKernelGGL(e2map_ramp_fwd_kernel, dim3(map_wgs(p)), dim3(256), 0, ctx->stream, p);
  E2_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" int e2_ramp_bwd(e2_ctx* ctx, const e2_tensor5* d_low, const e2_tensor5* d_big,
                           const float* margin, const e2_tensor5* dout, const e2_tensor5* dd_low,
                           const e2_tensor5* dd_big, int acc_low, int acc_big) {
  E2_REQUIRE(ctx && given(d_low) && given(d_big) && margin && given(dout),
             "e2_ramp_bwd: null argument");
  const bool wa = given(dd_low), wb = given(dd_big);
  E2_REQUIRE(wa || wb, "e2_ramp_bwd: no gradient view given");
  MapP p = MapP{};
  MArg a[5] = {{d_low, &p.va, true}, {d_big, &p.vb, true}, {dout, &p.vg, false}};
  int nv = 3;
  if (wa) a[nv++] = MArg{dd_low, &p.vda, true};
  if (wb) a[nv++] = MArg{dd_big, &p.vdb, true};
  if (int rc = map_geometry(a, nv, d_low->c, p, "e2_ramp_bwd")) return rc;
  p.a = d_low->ptr; p.b = d_big->ptr; p.g = dout->ptr; p.scalar = margin;
  p.da = wa ? dd_low->ptr : nullptr; p.db = wb ? dd_big->ptr : nullptr;
  E2_MAP_LAUNCH_BWD(e2map_ramp_bwd_kernel, ctx, p, acc_low != 0, acc_big != 0);
  E2_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" int e2_onehot(e2_ctx* ctx, const e2_tensor5* target, int n_class,
                         const e2_tensor5* out) {
  E2_REQUIRE(ctx && given(target) && given(out), "e2_onehot: null argument");
  E2_REQUIRE(n_class >= 1 && n_class < (1 << 24), "e2_onehot: %d classes", n_class);
  MapP p = MapP{};
  const MArg a[2] = {{target, &p.va, false}, {out, &p.vout, true}};
  if (int rc = map_geometry(a, 2, n_class, p, "e2_onehot")) return rc;
  p.a = target->ptr; p.out = out->ptr;
  hipLaunchKernelGGL(e2map_onehot_kernel, dim3(map_wgs(p)), dim3(256), 0, ctx->stream, p);
  E2_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" int e2_mean_fwd(e2_ctx* ctx, const e2_tensor5* x, float* partials) {
  E2_REQUIRE(ctx && given(x) && partials, "e2_mean_fwd: null argument");
  E2_REQUIRE((((uintptr_t)partials) & 15) == 0, "e2_mean_fwd: partials must be 16-byte aligned");
  MapP p = MapP{};
  const MArg a[1] = {{x, &p.va, true}};
  if (int rc = map_geometry(a, 1, x->c, p, "e2_mean_fwd")) return rc;
  p.a = x->ptr; p.partials = partials;
  // one row per work-group, as many as the mix will read for a term of these sizes
  const unsigned wgs = (unsigned)e2_loss_partials(ctx, x);
  E2_REQUIRE(wgs >= 1, "e2_mean_fwd: empty tensor");
  hipLaunchKernelGGL(e2map_mean_fwd_kernel, dim3(wgs), dim3(256), 0, ctx->stream, p);
  E2_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" int e2_mean_bwd(e2_ctx* ctx, const float* coef, const e2_tensor5* dx, int accumulate) {
  E2_REQUIRE(ctx && coef && given(dx), "e2_mean_bwd: null argument");
  MapP p = MapP{};
  const MArg a[1] = {{dx, &p.vda, true}};
  if (int rc = map_geometry(a, 1, dx->c, p, "e2_mean_bwd")) return rc;
  p.da = dx->ptr; p.scalar = coef;
  const dim3 g(map_wgs(p)), b(256);
  if (accumulate) hipLaunchKernelGGL((e2map_mean_bwd_kernel<true>), g, b, 0, ctx->stream, p);
  else hipLaunchKernelGGL((e2map_mean_bwd_kernel<false>), g, b, 0, ctx->stream, p);
  E2_CHECK_HIP(hipGetLastError());
  return 0;
}
